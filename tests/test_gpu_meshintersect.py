"""csrc/meshintersect.hip on the GPU: hits, count, sorted pairs and degenerate flags equal to the numpy restatement
tests/meshintersect_ref.py, through the raw C ABI in the order given and through surfd_amd.meshintersect, culled and brute
force, on every mesh of the contract's table, on each side of the kernel's tile (32), chunk (256) and split (64 chunks)
boundaries; independence of order, the capacity rule, two meshes, the refusals, the culling counter and the drivers."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshintersect_ref as mr  # noqa: E402
import mesh_udf_ref  # noqa: E402
import raycast_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L18 = mr.LATTICE
SENTINEL = -0x0123456789ABCDEF
ERR_ARG = -1


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def unpack(keys):
    keys = np.sort(np.asarray(keys, np.int64))
    return np.stack([keys >> 32, keys & 0xFFFFFFFF], 1).reshape(-1, 2)


class Raw:
    """the C ABI as it is: triangles in the order given (the Python wrapper sorts them)"""

    def __init__(self, v, f, L=L18):
        from surfd_amd import _native as N
        self.N, self.F = N, len(f)
        self.v, self.f = cu(np.asarray(v, np.float32)), cu(f, torch.int32)
        self.h = C.c_void_p()
        N.check(N.lib().surfd_isect_create(N.ptr(self.v), len(v), N.ptr(self.f), len(f), L, N.stream(), C.byref(self.h)))
        assert N.lib().surfd_isect_num_triangles(self.h) == len(f)

    def _call(self, other, flags, capacity, tail=16):
        N = self.N
        hits_a = torch.full((self.F,), -7, device="cuda", dtype=torch.int32)
        hits_b = None if other is None else torch.full((other.F,), -7, device="cuda", dtype=torch.int32)
        count = torch.full((1,), -7, device="cuda", dtype=torch.int64)
        keys = torch.full((capacity + tail,), SENTINEL, device="cuda", dtype=torch.int64)
        if other is None:
            N.check(N.lib().surfd_isect_self(self.h, flags, N.ptr(hits_a), N.ptr(keys), capacity, N.ptr(count), N.stream()))
        else:
            N.check(N.lib().surfd_isect_between(self.h, other.h, flags, N.ptr(hits_a), N.ptr(hits_b), N.ptr(keys), capacity, N.ptr(count),
                                                N.stream()))
        torch.cuda.synchronize()
        keys, n = keys.cpu().numpy(), int(count)
        assert (keys[capacity:] == SENTINEL).all(), "a key was written beyond the capacity"
        assert (keys[min(n, capacity):] == SENTINEL).all() and (keys[:min(n, capacity)] != SENTINEL).all()
        out = dict(count=n, hits=hits_a.cpu().numpy(), keys=keys[:min(n, capacity)])
        if other is not None:
            out.update(hits_a=out.pop("hits"), hits_b=hits_b.cpu().numpy())
        return out

    def self_pairs(self, flags=0, capacity=4096):
        return self._call(None, flags, capacity)

    def between(self, other, flags=0, capacity=4096):
        return self._call(other, flags, capacity)

    def counting(self, flags=0):
        N = self.N
        count = torch.full((1,), -7, device="cuda", dtype=torch.int64)
        N.check(N.lib().surfd_isect_self(self.h, flags, None, None, 0, N.ptr(count), N.stream()))
        return int(count)

    def degenerate(self):
        N = self.N
        flags = torch.full((self.F,), 9, device="cuda", dtype=torch.uint8)
        count = torch.full((1,), -7, device="cuda", dtype=torch.int64)
        N.check(N.lib().surfd_isect_degenerate(self.h, N.ptr(flags), N.ptr(count), N.stream()))
        return flags.cpu().numpy(), int(count)

    def skipped(self):
        s, t = C.c_int64(), C.c_int64()
        self.N.check(self.N.lib().surfd_isect_skipped(self.h, C.byref(s), C.byref(t), self.N.stream()))
        return int(s.value), int(t.value)

    def __del__(self):
        self.N.lib().surfd_isect_destroy(self.h)


def same_as_reference(got, ref, what):
    assert got["count"] == ref["count"], (what, got["count"], ref["count"])
    assert got["hits"].dtype == np.int32 and np.array_equal(got["hits"], ref["hits"]), (what, "hits")
    assert np.array_equal(unpack(got["keys"]), ref["pairs"]), (what, "pairs")


def wrapper_equals(v, f, ref, what, **kw):
    from surfd_amd.meshintersect import IntersectionScene
    r = IntersectionScene(cu(np.asarray(v, np.float32)), cu(f), L18).self_intersections(**kw)
    assert r["count"] == ref["count"] and isinstance(r["count"], int), what
    assert r["hits"].dtype == torch.int32 and np.array_equal(r["hits"].cpu().numpy(), ref["hits"]), what
    assert r["faces"].dtype == torch.bool and np.array_equal(r["faces"].cpu().numpy(), ref["hits"] > 0), what
    assert r["degenerate"].dtype == torch.bool and np.array_equal(r["degenerate"].cpu().numpy(), ref["degenerate"]), what
    assert r["pairs"].dtype == torch.int64 and np.array_equal(r["pairs"].cpu().numpy().reshape(-1, 2), ref["pairs"]), what
    solid = int((~ref["degenerate"]).sum())
    assert isinstance(r["fraction"], float) and r["fraction"] == (int((ref["hits"] > 0).sum()) / solid if solid else 0.0), what
    return r


# ---- the cases: name -> mesh; the reference of each is computed once ------------------------------------------------------------------
BOUNDARY_F = (1, 2, 31, 32, 33, 255, 256, 257, 511, 513)


def _cases():
    out = {f"table-{name}": make() for name, (make, _, _) in mr.TABLE.items()}
    v, f = mr.interleaved_spheres()
    for F in BOUNDARY_F:                                                # each side of a tile and of a chunk
        out[f"F-{F}"] = (v, f[:F])
    out["F-17153"] = mr.torus_with_patch()                              # 67 chunks: two chunks per split, every split boundary crossed
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    return mr.result(*CASES[name], L18)


# ---- 1, 2: equality with the restatement, culled and brute force --------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_restatement(name):
    v, f = CASES[name]
    ref = reference(name)
    scene = Raw(v, f)
    same_as_reference(scene.self_pairs(flags=1), ref, f"{name}, brute force")
    same_as_reference(scene.self_pairs(flags=0), ref, f"{name}, culled")
    assert scene.counting(0) == scene.counting(1) == ref["count"]       # the counting form: no hits, no pairs
    flags, n = scene.degenerate()
    assert np.array_equal(flags, ref["degenerate"].astype(np.uint8)) and n == int(ref["degenerate"].sum())
    wrapper_equals(v, f, ref, f"{name}, wrapper")
    wrapper_equals(v, f, ref, f"{name}, wrapper, brute force", brute_force=True)
    print(f"{name}: F = {len(f)}, {ref['count']} pairs, {int((ref['hits'] > 0).sum())} faces, {int(ref['degenerate'].sum())} degenerate")
    if name.startswith("table-"):
        assert (ref["count"], int(ref["degenerate"].sum())) == mr.TABLE[name[6:]][1:]
    if name == "F-17153":
        assert ref["count"] > 0 and (ref["pairs"][:, 1] >= 16896).all()  # the patch against the torus, nothing else
        # the same faces in random order: the intersecting pairs now lie in chunks all over the range, in many splits
        perm = np.random.default_rng(20).permutation(len(f))
        got = Raw(v, f[perm]).self_pairs()
        back = np.sort(perm[unpack(got["keys"])], 1)
        assert got["count"] == ref["count"] and np.array_equal(back[np.lexsort((back[:, 1], back[:, 0]))], ref["pairs"])
        assert len(set((unpack(got["keys"])[:, 1] // 256 // 2).tolist())) > 3          # partners in more than three splits
    if name == "F-513":
        p = ref["pairs"]
        assert (p[:, 0] // 32 == p[:, 1] // 32).any() and (p[:, 0] // 32 != p[:, 1] // 32).any() and (p[:, 0] // 256 != p[:, 1] // 256).any()


# ---- 3: independence of order, stability ------------------------------------------------------------------------------------------
def test_independent_of_face_order_and_corner_rotation():
    v, f = CASES["table-two_spheres"]
    ref = reference("table-two_spheres")
    rng = np.random.default_rng(21)
    perm = rng.permutation(len(f))
    g = np.stack([np.roll(f[p], rng.integers(0, 3)) for p in perm])
    got = Raw(v, g).self_pairs()
    back = np.sort(perm[unpack(got["keys"])], 1)
    back = back[np.lexsort((back[:, 1], back[:, 0]))]
    assert got["count"] == 88 and np.array_equal(back, ref["pairs"])
    hits = np.zeros(len(f), np.int32)
    hits[perm] = got["hits"]
    assert np.array_equal(hits, ref["hits"])
    wrapper_equals(v, g, dict(ref, pairs=mr.result(v, g, L18)["pairs"], hits=got["hits"]), "permuted, wrapper")


def test_two_repeats_give_identical_buffers():
    scene = Raw(*CASES["F-17153"])
    first = scene.self_pairs()
    again = scene.self_pairs()
    assert first["count"] == again["count"] and np.array_equal(first["hits"], again["hits"])
    assert np.array_equal(np.sort(first["keys"]), np.sort(again["keys"]))          # the order of the keys is not specified


# ---- 4: capacity ------------------------------------------------------------------------------------------------------------------
def test_capacity_bounds_the_writes_and_not_the_count():
    v, f = CASES["table-two_spheres"]
    ref = reference("table-two_spheres")
    truth = {(int(a), int(b)) for a, b in ref["pairs"]}
    scene = Raw(v, f)
    for capacity in (1, 10, 87, 88):
        for flags in (0, 1):
            got = scene.self_pairs(flags=flags, capacity=capacity)      # the sentinel tail is checked inside
            assert got["count"] == 88 and len(got["keys"]) == capacity
            assert np.array_equal(got["hits"], ref["hits"])
            keys = {(int(a), int(b)) for a, b in unpack(got["keys"])}
            assert len(keys) == capacity and keys <= truth
    from surfd_amd import _native as N
    assert N.lib().surfd_isect_self(scene.h, 0, None, None, 5, None, N.stream()) == ERR_ARG        # a capacity without a buffer
    assert N.lib().surfd_isect_self(scene.h, 0, None, None, -1, None, N.stream()) == ERR_ARG
    assert N.lib().surfd_isect_self(scene.h, 4, None, None, 0, None, N.stream()) == ERR_ARG         # an unknown flag
    wrapper_equals(v, f, ref, "wrapper, one re-call", capacity=7)


# ---- 5: two meshes ----------------------------------------------------------------------------------------------------------------
def test_between_two_meshes():
    from surfd_amd import _native as N
    from surfd_amd.meshintersect import IntersectionScene, mesh_intersections
    a = rr.icosphere(2, 0.75)
    b = mr.shifted(a, (0.5, 0.0625, 0.03125))
    ref = mr.result_between(*a, *b, L18)
    assert ref["count"] == 88
    ra, rb = Raw(*a), Raw(*b)
    for flags in (0, 1):
        got = ra.between(rb, flags=flags)
        assert got["count"] == 88 and np.array_equal(unpack(got["keys"]), ref["pairs"])
        assert np.array_equal(got["hits_a"], ref["hits_a"]) and np.array_equal(got["hits_b"], ref["hits_b"])
        back = rb.between(ra, flags=flags)
        flipped = unpack(back["keys"])[:, ::-1]
        assert np.array_equal(flipped[np.lexsort((flipped[:, 1], flipped[:, 0]))], ref["pairs"])
        assert np.array_equal(back["hits_a"], ref["hits_b"]) and np.array_equal(back["hits_b"], ref["hits_a"])
    # no sharing rule between meshes: a cube against a copy that touches it in one corner only
    cube = rr.cube()
    corner = mr.shifted(cube, (1.0, 1.0, 1.0))
    cref = mr.result_between(*cube, *corner, L18)
    got = Raw(*cube).between(Raw(*corner))
    assert cref["count"] == 36 and got["count"] == 36 and np.array_equal(unpack(got["keys"]), cref["pairs"])     # 6 x 6 faces at the corner
    # the wrapper, both directions, and the module function with its own lattice (18 for both meshes together)
    sa, sb = IntersectionScene(cu(a[0]), cu(a[1]), L18), IntersectionScene(cu(b[0]), cu(b[1]), L18)
    ab, ba = sa.intersections(sb), sb.intersections(sa, brute_force=True)
    auto = mesh_intersections(cu(a[0]), cu(a[1]), cu(b[0]), cu(b[1]))
    for r in (ab, auto):
        assert r["count"] == 88 and np.array_equal(r["pairs"].cpu().numpy(), ref["pairs"])
        assert np.array_equal(r["hits_a"].cpu().numpy(), ref["hits_a"]) and np.array_equal(r["hits_b"].cpu().numpy(), ref["hits_b"])
        assert np.array_equal(r["faces_a"].cpu().numpy(), ref["hits_a"] > 0) and np.array_equal(r["faces_b"].cpu().numpy(), ref["hits_b"] > 0)
        assert r["fraction"] == int((ref["hits_a"] > 0).sum()) / 320
    t = ba["pairs"].cpu().numpy()[:, ::-1]
    assert np.array_equal(t[np.lexsort((t[:, 1], t[:, 0]))], ref["pairs"]) and torch.equal(ba["hits_a"], ab["hits_b"])
    # different lattices
    other = Raw(*b, L=17)
    assert N.lib().surfd_isect_between(ra.h, other.h, 0, None, None, None, 0, None, N.stream()) == ERR_ARG
    assert b"lattice" in N.lib().surfd_last_error()
    with pytest.raises(RuntimeError, match="lattice"):
        sa.intersections(IntersectionScene(cu(b[0]), cu(b[1]), 17))


# ---- 6: refusals are errors, never faults ---------------------------------------------------------------------------------------
def test_refusals():
    from surfd_amd import _native as N
    from surfd_amd import meshintersect
    lib = N.lib()
    v, f = rr.cube()

    def create(v, f, L=L18, F=None):
        h = C.c_void_p()
        vt, ft = cu(np.asarray(v, np.float32)), cu(f, torch.int32)
        rc = lib.surfd_isect_create(N.ptr(vt), len(v), N.ptr(ft), len(f) if F is None else F, L, N.stream(), C.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            lib.surfd_isect_destroy(h)
        return rc, lib.surfd_last_error() or b""

    assert create(v, f)[0] == 0
    for bad in (len(v), -1, 2 ** 31 - 1):
        g = f.copy()
        g[7, 1] = bad
        rc, msg = create(v, g)
        assert rc == ERR_ARG and b"outside [0, 8)" in msg
    for value, where in ((np.nan, [(3, 1)]), (np.inf, [(0, 0), (1, 2)]), (2.0 + 2.0 ** -17, [(5, 2), (6, 0), (7, 1)])):   # 2 * 2^18 = 2^19 is the last one inside
        w = v.copy()
        for r, c in where:
            w[r, c] = value
        rc, msg = create(w, f)
        assert rc == ERR_ARG and f"{len(where)} of 8 vertices".encode() in msg, msg
    w = v.copy()
    w[5, 2] = 2.0
    assert create(w, f)[0] == 0
    assert create(v, f, F=0)[0] == ERR_ARG
    assert create(v, f, L=101)[0] == ERR_ARG
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshintersect.IntersectionScene(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        meshintersect.mesh_intersections(cu(v), cu(f), torch.from_numpy(v), torch.from_numpy(f))
    # the wrapper hands a bad index and a NaN on to the library, which refuses them
    g = f.copy()
    g[7, 1] = 99
    with pytest.raises(RuntimeError, match="outside"):
        meshintersect.IntersectionScene(cu(v), cu(g), L18)
    w = v.copy()
    w[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="1 of 8 vertices"):
        meshintersect.IntersectionScene(cu(w), cu(f), L18)
    with pytest.raises(ValueError):
        meshintersect.IntersectionScene(cu(w), cu(f))


# ---- 7: culling skips work ----------------------------------------------------------------------------------------------------------
def test_culling_skips_tile_visits_on_the_torus():
    from surfd_amd.meshintersect import IntersectionScene
    v, f = CASES["F-17153"]
    ref = reference("F-17153")
    raw = Raw(v, f)
    same_as_reference(raw.self_pairs(flags=2), ref, "culled, counting the skips")
    skipped, total = raw.skipped()
    waves, tiles = (len(f) + 63) // 64, (len(f) + 31) // 32
    assert total == sum(min(4, waves - 4 * x) * (tiles - 8 * x) for x in range((len(f) + 255) // 256))
    assert 0 < skipped <= total
    raw.self_pairs(flags=3)
    assert raw.skipped() == (0, total)                                   # brute force skips nothing
    scene = IntersectionScene(cu(v), cu(f), L18)
    r = scene.self_intersections(count_skipped=True)
    assert r["count"] == ref["count"] and scene.last_total_tiles == total
    print(f"skipped (wave, tile) visits: {skipped} of {total} in the order given ({skipped / total:.1%}), "
          f"{scene.last_skipped_tiles} in Morton order ({scene.last_skipped_tiles / total:.1%})")
    assert 0 < scene.last_skipped_tiles <= total


# ---- 8: the drivers -----------------------------------------------------------------------------------------------------------------
def test_evaluate_driver(tmp_path):
    from test_gpu_cloudsample import EVAL_ARGS, GOLDEN, make_eval_inputs     # the inputs and the command the golden JSON was written with
    env = dict(os.environ, PYTHONPATH=ROOT)
    script = [sys.executable, os.path.join(ROOT, "examples", "evaluate.py")]
    gen_dir, ref_dir = tmp_path / "one" / "gen", tmp_path / "one" / "ref"
    os.makedirs(gen_dir), os.makedirs(ref_dir)
    mesh_udf_ref.write_obj(gen_dir / "pair.obj", *mr.two_spheres())
    mesh_udf_ref.write_obj(ref_dir / "pair.obj", *rr.icosphere(2, 0.75))
    out = tmp_path / "one.json"
    r = subprocess.run(script + ["--generated", str(gen_dir), "--reference", str(ref_dir), "--paired", "--num_points", "256",
                                 "--self_intersections", "--collisions", "--output", str(out)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = json.load(open(out))
    ref = mr.result(*mr.two_spheres(), L18)
    item = m["items"]["pair"]
    assert item["self_intersecting_pairs"] == 88 and item["degenerate_faces"] == 0
    assert item["self_intersecting_faces"] == int((ref["hits"] > 0).sum()) / 640
    # against the first sphere alone: its own 320 faces coincide with it, and the second sphere's faces that cut it
    assert item["colliding_faces"] == (320 + int((ref["hits"][320:] > 0).sum())) / 640
    assert m["options"]["self_intersections"] is True and m["options"]["collisions"] is True and m["skipped"] == []
    assert m["mean"]["self_intersecting_pairs"] == 88.0 and m["mean"]["colliding_faces"] == item["colliding_faces"]
    # the inputs of the golden file: the default run is byte for byte the parent commit's, the options only add keys, and the
    # .npz item is skipped
    gen_dir, ref_dir = make_eval_inputs(str(tmp_path))
    base = script + ["--generated", gen_dir, "--reference", ref_dir] + EVAL_ARGS

    def call(extra, name):
        r = subprocess.run(base + extra + ["--output", str(tmp_path / name)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.load(open(tmp_path / name)), open(tmp_path / name, "rb").read()

    golden = json.load(open(GOLDEN))
    default, raw = call([], "default.json")
    assert default == golden and raw == json.dumps(golden, indent=1).encode()
    both, _ = call(["--self_intersections", "--collisions"], "both.json")
    assert both["skipped"] == ["item2"] and "self_intersecting_faces" not in both["items"]["item2"]
    for name in ("item0", "item1"):                                       # a box, and the same box stretched along y around it
        it = both["items"][name]
        assert (it.pop("self_intersecting_faces"), it.pop("self_intersecting_pairs"), it.pop("degenerate_faces")) == (0.0, 0, 0)
        assert 0.0 < it.pop("colliding_faces") <= 1.0                     # the faces at +-x and +-z lie in the reference's
    for k in ("self_intersecting_faces", "self_intersecting_pairs", "degenerate_faces", "colliding_faces"):
        both["mean"].pop(k)
    both["options"].pop("self_intersections"), both["options"].pop("collisions"), both.pop("skipped")
    assert both == golden


def test_reconstruct_mesh_quality_adds_its_key(tmp_path):
    from examples.reconstruct import item_metrics
    v, f = mr.two_spheres()
    path = str(tmp_path / "item.npz")
    np.savez(path, vertices=v, triangles=f)
    plain = item_metrics(path, v, f, None, 0)
    more = item_metrics(path, v, f, None, 0, mesh_quality=True)
    ref = mr.result(v, f, L18)
    assert "self_intersecting_faces" not in plain
    assert more.pop("self_intersecting_faces") == int((ref["hits"] > 0).sum()) / 640
    assert more == plain
