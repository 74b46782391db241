"""GPU tests of the mesh renderer (surfd_amd/render.py, csrc/raster.hip) against tests/render_ref.py: the fill, tie and drop
rules on hand-made scenes, the two raster paths against each other, every buffer against the numpy restatement bit for bit,
depth against fp64, the invariances (batch, face order, repetition), contours and the public surface.  Every test fails on a
tree without surfd_amd/render.py.

Tolerance against fp64: `python tests/render_ref.py` measures the restatement's own worst depth deviation
from fp64 on these scenes as 8.87 u of the scene's depth range (u = 2^-24); R.DEPTH_BASE_U = 8.9 and the bound here is 4 x that =
35.6 u.  Nothing is excluded."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
FLOATS = ("depth", "bary", "normal", "shaded")
BUFFERS = ("face", "mask") + FLOATS


@pytest.fixture(scope="module")
def RD():
    from surfd_amd import render
    return render


_renderers = {}


def gpu_render(RD, v, f, cams, H, W, **kw):
    """-> numpy buffers; one Renderer per size is kept and reused across the module"""
    r = _renderers.setdefault((H, W), RD.Renderer((H, W), max_views=8))
    vt = torch.as_tensor(np.asarray(v, np.float32).reshape(-1, 3)).cuda().contiguous()
    ft = torch.as_tensor(np.asarray(f, np.int32).reshape(-1, 3)).cuda().contiguous()
    out = r.render(vt, ft, torch.as_tensor(np.asarray(cams, np.float32)), **kw)
    return {k: t.cpu().numpy() for k, t in out.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(a, b, keys=BUFFERS + ("dropped",)):
    for k in keys:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


_ref_cache = {}


def reference(name):
    """the restatement of one of R.fp64_scenes(), computed once for the module"""
    if not _ref_cache:
        for s in R.fp64_scenes():
            _ref_cache[s[0]] = [s, None]
    ent = _ref_cache[name]
    if ent[1] is None:
        _, v, f, cams, H, W = ent[0]
        ent[1] = R.render_f32(v, f, cams, H, W)
        for a in ent[1].values():
            a.setflags(write=False)
    return ent[0], ent[1]


SCENES = [s[0] for s in R.fp64_scenes()]
PIX = R.pixel_camera()


# ---- rules ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["centres", "corners"])
def test_single_triangle_top_left_rule(RD, where):
    # centres: (1.5, 1.5), (6.5, 1.5), (1.5, 6.5); corners: (1, 1), (7, 1), (1, 7).  In both the top and the left edge own their
    # pixels, and the hypotenuse x + y = 8 runs through the centres with i + j = 7, which it does not own
    v = R.rule_triangle(where)
    g = gpu_render(RD, v, [[0, 1, 2]], PIX, 8, 8)
    j, i = np.mgrid[0:8, 0:8]
    want = (i >= 1) & (j >= 1) & (i + j <= 6)
    assert np.array_equal(g["mask"][0] != 0, want), g["mask"][0]
    assert_same(g, R.render_f32(v, [[0, 1, 2]], PIX, 8, 8))


@pytest.mark.parametrize("w0", [0, 1])
@pytest.mark.parametrize("w1", [0, 1])
def test_shared_edge_is_covered_once(RD, w0, w1):
    v = np.array([[2.5, 3.5, 1], [12.5, 3.5, 1], [12.5, 11.5, 2], [2.5, 11.5, 2]], np.float32)
    t0, t1 = [0, 1, 2], [0, 2, 3]
    f = [t0[::-1] if w0 else t0, t1[::-1] if w1 else t1]
    both = gpu_render(RD, v, f, PIX, 16, 16)
    a = gpu_render(RD, v, f[:1], PIX, 16, 16)["mask"][0] != 0
    b = gpu_render(RD, v, f[1:], PIX, 16, 16)["mask"][0] != 0
    j, i = np.mgrid[0:16, 0:16]
    rect = (i >= 2) & (i <= 11) & (j >= 3) & (j <= 10)          # left and top edge in, right and bottom edge out
    assert not (a & b).any() and np.array_equal(a | b, rect)
    assert np.array_equal(both["mask"][0] != 0, rect)
    assert np.array_equal(both["face"][0] == 0, a) and np.array_equal(both["face"][0] == 1, b)
    assert_same(both, R.render_f32(v, f, PIX, 16, 16))


def test_equal_depth_goes_to_the_lower_face_index(RD):
    # two right triangles with legs of 4 pixels (doubled area 2^20: barycentrics and their sum are exact) in the plane z = 1
    v = np.array([[1, 1, 1], [5, 1, 1], [1, 5, 1], [5, 5, 1]], np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3]], np.int32)
    ref = R.render_f32(v, f, PIX, 8, 8)
    alone = [R.render_f32(v, f[k:k + 1], PIX, 8, 8) for k in (0, 1)]
    overlap = (alone[0]["mask"][0] != 0) & (alone[1]["mask"][0] != 0)
    assert overlap.sum() >= 3
    assert np.array_equal(bits(alone[0]["depth"][0])[overlap], bits(alone[1]["depth"][0])[overlap])      # exact ties
    g = gpu_render(RD, v, f, PIX, 8, 8)
    assert (g["face"][0][overlap] == 0).all()
    h = gpu_render(RD, v, f[::-1].copy(), PIX, 8, 8)
    assert (h["face"][0][overlap] == 0).all()
    assert np.array_equal(bits(g["depth"]), bits(h["depth"])) and np.array_equal(g["mask"], h["mask"])
    only1 = (alone[1]["mask"][0] != 0) & ~overlap
    assert (g["face"][0][only1] == 1).all() and (h["face"][0][only1] == 0).all()
    assert_same(g, ref)


def test_half_off_screen_and_behind_near(RD):
    v = np.array([[-9.25, 3.0, 1], [6.0, -7.5, 2], [5.5, 30.0, 3]], np.float32)
    g = gpu_render(RD, v, [[0, 1, 2]], PIX, 8, 8)
    assert g["dropped"][0] == 0 and 0 < (g["mask"] != 0).sum() < 64
    assert_same(g, R.render_f32(v, [[0, 1, 2]], PIX, 8, 8))
    # perspective: one vertex behind the near plane -> the triangle is dropped and counted, the other one is drawn
    cams = RD.orbit_cameras(1, 0.0, 2.0, size=16, near=0.5).numpy()
    v = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0, 0.5, 0], [0, 0.2, 1.6]], np.float32)    # the last one has camera z = 0.4
    g = gpu_render(RD, v, [[0, 1, 3]], cams, 16, 16)
    assert g["dropped"].tolist() == [1] and not g["mask"].any() and (g["face"] == -1).all() and np.isinf(g["depth"]).all()
    g = gpu_render(RD, v, [[0, 1, 3], [0, 1, 2]], cams, 16, 16)
    assert g["dropped"].tolist() == [1] and g["mask"].any() and set(np.unique(g["face"])) == {-1, 1}
    assert_same(g, R.render_f32(v, [[0, 1, 3], [0, 1, 2]], cams, 16, 16))


def test_empty_meshes(RD):
    for v, f in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), (np.ones((3, 3), np.float32), np.zeros((0, 3), np.int32))):
        g = gpu_render(RD, v, f, np.repeat(PIX, 2, 0), 8, 8)
        assert g["face"].shape == (2, 8, 8) and (g["face"] == -1).all() and not g["mask"].any() and np.isinf(g["depth"]).all()
        assert not g["bary"].any() and not g["normal"].any() and not g["shaded"].any() and g["dropped"].tolist() == [0, 0]


# ---- both paths -----------------------------------------------------------------------------------------------------------------
def _random_triangles(n, lo, hi, seed):
    g = np.random.default_rng(seed)
    c = g.uniform(-2, 66, (n, 1, 2))
    ext = g.uniform(lo, hi, (n, 1, 1))
    xy = c + g.uniform(-0.5, 0.5, (n, 3, 2)) * ext
    z = g.uniform(1, 2, (n, 3, 1))
    return np.concatenate([xy, z], 2).reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


@pytest.mark.parametrize("scene", ["one-large", "sub-pixel", "mix"])
def test_small_and_large_path_agree(RD, scene):
    if scene == "one-large":
        v, f = np.array([[-10, -10, 1], [200, -10, 2], [-10, 200, 3]], np.float32), np.array([[0, 1, 2]], np.int32)
    elif scene == "sub-pixel":
        v, f = _random_triangles(5000, 0.8, 2.0, 1)               # boxes of at most 2 x 2 pixel centres, most of them empty or single
    else:
        v, f = _random_triangles(3000, 1.0, 12.0, 2)             # clipped boxes of 1 .. 144 pixel centres around the threshold of 16
    outs = [gpu_render(RD, v, f, PIX, 64, 64, flags=fl) for fl in (0, RD.FORCE_SMALL, RD.FORCE_LARGE)]
    assert_same(outs[0], outs[1])
    assert_same(outs[0], outs[2])
    covered = int((outs[0]["mask"] != 0).sum())
    assert covered == 64 * 64 if scene == "one-large" else covered > 300
    if scene == "mix":                                            # the threshold is really straddled
        sx, sy, valid, _, _ = R.project_f32(v, PIX[0])
        s = R._setup(sx, sy, valid, f, 64, 64)
        cnt = (s["i1"] - s["i0"] + 1) * (s["j1"] - s["j0"] + 1)
        assert (cnt <= R.SMALL_MAX).sum() > 300 and (cnt > R.SMALL_MAX).sum() > 300


# ---- against the restatement and fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_equals_the_restatement_bit_for_bit(RD, name):
    (_, v, f, cams, H, W), ref = reference(name)
    g = gpu_render(RD, v, f, cams, H, W)
    assert (ref["mask"] != 0).sum() > 0.1 * ref["mask"].size
    for k in ("face", "mask", "dropped"):
        assert np.array_equal(g[k], ref[k]), k
    for k in FLOATS:
        diff = bits(g[k]) != bits(ref[k])
        print(f"{name} {k}: {int(diff.sum())} of {diff.size} values differ in bits")
        assert not diff.any(), k


@pytest.mark.parametrize("name", SCENES)
def test_depth_against_fp64(RD, name):
    (_, v, f, cams, H, W), ref = reference(name)
    g = gpu_render(RD, v, f, cams, H, W)
    tol = R.DEPTH_TOL_FACTOR * R.DEPTH_BASE_U * R.U
    for i, cam in enumerate(cams):
        chosen, best, _, _, zrange = R.depth_f64(v, f, cam, H, W, g["face"][i])
        m = g["mask"][i] != 0
        assert np.array_equal(m, np.isfinite(best)) and np.isfinite(chosen[m]).all()
        err = float(np.abs(g["depth"][i][m].astype(np.float64) - chosen[m]).max() / zrange)
        tie = float((chosen[m] - best[m]).max() / zrange)
        print(f"{name} view {i}: depth error {err / R.U:.3f} u, chosen - fp64 minimum {tie / R.U:.3f} u of the depth range (bound {tol / R.U:.1f} u)")
        assert err <= tol and tie <= tol


# ---- invariances ------------------------------------------------------------------------------------------------------------------
def test_batch_permutation_and_repetition(RD):
    v, f = R.wavy_sheet(2000, jitter=0.004, seed=5)
    H, W = 61, 97
    cams = RD.orbit_cameras(5, 30.0, 2.6, size=(H, W)).numpy()
    batch = gpu_render(RD, v, f, cams, H, W)
    again = gpu_render(RD, v, f, cams, H, W)
    assert_same(batch, again)
    alone = gpu_render(RD, v, f, cams[3:4], H, W)
    for k in BUFFERS + ("dropped",):
        assert np.array_equal(bits(alone[k][0]), bits(batch[k][3])), k
    assert all(R.depth_ties(v, f, c, H, W) == 0 for c in cams[:2])
    perm = np.random.default_rng(0).permutation(len(f))
    p = gpu_render(RD, v, f[perm], cams[:2], H, W)
    for k in ("depth", "mask", "normal", "shaded"):
        assert np.array_equal(bits(p[k]), bits(batch[k][:2])), k
    m = batch["mask"][:2] != 0
    assert np.array_equal(perm[p["face"][m]], batch["face"][:2][m]) and (p["face"][~m] == -1).all()


# ---- contours ---------------------------------------------------------------------------------------------------------------------
def _reachable_from_border(free):
    """pixels 4-connected to the image border through `free` pixels"""
    seen = np.zeros_like(free)
    seen[0, :], seen[-1, :], seen[:, 0], seen[:, -1] = free[0, :], free[-1, :], free[:, 0], free[:, -1]
    while True:
        grow = seen.copy()
        grow[1:, :] |= seen[:-1, :]; grow[:-1, :] |= seen[1:, :]; grow[:, 1:] |= seen[:, :-1]; grow[:, :-1] |= seen[:, 1:]
        grow &= free
        if np.array_equal(grow, seen):
            return seen
        seen = grow


def test_contours(RD):
    H = W = 48
    r = _renderers.setdefault((H, W), RD.Renderer((H, W), max_views=8))
    v, f = R.box()
    cams = RD.orbit_cameras(3, 25.0, 2.6, size=H)
    buf = r.render(torch.as_tensor(v).cuda(), torch.as_tensor(f).cuda(), cams)
    for jump, crease in ((0.05, 30.0), (1e9, 180.0)):
        ink = r.contours(buf, jump, crease).cpu().numpy()
        ref = R.contours_ref(buf["mask"].cpu().numpy(), buf["depth"].cpu().numpy(), buf["normal"].cpu().numpy(), jump, RD.cos_crease(crease))
        assert np.array_equal(ink, ref)
    mask = buf["mask"].cpu().numpy() != 0
    for i in range(3):                                            # silhouette only: a closed ring around the shape
        outside = _reachable_from_border(ink[i] == 0)
        assert mask[i].any() and not (outside & mask[i]).any() and (ink[i] != 0).sum() < 0.5 * mask[i].sum()
    # a sheet folded by 90 degrees, seen from the front: a line along the fold at 30 degrees, none at 170
    v, f = R.folded_sheet(90.0)
    cam = RD.orbit_cameras(1, 0.0, 2.6, mode="orthographic", size=H)
    buf = r.render(torch.as_tensor(v).cuda(), torch.as_tensor(f).cuda(), cam)
    m = buf["mask"][0].cpu().numpy() != 0
    inner = m.copy()
    inner[1:, :] &= m[:-1, :]; inner[:-1, :] &= m[1:, :]; inner[:, 1:] &= m[:, :-1]; inner[:, :-1] &= m[:, 1:]
    sharp = r.contours(buf, 1e9, 30.0)[0].cpu().numpy() != 0
    flat = r.contours(buf, 1e9, 170.0)[0].cpu().numpy() != 0
    rows = np.nonzero(inner.any(1))[0]
    assert len(rows) > 20 and (sharp & inner)[rows].any(1).all()          # the line crosses every interior row
    assert set(np.nonzero((sharp & inner).any(0))[0]) <= {W // 2 - 1, W // 2}
    assert not (flat & inner).any()
    for ink, crease in ((sharp, 30.0), (flat, 170.0)):
        ref = R.contours_ref(buf["mask"].cpu().numpy(), buf["depth"].cpu().numpy(), buf["normal"].cpu().numpy(), 1e9, RD.cos_crease(crease))
        assert np.array_equal(ink, ref[0] != 0)


# ---- surface ----------------------------------------------------------------------------------------------------------------------
def test_render_mesh_from_an_obj_file(RD, tmp_path):
    from surfd_amd import meshprep
    v, f = R.wavy_sheet(200)
    path = tmp_path / "sheet.obj"
    path.write_text("".join(f"v {x!r} {y!r} {z!r}\n" for x, y, z in v.astype(np.float64).tolist()) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f))
    vt, ft = meshprep.read_mesh(path)
    assert np.array_equal(vt.numpy(), v) and ft.dtype == torch.int64
    out = RD.render_mesh(vt.cuda(), ft.cuda(), n_views=3, size=(40, 56), contours=True)
    assert out["shaded"].shape == (3, 40, 56) and out["ink"].shape == (3, 40, 56) and out["cameras"].shape == (3, 18)
    ref = R.render_f32(v, f, out["cameras"].numpy(), 40, 56)
    assert_same({k: t.cpu().numpy() for k, t in out.items()}, ref)
    rgb, m = RD.condition_image(out, 1)
    assert rgb.shape == (40, 56, 3) and rgb.dtype == np.uint8 and m.sum() == int(out["mask"][1].sum()) and not rgb[m == 0].any()


def test_smooth_normals(RD):
    from surfd_amd.meshproc import vertex_normals_by_angle
    v, f = R.wavy_sheet(800)
    H, W = 48, 48
    cams = RD.orbit_cameras(2, 35.0, 2.6, size=H).numpy()
    g = gpu_render(RD, v, f, cams, H, W, smooth=True)
    flat = gpu_render(RD, v, f, cams, H, W)
    m = g["mask"] != 0
    ln = np.linalg.norm(g["normal"].astype(np.float64), axis=-1)
    assert np.abs(ln[m] - 1).max() < 4 * R.U * 2 and not g["normal"][~m].any()           # a correctly rounded x / |x|: within 2 u of unit length
    assert (g["normal"][..., 2] <= 0).all()
    assert np.array_equal(g["face"], flat["face"]) and np.array_equal(bits(g["depth"]), bits(flat["depth"]))
    assert not np.array_equal(bits(g["normal"]), bits(flat["normal"]))
    vn = vertex_normals_by_angle(v, f).astype(np.float32)
    assert_same(g, R.render_f32(v, f, cams, H, W, vertex_normals=vn))
    given = gpu_render(RD, v, f, cams, H, W, vertex_normals=torch.as_tensor(vn).cuda(), light=(1.0, -1.0, -1.0), ambient=0.1)
    l = np.array([1.0, -1.0, -1.0]) / np.sqrt(3.0)
    assert_same(given, R.render_f32(v, f, cams, H, W, vertex_normals=vn, light=l.astype(np.float32), ambient=0.1))
    # a face without area in space has the zero normal, never NaN
    z = gpu_render(RD, np.array([[0, 0, 0], [0, 0, 0.2], [0, 0, 0.4], [0.3, 0, 0]], np.float32), [[0, 1, 2], [0, 1, 3]], cams, H, W)
    assert np.isfinite(z["normal"]).all() and np.isfinite(z["shaded"]).all()


class _Spy:
    """the library with every access to a raster entry point recorded"""
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name.startswith("surfd_raster_re") or name.startswith("surfd_raster_co"):
            self.calls.append(name)
        return getattr(self._lib, name)


def test_argument_errors_launch_nothing(RD, monkeypatch):
    r = RD.Renderer(16, max_views=2)
    v, f = (torch.as_tensor(a).cuda() for a in R.box())
    cams = RD.orbit_cameras(2, 20.0, 2.6, size=16)
    before = {k: t.clone() for k, t in r.render(v, f, cams).items()}
    spy = _Spy(RD.N.lib())
    monkeypatch.setattr(RD.N, "lib", lambda: spy)              # from here on every library call of the module is seen
    with pytest.raises(ValueError, match="no CPU fallback"):
        r.render(v.cpu(), f.cpu(), cams)
    with pytest.raises(TypeError, match="float32"):
        r.render(v.double(), f, cams)
    with pytest.raises(TypeError, match="int32 or int64"):
        r.render(v, f.float(), cams)
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        r.render(v[:, :2], f, cams)
    with pytest.raises(ValueError, match="contiguous"):
        r.render(v, f.t().contiguous().t(), cams)
    with pytest.raises(ValueError, match="outside"):
        r.render(v, f + 1, cams)
    with pytest.raises(ValueError, match="outside"):
        r.render(v, f - 1, cams)
    with pytest.raises(ValueError, match="NaN"):
        r.render(v * float("nan"), f, cams)
    with pytest.raises(ValueError, match="views"):
        r.render(v, f, RD.orbit_cameras(3, 20.0, 2.6, size=16))
    with pytest.raises(ValueError, match=r"\[n_views, 18\]"):
        r.render(v, f, cams[:, :12])
    with pytest.raises(TypeError, match="tensor"):
        r.render(v, f, cams.numpy())
    bad = cams.clone(); bad[0, 17] = 0.0
    with pytest.raises(ValueError, match="near"):
        r.render(v, f, bad)
    with pytest.raises(ValueError, match="flags"):
        r.render(v, f, cams, flags=3)
    with pytest.raises(ValueError, match="ambient"):
        r.render(v, f, cams, ambient=1.5)
    with pytest.raises(ValueError, match="not both"):
        r.render(v, f, cams, vertex_normals=v, smooth=True)
    with pytest.raises(ValueError, match="size"):
        RD.Renderer(4096)
    with pytest.raises(ValueError, match="max_views"):
        RD.Renderer(16, max_views=65)
    assert spy.calls == []                                     # every refusal above came before the library
    buf = r.render(v, f, cams)
    assert spy.calls == ["surfd_raster_render"]
    assert all(torch.equal(buf[k], before[k]) for k in before)  # and left the handle as it was
    with pytest.raises(ValueError, match="render"):
        r.contours({k: buf[k][:, :8] for k in ("mask", "depth", "normal")})
    with pytest.raises(ValueError, match="crease_deg"):
        r.contours(buf, 0.1, 200.0)
    assert spy.calls == ["surfd_raster_render"]
    assert RD.Renderer(16, device="cuda").device == v.device and RD.Renderer(16, device="cuda").render(v, f, cams[:1])["mask"].any()


def test_renderer_reuse(RD):
    r = RD.Renderer((24, 32), max_views=4)
    for n_tri, n_views in ((200, 1), (2000, 4), (12, 2), (0, 3), (800, 4)):
        v, f = R.box() if n_tri == 12 else (R.wavy_sheet(n_tri) if n_tri else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))
        cams = RD.orbit_cameras(n_views, 20.0, 2.6, size=(24, 32))
        out = r.render(torch.as_tensor(v).cuda(), torch.as_tensor(f).cuda(), cams)
        assert_same({k: t.cpu().numpy() for k, t in out.items()}, R.render_f32(v, f, cams.numpy(), 24, 32))


def test_example_drivers_write_views(RD, tmp_path):
    """python -m examples.render on an OBJ, and examples/reconstruct.py --preview: PNG views that read back as images"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    v, f = R.wavy_sheet(400)
    obj = tmp_path / "sheet.obj"
    obj.write_text("".join(f"v {x!r} {y!r} {z!r}\n" for x, y, z in v.astype(np.float64).tolist()) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f))
    r = subprocess.run([sys.executable, "-m", "examples.render", str(obj), "--views", "2", "--size", "64", "--out", str(tmp_path / "views"),
                        "--contours", "--smooth", "--clip_text", "a dress"], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "CLIP similarity skipped" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    names = sorted(os.listdir(tmp_path / "views"))
    assert names == sorted(f"sheet_v{k}_{n}.png" for k in (0, 1) for n in ("shaded", "depth", "normal", "ink")), names
    shaded = RD.read_png(str(tmp_path / "views" / "sheet_v0_shaded.png"))
    assert shaded.shape == (64, 64) and (shaded < 255).sum() > 400 and (shaded == 255).any()
    assert RD.read_png(str(tmp_path / "views" / "sheet_v1_normal.png")).shape == (64, 64, 3)
    ink = RD.read_png(str(tmp_path / "views" / "sheet_v0_ink.png"))
    assert ink.shape == (64, 64, 3) and set(np.unique(ink)) == {0, 255}
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "reconstruct.py"), "--synthetic", "--resolution", "64", "--num_points_pcd", "4000",
                        "--output_dir", str(tmp_path / "recon"), "--preview", "2"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    pngs = [n for n in os.listdir(tmp_path / "recon") if n.endswith(".png")]
    objs = [n for n in os.listdir(tmp_path / "recon") if n.endswith(".obj")]
    assert objs and len(pngs) == 6 * len(objs), (objs, pngs)
    assert RD.read_png(str(tmp_path / "recon" / sorted(pngs)[0])).shape[:2] == (512, 512)
