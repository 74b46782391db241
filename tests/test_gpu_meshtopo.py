"""csrc/meshtopo.hip on the GPU against the sequential restatement tests/meshtopo_ref.py.  Everything is
an integer or a bool, so every comparison is exact; the one tolerance is the winding numbers' own (winding_ref.tolerance).
Smallest shapes that can go wrong, then many workgroups and long chains (a strip of diameter 100 000), invariance under face
permutation and corner rotation, the orientation property checked on the returned mesh itself, the marching-cubes fixtures,
weld, outward, the winding numbers the feature exists for, and keep_components_with_at_least against meshproc's."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshtopo_ref as mt  # noqa: E402
import raycast_ref as rr  # noqa: E402
import winding_ref as wr  # noqa: E402
from test_meshtopo_cpu import FIXTURE_TABLE, fixture_mesh  # noqa: E402

pytestmark = pytest.mark.gpu

TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int64)


def cu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def topology(f, V=None):
    from surfd_amd.meshtopo import MeshTopology
    return MeshTopology(cu(np.asarray(f, dtype=np.int64).reshape(-1, 3)), V)


def arrays(topo, vertices=None):
    """every array of a MeshTopology as numpy"""
    out = {k: getattr(topo, k).cpu().numpy() for k in ("edges", "valence", "edge_offsets", "edge_halfedges", "face_edges", "face_neighbors", "degenerate")}
    for c in ("vertex", "edge", "manifold"):
        labels, sizes = topo.components(c)
        out["labels_" + c], out["sizes_" + c] = labels.cpu().numpy(), sizes.cpu().numpy()
    for k, a in zip(("loop_labels", "loop_sizes", "loop_simple"), topo.border_loops()):
        out[k] = a.cpu().numpy()
    flip, po = topo.orientation(None if vertices is None else cu(vertices))
    out["flip"], out["patch_orientable"] = flip.cpu().numpy(), po.cpu().numpy()
    return out


def ref_arrays(f, V=None, vertices=None):
    t = mt.build(f, V)
    out = {k: t[k] for k in ("edges", "valence", "edge_offsets", "edge_halfedges", "face_edges", "face_neighbors", "degenerate")}
    for c in ("vertex", "edge", "manifold"):
        out["labels_" + c], out["sizes_" + c] = mt.components(t, c)
    out["loop_labels"], out["loop_sizes"], out["loop_simple"] = mt.border_loops(t)
    out["flip"], out["patch_orientable"] = mt.orientation(t, vertices)
    return out


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(g, w), (k, np.nonzero(g.reshape(-1) != w.reshape(-1))[0][:8])


def check(f, V=None, vertices=None, summary=True):
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    topo = topology(f, V)
    got = arrays(topo, vertices)
    assert_same(got, ref_arrays(f, V, vertices))
    if summary:
        assert topo.summary() == mt.summary(mt.build(f, V))
    return topo, got


# ---- smallest shapes that can go wrong ----------------------------------------------------------------------------------------
def small_cases():
    bv, bf = mt.band(16, twist=True)
    av, af = mt.band(16, twist=False)
    return {
        "empty": (np.zeros((0, 3), dtype=np.int64), 0),
        "empty_with_vertices": (np.zeros((0, 3), dtype=np.int64), 5),
        "one_triangle": ([[0, 1, 2]], None),
        "one_triangle_spare_vertices": ([[4, 1, 2]], 9),
        "tetrahedron": (TET, None),
        "cube": (rr.cube()[1], None),
        "cube_flipped": (rr.cube_flipped()[1], None),
        "two_cubes_edge": (mt.two_cubes("edge")[1], None),
        "two_cubes_vertex": (mt.two_cubes("vertex")[1], None),
        "duplicated_face": ([[0, 1, 2], [0, 1, 2]], None),
        "duplicated_face_on_cube": (np.concatenate([rr.cube()[1], rr.cube()[1][3:4]]), None),
        "repeated_index": ([[0, 1, 2], [2, 2, 3], [2, 1, 3]], 4),
        "all_degenerate": ([[0, 0, 1], [2, 2, 2]], 3),
        "bow_tie": ([[0, 1, 2], [0, 3, 4]], None),
        "moebius": (bf, None),
        "annulus": (af, None),
        "torus": (rr.torus()[1], None),
        "octahedron": (rr.octahedron()[1], None),
    }


@pytest.mark.parametrize("name", sorted(small_cases()))
def test_small_shapes(name):
    f, V = small_cases()[name]
    check(f, V)


def test_small_shapes_by_hand():
    """the numbers the issue names, asserted on the device's own output"""
    s = topology(rr.torus()[1]).summary()
    assert s["closed"] and s["patches"][0]["genus"] == 1
    s = topology(mt.band(16, twist=True)[1]).summary()
    assert not s["orientable"] and s["border_loops"] == 1 and s["largest_border_loop"] == 32
    topo = topology(mt.band(16, twist=True)[1])
    assert not bool(topo.orientation()[0].any())
    assert topology(mt.band(16)[1]).border_loops()[1].tolist() == [16, 16]
    s = topology(mt.two_cubes("edge")[1]).summary()
    assert (s["components_edge"], s["components_manifold"], s["non_manifold_edges"]) == (1, 2, 1)
    assert int(topology(mt.two_cubes("edge")[1]).valence.max()) == 4
    s = topology(mt.two_cubes("vertex")[1]).summary()
    assert (s["components_vertex"], s["components_edge"]) == (1, 2)
    flip = topology(rr.cube_flipped()[1]).orientation()[0].cpu().numpy()
    turned = np.arange(12) % 2 == 0
    assert np.array_equal(flip, turned ^ turned[0])
    s = topology(np.zeros((0, 3), dtype=np.int64), 0).summary()
    assert s["faces"] == 0 and s["edges"] == 0 and s["patches"] == []


def test_refusals():
    from surfd_amd.meshtopo import MeshTopology
    with pytest.raises(RuntimeError, match="outside"):
        MeshTopology(cu(np.array([[0, 1, 5]])), 5)
    with pytest.raises(RuntimeError, match="face 1"):
        MeshTopology(cu(np.array([[0, 1, 2], [0, -1, 2]])), 3)
    with pytest.raises(ValueError):
        topology(TET).components("face")


# ---- many workgroups and long chains ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_case(name):
    if name == "strip":
        v, f = mt.strip(100_000)
        f, perm, turned = mt.turned_and_shuffled(f, 0.4, seed=11)
    elif name == "icosphere6":
        v, f = rr.icosphere(6)
        f, perm, turned = mt.turned_and_shuffled(f, 0.4, seed=12)
    else:
        v, f = mt.interleaved_copies(*rr.icosphere(2), copies=64)
        turned = np.zeros(len(f), dtype=bool)
    return v, f, turned, ref_arrays(f, len(v))


@pytest.mark.parametrize("name", ["strip", "icosphere6", "copies"])
def test_many_workgroups_and_long_chains(name):
    v, f, turned, want = big_case(name)
    got = arrays(topology(f, len(v)))
    assert_same(got, want)
    labels = got["labels_manifold"]
    first = np.full(labels.max() + 1, len(f))
    np.minimum.at(first, labels, np.arange(len(f)))
    assert np.array_equal(got["flip"], turned ^ turned[first[labels]])       # exactly the turned set relative to each patch's lowest face
    assert mt.same_direction_manifold_edges(mt.oriented(f, got["flip"])) == 0
    if name == "strip":
        assert got["sizes_manifold"].tolist() == [100_000] and got["loop_sizes"].tolist() == [100_002]
    if name == "icosphere6":
        assert len(f) == 81_920 and got["sizes_vertex"].tolist() == [81_920] and len(got["loop_sizes"]) == 0
    if name == "copies":
        assert np.array_equal(got["labels_vertex"], np.arange(len(f)) % 64)  # canonical: copy c's lowest face is face c
        assert got["sizes_edge"].tolist() == [320] * 64


# ---- invariance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["noisy_blob_48", "two_cubes_edge", "moebius"])
def test_face_permutation_and_corner_rotation(mesh):
    f = {"noisy_blob_48": lambda: fixture_mesh("noisy_blob_48")[1], "two_cubes_edge": lambda: mt.two_cubes("edge")[1],
         "moebius": lambda: mt.band(16, twist=True)[1]}[mesh]()
    rng = np.random.default_rng(5)
    f = mt.turned_and_shuffled(f, 0.3, seed=6)[0]
    base = arrays(topology(f))
    # a cyclic rotation of a face's indices changes nothing but the columns of that face's rows
    shift = rng.integers(0, 3, len(f))
    rot = np.stack([f[np.arange(len(f)), (c + shift) % 3] for c in range(3)], 1)
    got = arrays(topology(rot))
    for k in base:
        if k in ("face_edges", "face_neighbors"):
            assert np.array_equal(np.stack([got[k][np.arange(len(f)), (c - shift) % 3] for c in range(3)], 1), base[k]), k
        elif k == "edge_halfedges":
            h = got[k]
            back = 3 * (h // 3) + (h % 3 + shift[h // 3]) % 3                 # the same half-edges, renamed; sorted per edge they agree
            off = base["edge_offsets"]
            assert all(sorted(back[off[e]:off[e + 1]]) == list(base[k][off[e]:off[e + 1]]) for e in range(len(off) - 1))
        else:
            assert np.array_equal(got[k], base[k]), k
    # a permutation of the faces: the same partitions, classes and counts, and the same oriented mesh up to whole-patch flips
    perm = rng.permutation(len(f))
    got = arrays(topology(f[perm]))
    for k in ("edges", "valence", "edge_offsets", "degenerate"):
        assert np.array_equal(got[k] if k != "degenerate" else np.sort(got[k]), base[k] if k != "degenerate" else np.sort(base[k])), k
    for c in ("vertex", "edge", "manifold"):
        a, b = got["labels_" + c], base["labels_" + c][perm]
        assert len(np.unique(np.stack([a, b], 1), axis=0)) == len(base["sizes_" + c]) == len(got["sizes_" + c])
        assert sorted(got["sizes_" + c].tolist()) == sorted(base["sizes_" + c].tolist())
    assert sorted(got["loop_sizes"].tolist()) == sorted(base["loop_sizes"].tolist())
    assert sorted(got["patch_orientable"].tolist()) == sorted(base["patch_orientable"].tolist())
    differs = got["flip"] ^ base["flip"][perm]
    lab = got["labels_manifold"]
    for p in range(len(got["sizes_manifold"])):
        assert differs[lab == p].all() or not differs[lab == p].any()


def test_a_second_topology_of_the_same_input_gives_equal_arrays():
    v, f, _, want = big_case("strip")
    a = arrays(topology(f, len(v)))
    other = arrays(topology(fixture_mesh("noisy_blob_48")[1]))              # another mesh of the process in between
    b = arrays(topology(f, len(v)))
    assert_same(a, b)
    assert len(other["sizes_vertex"]) == 19


# ---- the property itself, on the returned mesh ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["cube_flipped", "torus", "noisy_blob_48", "two_cubes_edge"])
def test_oriented_triangles_have_no_same_direction_manifold_edge(mesh):
    f = {"cube_flipped": lambda: rr.cube_flipped()[1], "torus": lambda: rr.torus()[1], "noisy_blob_48": lambda: fixture_mesh("noisy_blob_48")[1],
         "two_cubes_edge": lambda: mt.two_cubes("edge")[1]}[mesh]()
    f = mt.turned_and_shuffled(f, 0.4, seed=21)[0]
    assert mt.same_direction_manifold_edges(f) > 0
    topo = topology(f)
    out = topo.oriented_triangles().cpu().numpy()
    assert mt.same_direction_manifold_edges(out) == 0
    assert np.array_equal(np.sort(out, 1), np.sort(f, 1))
    labels = topo.components("manifold")[0].cpu().numpy()
    for p in range(labels.max() + 1):
        lowest = np.nonzero(labels == p)[0][0]
        assert np.array_equal(out[lowest], f[lowest])                        # every patch's lowest face is untouched


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURE_TABLE))
def test_fixtures_reproduce_the_table(name):
    F, V, E, chi, border, nonmanifold, comps, loops, same_dir = FIXTURE_TABLE[name]
    v, f = fixture_mesh(name)
    topo, got = check(f, len(v))
    s = topo.summary()
    assert (s["faces"], s["referenced_vertices"], s["edges"], s["euler_characteristic"]) == (F, V, E, chi)
    assert (s["border_edges"], s["non_manifold_edges"]) == (border, nonmanifold)
    assert (s["components_vertex"], s["components_edge"], s["components_manifold"]) == comps
    assert s["border_loops"] == loops
    assert int(got["flip"].sum()) == 0 and s["consistently_oriented"]
    from surfd_amd.meshtopo import is_closed
    assert is_closed(cu(f)) == (border == 0)


# ---- weld ---------------------------------------------------------------------------------------------------------------------
def test_weld_exploded_icosphere():
    from surfd_amd.meshtopo import weld_vertices
    v, f = rr.icosphere(3)
    ev, ef = mt.exploded(v, f)
    wv, wf, vmap = [x.cpu().numpy() for x in weld_vertices(cu(ev), cu(ef))]
    rv, rf, rmap = mt.weld(ev, ef)
    assert np.array_equal(wv, rv) and np.array_equal(wf, rf) and np.array_equal(vmap, rmap)
    assert len(wv) == len(v) and np.array_equal(wv[wf], v[f])
    assert topology(wf, len(wv)).summary() == topology(f, len(v)).summary()
    keys = ("sizes_vertex", "sizes_edge", "sizes_manifold", "loop_sizes", "flip", "face_neighbors")      # what does not name a vertex
    assert_same({k: a for k, a in arrays(topology(wf, len(wv))).items() if k in keys}, {k: a for k, a in arrays(topology(f, len(v))).items() if k in keys})


def test_weld_signed_zero_and_nan():
    from surfd_amd.meshtopo import weld_vertices
    pts = np.array([[0.0, 1, 2], [-0.0, 1, 2], [np.nan, 0, 0], [np.nan, 0, 0], [5, 5, 5], [0, 1, 2], [5, 5, -0.0], [5, 5, 0.0], [1, np.nan, 2]], dtype=np.float32)
    tri = np.array([[0, 1, 4], [2, 3, 5], [6, 7, 8]])
    wv, wf, vmap = [x.cpu().numpy() for x in weld_vertices(cu(pts), cu(tri))]
    rv, rf, rmap = mt.weld(pts, tri)
    assert vmap.tolist() == rmap.tolist() == [0, 0, 1, 2, 3, 0, 4, 4, 5]
    assert np.array_equal(wf, rf) and np.array_equal(wv.view(np.uint32), rv.view(np.uint32))
    rng = np.random.default_rng(8)
    many = rng.integers(-2, 3, (5000, 3)).astype(np.float32) * np.float32(0.5)       # 125 classes, several workgroups, signed zeros
    many[rng.random(5000) < 0.02, 1] = np.nan
    wv, wf, vmap = [x.cpu().numpy() for x in weld_vertices(cu(many), cu(np.zeros((0, 3), dtype=np.int64)))]
    rv, rf, rmap = mt.weld(many, np.zeros((0, 3), dtype=np.int64))
    assert np.array_equal(vmap, rmap) and np.array_equal(wv.view(np.uint32), rv.view(np.uint32)) and wf.shape == (0, 3)


# ---- outward ------------------------------------------------------------------------------------------------------------------
def test_outward():
    from surfd_amd.meshtopo import orient_faces
    v, f = rr.icosphere(3)
    inverted = f[:, [0, 2, 1]]
    out, info = orient_faces(cu(v), cu(inverted), outward=True)
    assert np.array_equal(out.cpu().numpy(), f) and info["flipped"] == len(f)
    assert sum(mt.signed_volume_terms(v, out.cpu().numpy())) > 0
    out, info = orient_faces(cu(v), cu(inverted))                             # without outward the lowest face keeps its winding
    assert info["flipped"] == 0
    mixed = mt.turned_and_shuffled(f, 0.4, seed=4)[0]
    check(mixed, len(v), vertices=v, summary=False)
    out, info = orient_faces(cu(v), cu(mixed), outward=True)
    assert sum(mt.signed_volume_terms(v, out.cpu().numpy())) > 0 and mt.same_direction_manifold_edges(out.cpu().numpy()) == 0
    sv, sf = fixture_mesh("open_sheet_48")
    turned = sf[:, [0, 2, 1]]
    out, info = orient_faces(cu(sv), cu(turned), outward=True)                # an open sheet is left alone
    assert info["flipped"] == 0 and np.array_equal(out.cpu().numpy(), turned)
    # two shells, the inner one a cavity: patch by patch, both end up outward
    v2, f2 = np.concatenate([v, v * np.float32(0.5)]), np.concatenate([f, inverted + len(v)])
    check(f2, len(v2), vertices=v2, summary=False)
    out, info = orient_faces(cu(v2), cu(f2), outward=True)
    assert np.array_equal(out.cpu().numpy(), np.concatenate([f, f + len(v)]))
    # a soup: only the welded topology can orient it
    ev, ef = mt.exploded(v, mixed)
    out, info = orient_faces(cu(ev), cu(ef), outward=True, weld=True)
    assert np.array_equal(ev[out.cpu().numpy()], v[mt.oriented(mixed, mt.orientation(mt.build(mixed), v)[0])])


# ---- winding numbers: the reason for the feature --------------------------------------------------------------------------------
def test_winding_numbers_of_a_mesh_with_turned_faces():
    from surfd_amd.winding import WindingScene, winding_number
    v, f = rr.icosphere(3)
    mixed = f.copy()
    turned = np.random.default_rng(30).random(len(f)) < 0.3
    mixed[turned] = mixed[turned][:, [0, 2, 1]]
    q, kept, inside = wr.holed_sphere_queries([], n=2000)
    q = q[kept]
    good = winding_number(cu(v), cu(f), cu(q)).cpu().numpy()
    assert np.abs(good - inside[kept]).max() < 1e-6
    for orient in (True, "outward"):
        w = winding_number(cu(v), cu(mixed), cu(q), orient=orient).cpu().numpy()
        sign = 1.0 if orient == "outward" or not turned[0] else -1.0             # True keeps face 0 as it came
        err = np.abs(sign * w - good).max()
        print(f"orient={orient}: max |w - w_untouched| = {err:.3e} (bound {wr.tolerance(len(f)):.3e})")
        assert err <= wr.tolerance(len(f))
    assert np.array_equal(WindingScene(cu(v), cu(mixed), orient="outward").triangles.cpu().numpy(), f)
    bad = winding_number(cu(v), cu(mixed), cu(q)).cpu().numpy()               # without orient the same call is wrong
    assert min(np.abs(bad - good).max(), np.abs(-bad - good).max()) > 0.1
    bv, bf = mt.band(16, twist=True)
    with pytest.raises(ValueError, match="face 0"):
        WindingScene(cu(bv), cu(bf), orient=True)


# ---- the drivers --------------------------------------------------------------------------------------------------------------
def test_evaluate_and_reconstruct_topology_add_their_key(tmp_path):
    """in process (the byte-for-byte default of evaluate.py is pinned by the older driver tests): --topology only adds keys"""
    import json
    import mesh_udf_ref
    from examples import evaluate
    from examples.reconstruct import item_metrics
    from test_gpu_cloudsample import EVAL_ARGS, GOLDEN, make_eval_inputs     # the inputs and the command the golden JSON was written with
    gen_dir, ref_dir = make_eval_inputs(str(tmp_path))
    base = ["--generated", gen_dir, "--reference", ref_dir] + EVAL_ARGS
    plain = evaluate.run(evaluate.parse(base + ["--output", str(tmp_path / "plain.json")]))
    assert json.load(open(tmp_path / "plain.json")) == json.load(open(GOLDEN))
    more = evaluate.run(evaluate.parse(base + ["--topology", "--output", str(tmp_path / "more.json")]))
    assert more["options"].pop("topology") is True and more["options"] == plain["options"]
    assert more["skipped"] == ["item2"] and "topology" not in more["items"]["item2"]      # the .npz item carries no mesh
    for name in ("item0", "item1"):                                          # boxes: closed, one piece, genus 0 says chi = 2
        t = more["items"][name].pop("topology")
        assert t["closed"] and t["edge_manifold"] and t["consistently_oriented"] and "patches" not in t
        assert (t["components_vertex"], t["border_loops"], t["euler_characteristic"]) == (1, 0, 2)
        assert more["items"][name] == plain["items"][name]
    assert more["mean"].pop("topology_closed") == 1.0 and more["mean"].pop("topology_components_vertex") == 1.0
    assert more["mean"].pop("topology_border_loops") == 0.0 and more["mean"].pop("topology_non_manifold_edges") == 0.0
    assert more["mean"] == plain["mean"]
    with pytest.raises(SystemExit, match="--paired"):
        evaluate.run(evaluate.parse(["--generated", gen_dir, "--reference", ref_dir, "--topology"]))
    v, f = fixture_mesh("noisy_blob_48")
    path = str(tmp_path / "item.npz")
    np.savez(path, vertices=v, triangles=f)
    a = item_metrics(path, v, f, None, 0)
    b = item_metrics(path, v, f, None, 0, topology=True)
    t = b.pop("topology")
    assert b == a and (t["components_vertex"], t["border_loops"], t["border_edges"], t["closed"]) == (19, 15, 967, False)


def test_preprocess_orient_and_weld(tmp_path):
    """a soup of mixed orientation: --signed --sign winding --orient --weld writes the labels of the clean mesh"""
    import mesh_udf_ref
    from examples import preprocess_udfs
    v, f = rr.icosphere(2)
    mixed = mt.turned_and_shuffled(f, 0.4, seed=2)[0]
    ev, ef = mt.exploded(v, mixed)
    os.makedirs(tmp_path / "in")
    mesh_udf_ref.write_obj(tmp_path / "in" / "clean.obj", v * np.float32(0.9), f)
    os.makedirs(tmp_path / "in2")
    mesh_udf_ref.write_obj(tmp_path / "in2" / "soup.obj", ev * np.float32(0.9), ef)
    small = ["--num_surface_points", "2000", "--num_queries_per_std", "500", "500", "200", "200", "--num_queries_on_surface", "100",
             "--signed", "--sign", "winding"]
    preprocess_udfs.run(preprocess_udfs.parse([str(tmp_path / "in"), "--output_dir", str(tmp_path / "a")] + small))
    preprocess_udfs.run(preprocess_udfs.parse([str(tmp_path / "in2"), "--output_dir", str(tmp_path / "b"), "--orient", "--weld"] + small))
    preprocess_udfs.run(preprocess_udfs.parse([str(tmp_path / "in2"), "--output_dir", str(tmp_path / "c")] + small))
    files = {k: [os.path.join(r, x) for r, _, xs in os.walk(tmp_path / k) for x in xs if x.endswith(".npz")][0] for k in "abc"}
    clean, fixed, broken = [np.load(files[k]) for k in "abc"]
    inside = lambda z: z["labels"][100:] < 0                                  # noqa: E731
    # the soup has the same triangles in another order, so the random draws differ: compare each item with the analytic sphere,
    # away from the faceted surface (the sagitta of icosphere(2) is about 0.012)
    for z in (clean, fixed):
        r = np.linalg.norm(z["coords"][100:], axis=1)
        away = np.abs(r - 0.9 * 0.75) > 0.03
        assert away.sum() > 200 and np.array_equal(inside(z)[away], (r < 0.9 * 0.75)[away])
    r = np.linalg.norm(broken["coords"][100:], axis=1)
    away = np.abs(r - 0.9 * 0.75) > 0.03
    assert not np.array_equal(inside(broken)[away], (r < 0.9 * 0.75)[away])             # without --orient: 0.6 - 0.4 = 0.2 inside
    with pytest.raises(SystemExit, match="--sign winding"):
        preprocess_udfs.run(preprocess_udfs.parse([str(tmp_path / "in"), "--orient", "--signed"]))


# ---- components ---------------------------------------------------------------------------------------------------------------
def test_keep_components_matches_meshproc():
    from surfd_amd import meshproc
    from surfd_amd.meshtopo import face_components, keep_components_with_at_least
    v, f = fixture_mesh("noisy_blob_48")
    labels = face_components(cu(f), len(v)).cpu().numpy()
    sizes = np.bincount(labels)
    assert len(sizes) == 19
    min_faces = int(np.sort(sizes)[len(sizes) // 2])
    assert 0 < (sizes < min_faces).sum() < 19                                # some go
    kv, kf = keep_components_with_at_least(cu(v), cu(f), min_faces)
    pv, pf = meshproc.keep_components_with_at_least(v, f, min_faces)
    assert np.array_equal(kf.cpu().numpy(), pf) and np.array_equal(kv.cpu().numpy().astype(np.float64), pv)
    assert len(np.unique(np.stack([labels, meshproc.face_components(f, len(v))], 1), axis=0)) == 19
