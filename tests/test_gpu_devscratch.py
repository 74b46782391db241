"""The device scratch and hipcub scaffold of the mesh builds (csrc/devscratch.h, csrc/meshedit.h) on the GPU, on the paths the suites
of its five users do not reach: a create that is refused halfway, a workspace that serves sorts of several lengths in one build,
the handle's own scan workspace over every later call, weld around the block edge, weld and merge through the one representative
routine, the arena's users after refused calls, and a hierarchy built after refused calls.  Everything is compared bit for bit
with the sequential restatements (meshtopo_ref, meshsmooth_ref, bvh_ref, meshsimplify_ref) and with meshproc."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshsmooth_ref as R  # noqa: E402
import meshtopo_ref as mt  # noqa: E402
import raycast_ref as rr  # noqa: E402
import test_gpu_meshbvh as bvh_suite  # noqa: E402
from test_gpu_meshtopo import TET, assert_same, cu, topology  # noqa: E402

pytestmark = pytest.mark.gpu


def test_a_refused_create_leaves_nothing_behind():
    from surfd_amd.meshsmooth import MeshSmoother
    from surfd_amd.meshtopo import MeshTopology
    v, f = R.icosphere(2, 0.02, seed=4)
    assert len(f) == 320
    V, x, good = len(v), cu(v), cu(f)

    def state():
        topo, s = MeshTopology(good, V), MeshSmoother(good, V)
        out = dict(topo._read())
        out["counts"] = torch.tensor([topo.num_edges, topo.num_degenerate, topo.num_referenced_vertices, s.num_border_halfedges, s.num_border_vertices])
        out["laplacian"] = s.laplacian(x, steps=2)
        return out

    before = state()
    last_bad = f.copy()
    last_bad[-1, 2] = V
    for bad, bad_V in ((np.array([[0, 1, 2], [0, -1, 2]]), 4), (last_bad, V)):
        for handle in (MeshTopology, MeshSmoother):
            with pytest.raises(RuntimeError, match=rf"libsurfd_hip error -1: .*outside \[0, {bad_V}\)"):
                handle(cu(bad), bad_V)
    after = state()
    assert sorted(after) == sorted(before)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    assert np.array_equal(after["laplacian"].cpu().numpy(), R.laplacian(v, f, 2))
    assert_same({k: after[k].cpu().numpy() for k in ("edges", "valence", "face_neighbors")}, {k: mt.build(f, V)[k] for k in ("edges", "valence", "face_neighbors")})


@pytest.mark.parametrize("n", [3, 257, 70_000])
def test_one_workspace_serves_sorts_of_comparable_lengths(n):
    """an open strip: every face has a border edge, so the sort of the 2 B = 2 n + 4 border records follows that of the 3 n keys"""
    from surfd_amd.meshsmooth import MeshSmoother
    v, f = mt.strip(n)
    v = v.astype(np.float64) + 0.1 * np.random.default_rng(n).standard_normal(v.shape)
    s = MeshSmoother(cu(f), len(v))
    assert (s.num_border_halfedges, s.num_border_vertices) == R.counts(f) == (n + 2, n + 2)
    got = s.smooth_borders(cu(v), iterations=2).cpu().numpy()
    assert np.array_equal(got, R.smooth_borders(v, f, iterations=2))


@pytest.mark.parametrize("mesh", ["tetrahedron", "icosphere3"])
def test_the_handles_scan_workspace_serves_every_later_call(mesh):
    """closed meshes, E = 3 F / 2 > F: border_loops scans more items than components does, all in the workspace create sized"""
    f = TET if mesh == "tetrahedron" else rr.icosphere(3)[1]
    topo = topology(f)
    assert topo.num_edges > topo.num_faces
    t = mt.build(f)
    for c in ("vertex", "edge", "manifold"):
        labels, sizes = topo.components(c)
        want = mt.components(t, c)
        assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(sizes.cpu().numpy(), want[1]), c
    for got, want in zip(topo.border_loops(), mt.border_loops(t)):
        assert np.array_equal(got.cpu().numpy(), want)
    topo._components.pop("vertex")                           # the library is asked again, not the object's memory
    labels, sizes = topo.components("vertex")
    want = mt.components(t, "vertex")
    assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(sizes.cpu().numpy(), want[1])


def block_edge_points(rng, V):
    pts = rng.integers(-1, 2, (V, 3)).astype(np.float32) * np.float32(0.5)       # 27 classes
    pts[rng.random(pts.shape) < 0.3] *= np.float32(-1)                           # signed zeros among them
    pts[-1] = pts[0]                                                           # a duplicate across the whole range
    return pts


@pytest.mark.parametrize("V", [1, 255, 256, 257])
def test_weld_around_the_block_edge(V):
    from surfd_amd.meshtopo import weld_vertices
    rng = np.random.default_rng(V)
    pts = block_edge_points(rng, V)
    tri = rng.integers(0, V, (V, 3))
    wv, wf, vmap = [x.cpu().numpy() for x in weld_vertices(cu(pts), cu(tri))]
    rv, rf, rmap = mt.weld(pts, tri)
    assert len(rv) < V or V == 1
    assert np.array_equal(vmap, rmap) and np.array_equal(wf, rf) and np.array_equal(wv.view(np.uint32), rv.view(np.uint32))


@pytest.mark.parametrize("V", [1, 255, 256, 257])
def test_weld_and_merge_through_the_one_representative_routine(V):
    """exact fp32 equality (meshtopo's weld) and quantisation at 1e-8 (meshclean's cull) give the same classes on {-0.5, 0, 0.5}^3,
    every vertex takes part, and both reach their survivors through group_representatives: one result, three ways"""
    from surfd_amd import meshproc as mp
    from surfd_amd.meshclean import cull_and_merge
    from surfd_amd.meshtopo import weld_vertices
    pts = block_edge_points(np.random.default_rng(V), V)
    i = np.arange(V)
    tri = np.stack([i, (i + 1) % V, (i + 2) % V], 1)
    p64 = pts.astype(np.float64)                                                # exact
    rv, rf, _ = mt.weld(pts, tri)
    cv, cf = mp.cull_and_merge(p64, tri)
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.int64)         # noqa: E731
    assert np.array_equal(bits(rv), bits(cv)) and np.array_equal(rf, cf)        # the two references agree on these inputs
    assert len(rv) < V or V == 1
    wv, wf, _ = [x.cpu().numpy() for x in weld_vertices(cu(pts), cu(tri))]
    assert wv.dtype == np.float32 and np.array_equal(wv.view(np.uint32), rv.view(np.uint32)) and np.array_equal(wf, rf)
    gv, gf = [x.cpu().numpy() for x in cull_and_merge(cu(p64), cu(tri))]
    assert gv.dtype == np.float64 and np.array_equal(bits(gv), bits(cv)) and np.array_equal(gf, cf)
    assert len(wv) == len(gv) and np.array_equal(bits(wv), bits(gv)) and np.array_equal(wf, gf)


def test_a_refused_call_leaves_nothing_behind_in_the_arenas_users():
    """clean_until_stable (four arenas) and the quadric simplification (two stages of one) on the icosphere; then every entry point
    is refused for a face that names vertex V, and the simplification once more between its two stages; then the first calls again"""
    import meshsimplify_ref as sr
    from surfd_amd import meshclean as MC, meshproc as mp
    from surfd_amd.meshsimplify import simplify_vertex_clustering as simplify
    v, f = R.icosphere(2, 0.02, seed=4)
    assert len(f) == 320
    V, dv, df = len(v), cu(v), cu(f)

    def state():
        cv, cf, st = MC.clean_until_stable(dv, df, return_stats=True)
        sv, sf, sm, ss = simplify(dv, df, 0.3, representative="quadric", return_map=True, return_stats=True)
        return dict(cv=cv, cf=cf, sv=sv, sf=sf, sm=sm), (st, ss)

    before, stats = state()
    assert len(before["sv"]) > 1 and len(before["sf"]) > 0                       # more than one cluster: the records are sorted
    bad = f.copy()
    bad[-1, 2] = V
    for call in (MC.cull_and_merge, MC.drop_degenerate_faces, MC.fill_small_holes, MC.clean_until_stable,
                 lambda a, b: simplify(a, b, 0.3, representative="quadric"), lambda a, b: simplify(a, b, 0.3, representative="mean")):
        with pytest.raises(RuntimeError, match=rf"libsurfd_hip error -1:.*outside \[0, {V}\)"):
            call(dv, cu(bad))
    with pytest.raises(RuntimeError, match="libsurfd_hip error -1:.*negative"):
        MC.drop_duplicate_faces(cu(np.where(bad == V, -1, bad)))                # this pass has no V: a negative index is its refusal
    with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*2\^21"):     # after the first host read, before the second stage
        simplify(dv, df, 2.0 ** -21, representative="quadric")
    after, stats_after = state()
    assert stats_after == stats
    for k in before:
        assert after[k].dtype == before[k].dtype and torch.equal(after[k].view(torch.int64) if after[k].dtype == torch.float64 else after[k],
                                                                 before[k].view(torch.int64) if before[k].dtype == torch.float64 else before[k]), k
    hv, hf = mp.clean_until_stable(v, f)
    assert np.array_equal(after["cv"].cpu().numpy().view(np.int64), hv.view(np.int64)) and np.array_equal(after["cf"].cpu().numpy(), hf)
    wv, wf, wm, _ = sr.simplify(v, f, 0.3, representative="quadric")
    assert np.array_equal(after["sv"].cpu().numpy().view(np.int64), np.ascontiguousarray(wv).view(np.int64))
    assert np.array_equal(after["sf"].cpu().numpy(), wf) and np.array_equal(after["sm"].cpu().numpy(), wm)


def test_a_hierarchy_built_after_refused_calls():
    bvh_suite.test_hierarchy_flag_without_a_build_is_an_error()
    for F in (1, 257):
        bvh_suite.test_hierarchy_invariants_from_the_read_out(F)
