"""The device scratch and hipcub scaffold of the mesh builds (csrc/devscratch.h) on the GPU, on the paths the suites of its three
users do not reach: a create that is refused halfway, a workspace that serves sorts of several lengths in one build, the
handle's own scan workspace over every later call, weld around the block edge, and a hierarchy built after refused calls.
Everything is compared bit for bit with the sequential restatements (meshtopo_ref, meshsmooth_ref, bvh_ref)."""
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


@pytest.mark.parametrize("V", [1, 255, 256, 257])
def test_weld_around_the_block_edge(V):
    from surfd_amd.meshtopo import weld_vertices
    rng = np.random.default_rng(V)
    pts = rng.integers(-1, 2, (V, 3)).astype(np.float32) * np.float32(0.5)       # 27 classes
    pts[rng.random(pts.shape) < 0.3] *= np.float32(-1)                           # signed zeros among them
    pts[-1] = pts[0]                                                           # a duplicate across the whole range
    tri = rng.integers(0, V, (V, 3))
    wv, wf, vmap = [x.cpu().numpy() for x in weld_vertices(cu(pts), cu(tri))]
    rv, rf, rmap = mt.weld(pts, tri)
    assert len(rv) < V or V == 1
    assert np.array_equal(vmap, rmap) and np.array_equal(wf, rf) and np.array_equal(wv.view(np.uint32), rv.view(np.uint32))


def test_a_hierarchy_built_after_refused_calls():
    bvh_suite.test_hierarchy_flag_without_a_build_is_an_error()
    for F in (1, 257):
        bvh_suite.test_hierarchy_invariants_from_the_read_out(F)
