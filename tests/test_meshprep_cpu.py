"""CPU-side checks of mesh preprocessing (surfd_amd/meshprep.py, csrc/meshdist.hip): the C ABI is exported, bound and reports
bad arguments through return codes; the kernels are in the code object without spills or scratch; the module refuses what it
cannot run before any launch; read_mesh covers every face form; sample_points_around_pcd draws what the reference's function
draws (fixture g19); and the fp64 oracle of the GPU tests (tests/mesh_udf_ref.py) reproduces constructed answers."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from surfd_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_udf_ref as R  # noqa: E402

MESH_EXPORTS = ("surfd_mesh_create", "surfd_mesh_destroy", "surfd_mesh_num_triangles", "surfd_mesh_closest")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        from surfd_amd.build import build_library
        build_library()
    return N.lib()


def test_exports(lib):
    raw = C.CDLL(N.LIB_PATH)
    for sym in MESH_EXPORTS:
        assert hasattr(raw, sym), sym
        assert sym in N.EXPORTED_SYMBOLS, sym
        assert getattr(lib, sym).argtypes is not None
    assert lib.surfd_abi_version() == 1


def test_error_codes_without_a_device(lib):
    h = C.c_void_p()
    p = C.c_void_p(16)
    assert lib.surfd_mesh_create(None, 3, p, 1, None, C.byref(h)) == -1
    assert b"null vertices" in lib.surfd_last_error()
    assert lib.surfd_mesh_create(p, 3, None, 1, None, C.byref(h)) == -1
    assert lib.surfd_mesh_create(p, 3, p, 1, None, None) == -1
    assert lib.surfd_mesh_create(p, 3, p, 0, None, C.byref(h)) == -1                 # F = 0
    assert b"F = 0" in lib.surfd_last_error()
    assert lib.surfd_mesh_create(p, 0, p, 1, None, C.byref(h)) == -1
    assert not h.value
    assert lib.surfd_mesh_closest(None, p, 4, 0, None, None, None, None, None) == -1
    assert b"null handle" in lib.surfd_last_error()
    assert lib.surfd_mesh_closest(p, p, -1, 0, None, None, None, None, None) == -1      # negative Q: refused before the handle is read
    assert b"negative" in lib.surfd_last_error()
    assert lib.surfd_mesh_closest(p, p, 4, 2, None, None, None, None, None) == -1       # unknown flag bit
    assert b"flags" in lib.surfd_last_error()
    assert lib.surfd_mesh_num_triangles(None) == 0
    lib.surfd_mesh_destroy(None)


def test_kernels_do_not_spill():
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    meta = mod.kernel_metadata()
    names = [k for k in meta if "surfd::md_" in k]
    for base in ("md_prepare_kernel", "md_bounds_kernel", "md_closest_kernel<true>", "md_closest_kernel<false>", "md_finish_kernel"):
        assert any(f"surfd::{base}" in k for k in names), (base, names)
    assert len(names) == 5, names
    for k in names:
        v = meta[k]
        assert v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".private_segment_fixed_size"] == 0, (k, v)


def test_module_refuses_cpu_tensors_and_wrong_inputs():
    from surfd_amd import meshprep as M
    v = torch.zeros(4, 3)
    t = torch.tensor([[0, 1, 2]])
    q = torch.zeros(5, 3)
    for call in (lambda: M.closest_points(v, t, q), lambda: M.MeshDistance(v, t), lambda: M.compute_udf_and_gradients(v, t, q),
                 lambda: M.compute_udf_from_mesh(v, t), lambda: M.point_to_mesh_distance(q, v, t), lambda: M.mesh_distance(v, t, v, t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        M.closest_points(torch.zeros(4, 2), t, q)
    with pytest.raises(TypeError, match="float32"):
        M.closest_points(v.double(), t, q)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        M.closest_points(v, torch.zeros(0, 3, dtype=torch.long), q)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        M.closest_points(v, torch.zeros(2, 4, dtype=torch.long), q)
    with pytest.raises(TypeError, match="int32 or int64"):
        M.closest_points(v, t.float(), q)
    with pytest.raises(ValueError, match=r"queries must be \[N, 3\]"):
        M.closest_points(v, t, torch.zeros(5))
    with pytest.raises(TypeError, match="queries must be float32"):
        M.closest_points(v, t, q.double())


OBJ_TEXT = """# every face form
mtllib none.mtl
o thing
v 0 0 0
v 1 0 0
v 1 1 0 0.5 0.5 0.5
v 0 1 0
vt 0 0
vn 0 0 1
g faces
f 1 2 3
f 1/1 3/1 4/1
f 1/1/1 2/1/1 3/1/1
f 1//1 2//1 4//1
v 0.5 0.5 1
f -1 -5 -4
f 1 2 3 4
f 1//1 2//1 3//1 4//1 5//1
s off
usemtl x
l 1 2
"""


def test_read_mesh_face_forms(tmp_path):
    from surfd_amd.meshprep import read_mesh
    p = tmp_path / "forms.obj"
    p.write_text(OBJ_TEXT)
    v, t = read_mesh(p)
    assert v.dtype == torch.float32 and t.dtype == torch.int64
    assert v.shape == (5, 3) and torch.equal(v[2], torch.tensor([1.0, 1.0, 0.0])) and torch.equal(v[4], torch.tensor([0.5, 0.5, 1.0]))
    want = [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 1, 3], [4, 0, 1], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    assert t.tolist() == want
    with pytest.raises(ValueError, match="does not exists"):
        read_mesh(tmp_path / "missing.obj")
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nf 1 2 7\n")
    with pytest.raises(ValueError, match="does not exist"):
        read_mesh(bad)


def test_sample_points_around_pcd_matches_reference(golden):
    from surfd_amd.meshprep import sample_points_around_pcd
    z = golden("g19_meshprep")
    for tag in ("larger", "smaller", "exact"):
        pcd = torch.from_numpy(z[f"{tag}__pcd"])
        counts = [int(c) for c in z[f"{tag}__counts"]]
        torch.manual_seed(19)
        got = sample_points_around_pcd(pcd, [0.003, 0.01, 0.1], counts, (-1.0, 1.0), "cpu")
        assert got.dtype == torch.float32 and got.shape == (sum(counts), 3)
        assert np.array_equal(got.numpy(), z[f"{tag}__coords"]), tag
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g19_meshprep.npz")) < 1 << 20


def test_sample_points_uniformly_on_the_cpu_is_seeded_and_on_the_mesh():
    from surfd_amd.meshprep import sample_points_uniformly
    v, t = R.wavy_sheet(12)
    vt, tt = torch.from_numpy(v), torch.from_numpy(t)
    a = sample_points_uniformly(vt, tt, 2000, generator=torch.Generator().manual_seed(4))
    b = sample_points_uniformly(vt, tt, 2000, generator=torch.Generator().manual_seed(4))
    assert a.dtype == torch.float32 and a.shape == (2000, 3) and torch.equal(a, b)
    assert R.closest_fp64(v, t, a.numpy())[0].max() < 1e-6


def test_oracle_reproduces_constructed_answers():
    """tests/mesh_udf_ref.py against itself: on the convex polyhedron a query c + s n over a point c strictly inside a face has
    distance s, closest point c and a triangle of that face; a query on a vertex has distance 0."""
    v, t, face = R.convex_polyhedron(levels=2)
    v64 = v.astype(np.float64)
    g = np.random.default_rng(0)
    pick = g.integers(0, len(t), 300)
    w = g.dirichlet([2.0, 2.0, 2.0], 300)
    a, b, c = v64[t[pick, 0]], v64[t[pick, 1]], v64[t[pick, 2]]
    cpt = w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert ((cpt * n).sum(1) > 0).all()                                   # outward orientation (the origin is inside)
    s = 10.0 ** g.uniform(-4, np.log10(0.5), 300)
    d, x, j = R.closest_fp64(v, t, cpt + s[:, None] * n)
    assert np.abs(d - s).max() < 1e-12
    assert np.abs(x - cpt).max() < 1e-12
    assert (face[j] == face[pick]).all()
    d, x, _ = R.closest_fp64(v, t, v64[:50])
    assert d.max() == 0.0 and np.array_equal(x, v64[:50])
    # degenerate triangles are the union of their edges
    zv, zt = R.zero_area_mesh(count=8)
    d, _, _ = R.closest_fp64(zv, zt, zv.astype(np.float64))
    assert d.max() == 0.0
    # the fp32 restatement of the kernel's formulas agrees with the oracle on a small case, degenerate triangles included
    sv, st = R.spliced_sheet(8)
    q = g.uniform(-1, 1, (400, 3)).astype(np.float32)
    d32 = R.kernel_formulas_fp32(sv, st, q)[0]
    assert np.abs(d32 - R.closest_fp64(sv, st, q)[0]).max() < 1e-5
    assert np.isfinite(d32).all()
