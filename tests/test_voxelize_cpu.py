"""CPU-side checks of the voxeliser (surfd_amd/voxelize.py, csrc/voxel.hip): the numpy restatement (tests/voxel_ref.py) against
its Python-integer second form on triangles at the +-2^19 limit of the snap (the check that the int64 bounds of DESIGN.md
section 8.5 hold) and on the hand-made rule cases, the rule cases on the restatement itself, the counters including out-of-range
indices, the exports and their table, the argument checks of the library (before any HIP call), the module's refusal of CPU
tensors, and the kernels' code-object metadata (no spills, no scratch).  Every test of sections 1, 4 and 5 fails on a tree
without surfd_amd/voxelize.py or without the surfd_voxel_* symbols; all fail without tests/voxel_ref.py."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from surfd_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_ref as X  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOXEL_EXPORTS = ("surfd_voxel_workspace_bytes", "surfd_voxel_surface", "surfd_voxel_solid", "surfd_voxel_points", "surfd_voxel_iou")
SURFD_ERR_ARG = -1                                             # include/surfd_hip.h


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        from surfd_amd.build import build_library
        build_library()
    return N.lib()


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _snapped(tris):
    tri = np.asarray(tris, np.int64).reshape(-1, 3, 3)
    return tri, np.ones(len(tri), bool)


# ---- 1. library -------------------------------------------------------------------------------------------------------------------
def test_exports_bindings_and_table(lib):
    raw = C.CDLL(N.LIB_PATH)
    for sym in VOXEL_EXPORTS:
        assert hasattr(raw, sym), sym
        assert sym in N.EXPORTED_SYMBOLS, sym
    assert lib.surfd_abi_version() == 1
    assert "voxel.hip" in __import__("surfd_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "voxel.hip" not in __import__("surfd_amd.build", fromlist=["FILE_FLAGS"]).FILE_FLAGS            # no per-file flag
    rows = {r.split("|")[1].strip(" `"): r for r in _tool("abi_table").table().splitlines()[2:]}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for sym in VOXEL_EXPORTS:
        assert "no reference counterpart (" in rows[sym] and "`surfd_amd/voxelize.py`" in rows[sym], rows[sym]
        assert f"| `{sym}` |" in doc, sym
    hdr = open(os.path.join(ROOT, "include", "surfd_hip.h")).read()
    assert f"SURFD_ERR_ARG = {SURFD_ERR_ARG}," in hdr


def test_workspace_size(lib):
    assert lib.surfd_voxel_workspace_bytes(0, 1) == 4 * (16 + 0 + 1 + 1)
    assert lib.surfd_voxel_workspace_bytes(2000, 40) == 4 * (16 + 2000 + 40 * 40 * 2 + 40 * 40)
    assert lib.surfd_voxel_workspace_bytes(700_000_000, 512) == 4 * (16 + 700_000_000 + 512 * 512 * 16 + 512 * 512)
    assert lib.surfd_voxel_workspace_bytes(5, 0) == 0 and lib.surfd_voxel_workspace_bytes(5, 513) == 0 and lib.surfd_voxel_workspace_bytes(-1, 8) == 0


def test_argument_errors_are_return_codes_before_any_hip_call(lib):
    """every call below fails its checks first: the pointers are never dereferenced and no HIP call is made (no GPU here)"""
    p = C.c_void_p(16)
    big = (1 << 31) // 3 + 1                                   # 3 * big >= 2^31

    def surface(V=3, F=1, lo=-1.0, hi=1.0, R=8, flags=0, ws=p, bits=p):
        return lib.surfd_voxel_surface(p, V, p, F, lo, hi, R, flags, ws, bits, None, None, None)

    def solid(V=3, F=1, lo=-1.0, hi=1.0, R=8, flags=0, ws=p, bits=p):
        return lib.surfd_voxel_solid(p, V, p, F, lo, hi, R, flags, ws, 1, bits, None, None, None)

    for fn, name in ((surface, b"surfd_voxel_surface"), (solid, b"surfd_voxel_solid")):
        for kw, word in (({"R": 0}, b"R = 0"), ({"R": 513}, b"R = 513"), ({"R": -3}, b"R = -3"), ({"lo": 1.0, "hi": 1.0}, b"lo < hi"),
                         ({"lo": 1.0, "hi": -1.0}, b"lo < hi"), ({"hi": float("nan")}, b"lo < hi"), ({"flags": 3}, b"exclude each other"),
                         ({"flags": 4}, b"flags = 4"), ({"F": big}, b"2^31"), ({"V": big}, b"2^31"), ({"V": -1}, b"negative"),
                         ({"ws": None}, b"null workspace"), ({"bits": None}, b"null workspace or bits")):
            assert fn(**kw) == SURFD_ERR_ARG, (name, kw)
            msg = lib.surfd_last_error()
            assert name in msg and word in msg, (kw, msg)
    assert lib.surfd_voxel_surface(None, 3, p, 1, -1.0, 1.0, 8, 0, p, p, None, None, None) == SURFD_ERR_ARG
    for kw in ({"R": 0}, {"R": 513}, {"lo": 0.5, "hi": 0.5}, {"P": big}, {"P": -1}, {"bits": None}):
        a = {"P": 4, "lo": -1.0, "hi": 1.0, "R": 8, "bits": p, **kw}
        assert lib.surfd_voxel_points(p, a["P"], a["lo"], a["hi"], a["R"], a["bits"], None, None) == SURFD_ERR_ARG, kw
        assert b"surfd_voxel_points" in lib.surfd_last_error()
    for M, Nn, R, paired, word in ((1, 1, 0, 0, b"R = 0"), (1, 1, 513, 0, b"R = 513"), (2, 3, 8, 1, b"M = N"), (-1, 1, 8, 0, b"negative"),
                                   (65536, 65536, 8, 0, b"2^31")):
        assert lib.surfd_voxel_iou(p, M, p, Nn, R, paired, p, p, p, None) == SURFD_ERR_ARG, (M, Nn, R, paired)
        assert b"surfd_voxel_iou" in lib.surfd_last_error() and word in lib.surfd_last_error()
    assert lib.surfd_voxel_iou(p, 1, p, 1, 8, 0, None, p, p, None) == SURFD_ERR_ARG
    assert lib.surfd_voxel_iou(p, 0, p, 0, 8, 1, None, None, None, None) == 0             # nothing to do


def test_kernels_do_not_spill():
    meta = _tool("kernel_regs").kernel_metadata()
    names = sorted(k for k in meta if "surfd::vx_" in k)
    want = ["vx_iou_finish_kernel", "vx_iou_kernel", "vx_points_kernel", "vx_solid_large_kernel", "vx_solid_merge_kernel",
            "vx_solid_small_kernel", "vx_surface_large_kernel", "vx_surface_small_kernel"]
    assert len(names) == len(want) and all(any(w + "(" in k for k in names) for w in want), names
    for k in names:
        v = meta[k]
        assert v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".private_segment_fixed_size"] == 0, (k, v)


# ---- 2. the restatement against the Python-integer form -----------------------------------------------------------------------------
M = X.SNAP_MAX
EXTREME = [
    [[-M, -M, -M], [M, M, -M + 300], [-M, M, M]],              # the longest edges the snap admits, through the grid
    [[M, -M, M], [-M, M, M - 1], [-M, -M, -M]],
    [[-M, M, 1000], [M, -M, 1001], [M, M, 999]],               # nearly flat, doubled area near 2^41
    [[-M, -M, M], [M, -M, -M], [0, M, 77]],
    [[M, M, M], [M - 1, M, M], [M, M - 1, M]],                 # a sliver far outside: clipped box empty
    [[-M, 300, 500], [M, 301, 499], [0, -M, 2048]],
]


@pytest.mark.parametrize("R", [4, 8])
def test_int64_restatement_equals_big_integers_at_the_snap_limit(R):
    tri, ok = _snapped(EXTREME)
    for t in tri:
        n = X.normal(t)
        big = X._cross([int(x) for x in t[1] - t[0]], [int(x) for x in t[2] - t[0]])
        assert tuple(int(x) for x in n) == big                 # the area vector itself did not wrap
    assert max(abs(int(x)) for t in tri for x in X.normal(t)) == 2 ** 40      # the doubled area of half the square [-2^19, 2^19]^2: the maximum
    got = X.surface_snapped(tri, ok, R)
    assert np.array_equal(got["dense"], X.surface_big(tri, ok, R)) and got["dense"].any()
    assert got["dropped"] == 0 and got["degenerate"] == 0
    s = X.solid_snapped(tri, ok, R)
    fill, parity = X.solid_big(tri, ok, R)
    assert np.array_equal(s["fill"], fill) and np.array_equal(s["parity"], parity) and parity.any()


def test_restatement_equals_big_integers_on_the_rule_cases():
    R = 8
    for tris in (X.PLANE_TRIANGLE, X.CORNER_TRIANGLE, X.SLANTED_TRIANGLE):
        tri, ok = X.snap_mesh(tris, [[0, 1, 2]], 0.0, float(R), R)
        assert np.array_equal(tri[0], (tris.astype(np.float64) * 256).astype(np.int64))          # bounds (0, R): q = 256 x
        assert np.array_equal(X.surface_snapped(tri, ok, R)["dense"], X.surface_big(tri, ok, R))
    v, f = X.octahedron((4.5, 4.5, 4.0), 3.0)
    tri, ok = X.snap_mesh(v, f, 0.0, float(R), R)
    s = X.solid_snapped(tri, ok, R)
    fill, parity = X.solid_big(tri, ok, R)
    assert np.array_equal(s["fill"], fill) and np.array_equal(s["parity"], parity)
    assert np.array_equal(X.surface_snapped(tri, ok, R)["dense"], X.surface_big(tri, ok, R))


# ---- 3. the rules, on the restatement itself ----------------------------------------------------------------------------------------
def test_surface_rules_of_the_restatement():
    R = 8
    d = X.surface_ref(X.PLANE_TRIANGLE, [[0, 1, 2]], R, X.VOXEL_UNITS(R))["dense"]
    assert d[:, :, 2].any() and np.array_equal(d[:, :, 2], d[:, :, 3]) and not d[:, :, :2].any() and not d[:, :, 4:].any()
    d = X.surface_ref(X.CORNER_TRIANGLE, [[0, 1, 2]], R, X.VOXEL_UNITS(R))["dense"]
    want = np.zeros((R, R, R), bool)
    want[3:5, 3:5, 3:5] = True
    assert np.array_equal(d, want)
    tri, ok = X.snap_mesh(X.SLANTED_TRIANGLE, [[0, 1, 2]], 0.0, float(R), R)
    i, j, k = (np.array([x], np.int64) for x in X.SLANTED_CLEAR)
    box, plane, edges = X.sat_parts(tri[0], i, j, k)
    assert box[0] and plane[0] and not edges[0]
    d = X.surface_snapped(tri, ok, R)["dense"]
    assert not d[X.SLANTED_CLEAR] and d.any()
    assert X.slanted_search()[1] == X.SLANTED_CLEAR and np.array_equal(X.slanted_search()[0], X.SLANTED_TRIANGLE)
    # a triangle through the whole grid touches both far corners; one wholly outside sets nothing and is not "dropped"
    d = X.surface_ref(X.SPANNING_TRIANGLE, [[0, 1, 2]], R, (0.0, 1.0))["dense"]
    assert d[0, 0, 0] and d[R - 1, R - 1, 1] and d[0, R - 1, R - 1] and not d[R - 1, 0, R - 1]
    r = X.surface_ref(X.SPANNING_TRIANGLE + np.float32(1.5), [[0, 1, 2]], R, (0.0, 1.0))
    assert not r["dense"].any() and r["dropped"] == 0


def test_counters_of_the_restatement():
    R = 8
    v = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [1, 1, 1], [np.nan, 0, 0], [3e5, 0, 0], [0.25, 0, 0]], np.float32)
    f = [[0, 1, 2],                                            # fine
         [0, 1, 6], [3, 3, 3], [0, 0, 1],                      # collinear, a point, a repeated vertex: degenerate
         [0, 1, 4], [0, 5, 2],                                 # NaN, snapped beyond 2^19: dropped
         [0, 1, 7], [-1, 1, 2], [0, 2 ** 31 - 1, 2]]           # indices outside [0, V): dropped, never read
    r = X.surface_ref(v, f, R)
    assert (r["dropped"], r["degenerate"]) == (5, 3) and r["dense"].any()
    assert np.array_equal(r["dense"], X.surface_ref(v, f[:1], R)["dense"])
    s = X.solid_ref(v, f, R)
    assert s["dropped"] == 5
    tri, ok = X.snap_mesh(v, f, -1.0, 1.0, R)
    assert ok.tolist() == [True] * 4 + [False] * 5
    # the snap limit itself: |q| = 2^19 is valid, one unit more is not
    q, valid = X.snap(np.array([2.0 ** 19 / 256, 2.0 ** 19 / 256 + 1 / 256, -2.0 ** 19 / 256], np.float32), 0.0, float(R), R)
    assert valid.tolist() == [True, False, True] and q[0] == 2 ** 19 and q[2] == -2 ** 19
    assert X.snap(np.array([0.5 / 256, 1.5 / 256, 2.5 / 256], np.float32), 0.0, float(R), R)[0].tolist() == [0, 2, 2]     # ties to even


def test_solid_rules_of_the_restatement():
    R = 8
    U = X.VOXEL_UNITS(R)
    s = X.solid_ref(*X.box_mesh((1, 2, 3), (4, 4, 7)), R, U, include_surface=False)
    want = np.zeros((R, R, R), bool)
    want[1:4, 2:4, 3:7] = True                                 # faces on voxel boundaries: exactly w h d voxels
    assert np.array_equal(s["fill"], want) and s["odd_columns"] == 0
    # faces exactly through voxel centres: a centre ON the crossing is not strictly above it, so the lower face's layer is
    # left out and the upper face's layer is filled; in x and y the top-left rule gives the lower side and not the upper
    s = X.solid_ref(*X.box_mesh((1.5, 1.5, 1.5), (4.5, 4.5, 4.5)), R, U, include_surface=False)
    want = np.zeros((R, R, R), bool)
    want[1:4, 1:4, 2:5] = True
    assert np.array_equal(s["fill"], want) and s["odd_columns"] == 0
    # an octahedron whose apex and edges pass through column centres: each crossing once
    s = X.solid_ref(*X.octahedron((4.5, 4.5, 4.0), 3.0), R, U, include_surface=False)
    assert s["odd_columns"] == 0 and s["fill"].any() and not (s["fill"].sum(2) % 2).any()      # symmetric about z = 4
    assert s["fill"][4, 4].tolist() == [False, True, True, True, True, True, True, False]
    # nested boxes: hollow
    vo, fo = X.box_mesh((1, 1, 1), (7, 7, 7))
    vi, fi = X.box_mesh((3, 3, 3), (5, 5, 5))
    s = X.solid_ref(np.concatenate([vo, vi]), np.concatenate([fo, fi + 8]), R, U, include_surface=False)
    assert s["fill"].sum() == 6 ** 3 - 2 ** 3 and not s["fill"][3:5, 3:5, 3:5].any() and s["odd_columns"] == 0
    # an open box (the +z lid removed) leaks: odd columns exactly under the missing lid
    v, f = X.box_mesh((1, 2, 3), (4, 4, 7))
    lid = [n for n, t in enumerate(f) if (v[t][:, 2] == 7).all()]
    s = X.solid_ref(v, np.delete(f, lid, 0), R, U, include_surface=False)
    assert s["odd_columns"] == 3 * 2


def test_points_and_iou_rules_of_the_restatement():
    R = 8
    pts = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [8.0, 8.0, 8.0], [8.0, 0.5, 0.5], [8.004, 1, 1], [-0.004, 1, 1], [np.nan, 1, 1], [2.99, 3.0, 3.01]], np.float32)
    r = X.points_ref(pts, R, X.VOXEL_UNITS(R))
    assert sorted(zip(*np.nonzero(r["dense"]))) == [(0, 0, 0), (1, 2, 3), (2, 3, 3), (7, 0, 0), (7, 7, 7)] and r["outside"] == 3
    a = np.zeros((2, R, R, R), bool)
    a[0, :4] = True
    a[1, 2:6] = True
    pa = X.pack(a)
    assert np.array_equal(X.unpack(pa, R), a)
    inter, union, iou = X.iou_ref(pa, pa)
    assert inter.tolist() == [[256, 128], [128, 256]] and union.tolist() == [[256, 384], [384, 256]]
    assert iou.dtype == np.float32 and iou[0, 1] == np.float32(128) / np.float32(384)
    assert X.iou_ref(X.pack(np.zeros((1, R, R, R), bool)), X.pack(np.zeros((1, R, R, R), bool)))[2].tolist() == [[1.0]]
    assert X.pack(np.ones((40, 40, 40), bool))[0, 0].tolist() == [0xFFFFFFFF, 0xFF]         # padding bits stay clear


# ---- 4. the module's refusals (no GPU needed) -------------------------------------------------------------------------------------
def test_module_refuses_cpu_tensors_and_bad_input():
    from surfd_amd import voxelize as VZ
    v, f = (torch.from_numpy(a) for a in X.box_mesh((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)))
    for call in (lambda: VZ.voxelize_surface(v, f), lambda: VZ.voxelize_solid(v, f), lambda: VZ.voxelize_points(v),
                 lambda: VZ.is_closed(v, f, 16), lambda: VZ.voxel_iou(VZ.VoxelGrid.empty(8, device="cpu"), VZ.VoxelGrid.empty(8, device="cpu")),
                 lambda: VZ.voxel_iou_matrix(torch.zeros(2, 8, 8, 1, dtype=torch.int32), torch.zeros(3, 8, 8, 1, dtype=torch.int32)),
                 lambda: VZ.VoxelGrid.empty(8, device="cpu").count()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="float32"):
        VZ.voxelize_surface(v.double(), f)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        VZ.voxelize_surface(v, f.reshape(-1))
    with pytest.raises(ValueError, match="resolution"):
        VZ.voxelize_surface(v, f, 513)
    with pytest.raises(ValueError, match="lo < hi"):
        VZ.voxelize_points(v, 8, (1.0, 1.0))
    with pytest.raises(ValueError, match="path"):
        VZ.voxelize_surface(v, f, path="medium")
    src = open(os.path.join(ROOT, "surfd_amd", "voxelize.py")).read()
    assert "oracle" not in src


def test_voxelgrid_layout_round_trip_on_the_host():
    """from_dense / dense are layout changes in torch and work on any device; they agree with the restatement's pack / unpack"""
    from surfd_amd import voxelize as VZ
    for R in (8, 32, 40):
        d = np.random.default_rng(R).random((R, R, R)) < 0.3
        g = VZ.VoxelGrid.from_dense(torch.from_numpy(d), bounds=(0.0, 1.0))
        assert g.resolution == R and g.bounds == (0.0, 1.0) and g.packed.dtype == torch.int32 and tuple(g.packed.shape) == (R, R, VZ.words(R))
        assert np.array_equal(g.packed.numpy().view(np.uint32), X.pack(d))
        assert np.array_equal(g.dense().numpy(), d)


# ---- 5. the example driver's frame (no GPU needed) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "bbox", "unit_sphere"])
def test_evaluate_applies_the_reference_items_transform(mode):
    """--voxel_iou voxelises both items of a pair in the reference item's frame: reference_frame() is the transform
    cloudmetrics.normalize_clouds applies to that item, and the options parse with their defaults"""
    from examples import evaluate as E
    from surfd_amd import cloudmetrics
    x = torch.from_numpy(np.random.default_rng(5).normal(size=(200, 3)).astype(np.float32)) * torch.tensor([1.0, 3.0, 0.5]) + 2.0
    c, r = E.reference_frame(x, mode)
    assert torch.allclose((x - c) / r, cloudmetrics.normalize_clouds(x, mode), atol=1e-6)
    a = E.parse(["--generated", "g", "--reference", "r"])
    assert a.voxel_iou == 0 and tuple(a.voxel_bounds) == (-1.0, 1.0) and a.voxel_mode == "surface"
    a = E.parse(["--generated", "g", "--reference", "r", "--voxel_iou", "64", "--voxel_bounds", "-2", "2", "--voxel_mode", "solid"])
    assert a.voxel_iou == 64 and list(a.voxel_bounds) == [-2.0, 2.0] and a.voxel_mode == "solid"
    with pytest.raises(SystemExit, match="--paired"):
        E.run(a)
