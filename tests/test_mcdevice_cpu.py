"""What of the device marching cubes (csrc/mcdevice.hip) can be checked without a GPU: the exports, the
refusals, the unchanged signature of get_watertight_mesh, and the property of the case tables that the kernels' index
arithmetic rests on."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from surfd_amd import _native as N

# corner pairs of the twelve cube edges, marching-cubes numbering
EDGE_CORNERS = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
# the fans a case may end in (mcubes.cpp: choose), with the triangles choose() names for each
FANS_OF_CASE = {1: [("TILING1", 1)], 2: [("TILING2", 2)], 3: [("TILING3_1", 2), ("TILING3_2", 4)], 4: [("TILING4_1", 2), ("TILING4_2", 6)],
                5: [("TILING5", 3)], 6: [("TILING6_1_1", 3), ("TILING6_1_2", 9), ("TILING6_2", 5)],
                7: [("TILING7_1", 3), ("TILING7_2", 5), ("TILING7_3", 9), ("TILING7_4_1", 5), ("TILING7_4_2", 9)],
                8: [("TILING8", 2)], 9: [("TILING9", 4)],
                10: [("TILING10_1_1", 4), ("TILING10_1_1_", 4), ("TILING10_1_2", 8), ("TILING10_2", 8), ("TILING10_2_", 8)], 11: [("TILING11", 4)],
                12: [("TILING12_1_1", 4), ("TILING12_1_1_", 4), ("TILING12_1_2", 8), ("TILING12_2", 8), ("TILING12_2_", 8)],
                13: [("TILING13_1", 4), ("TILING13_1_", 4), ("TILING13_2", 6), ("TILING13_2_", 6), ("TILING13_3", 10), ("TILING13_3_", 10),
                     ("TILING13_4", 12), ("TILING13_5_1", 6), ("TILING13_5_2", 10)], 14: [("TILING14", 4)]}


def crossing_edges(pattern):
    return {e for e, (a, b) in enumerate(EDGE_CORNERS) if ((pattern >> a) ^ (pattern >> b)) & 1}


def test_new_exports_are_bound_with_their_signatures():
    P = C.c_void_p
    i64p = C.POINTER(C.c_int64)
    want = {"surfd_mcd_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(P)]),
            "surfd_mcd_destroy": (None, [P]),
            "surfd_mcd_run": (C.c_int, [P, P, C.c_double, C.c_int, P, i64p, i64p]),
            "surfd_mcd_emit": (C.c_int, [P, P, P, P, P, P]),
            "surfd_mcd_active": (C.c_int, [P, i64p]),
            "surfd_mcd_classify": (C.c_int, [P, P, C.c_double, C.c_int, P])}
    for name, sig in want.items():
        assert name in N.EXPORTED_SYMBOLS, name
        assert N._SIGS[name] == sig, name
        assert hasattr(N.lib(), name), name


def test_create_refuses_what_it_cannot_hold():
    L = N.lib()
    h = C.c_void_p()
    assert L.surfd_mcd_create(4, 1, 4, C.byref(h)) == -1 and h.value is None            # an extent of 1
    assert L.surfd_mcd_create(2048, 1024, 1024, C.byref(h)) == -4 and h.value is None    # 2^31 voxels
    assert L.surfd_mcd_emit(None, None, None, None, None, None) == -1


def test_marching_cubes_device_refuses_cpu_and_malformed_input():
    from surfd_amd.mcubes import marching_cubes_device
    with pytest.raises(ValueError, match="no CPU fallback"):
        marching_cubes_device(torch.zeros(4, 4, 4), 0.0)
    with pytest.raises(ValueError):
        marching_cubes_device(np.zeros((4, 4, 4), np.float32), 0.0)


def test_get_watertight_mesh_device_refuses_a_cpu_grid(monkeypatch):
    """the grid of a filler that lives on the host is not meshed there behind the caller's back"""
    from surfd_amd import meshudf

    class HostFiller:
        def __init__(self, n):
            self.n = n

        def fill_grid(self, udf_func, max_batch, with_grads=True):
            return torch.ones(self.n, self.n, self.n), None

    monkeypatch.setattr(meshudf, "GridFiller", HostFiller)
    with pytest.raises(ValueError, match="no CPU fallback"):
        meshudf.get_watertight_mesh(lambda c: c[:, 0], 8, device=True)
    v, f = meshudf.get_watertight_mesh(lambda c: c[:, 0], 8)                                # the host path is as it was
    assert isinstance(v, np.ndarray) and v.shape == (0, 3) and f.shape == (0, 3)


def test_get_watertight_mesh_keeps_its_parameters_and_defaults():
    from surfd_amd.meshudf import get_watertight_mesh
    p = inspect.signature(get_watertight_mesh).parameters
    names = list(p)
    assert names[:6] == ["udf_func", "N", "max_batch", "level", "normalize", "classic"]
    assert [p[n].default for n in names[2:6]] == [2 ** 16, 0.01, False, True]
    assert names[6:] == ["device", "min_faces"] and p["device"].default is False and p["min_faces"].default is None


def test_every_fan_names_exactly_the_crossing_edges_of_its_pattern():
    """The kernels find the cube that creates an edge's vertex by index arithmetic: the first in-range cube around the edge.
    That is the first cube that NAMES the edge only if every fan a cube can end in names every edge of the cube whose corners
    lie on different sides (and no other edge, else a cube could look for a vertex that no cube makes).  Every row of every
    table, every sub-configuration; edge 12 is the cube's own interior vertex."""
    from surfd_amd.mcubes import lut_tables
    T = lut_tables()
    classic, cases = T["CASESCLASSIC"], T["CASES"]
    assert classic.shape == (256, 16) and cases.shape == (256, 2)
    rows_checked = 0
    for pattern in range(256):
        want = crossing_edges(pattern)
        row = [int(e) for e in classic[pattern]]
        n = row.index(-1)
        assert n % 3 == 0 and n <= 15 and all(e == -1 for e in row[n:])
        assert set(row[:n]) == want, ("classic", pattern)
        assert (n == 0) == (pattern in (0, 255))
        mc_case, config = int(cases[pattern, 0]), int(cases[pattern, 1])
        assert (mc_case <= 0) == (pattern in (0, 255)), pattern
        if mc_case <= 0:
            continue
        for name, nt in FANS_OF_CASE[mc_case]:
            t = T[name]
            assert t.shape[-1] == 3 * nt, name                      # the triangle count choose() names is the row's length
            fans = t[config].reshape(-1, 3 * nt)                     # one row, or one per sub-configuration
            for fan in fans:
                assert set(int(e) for e in fan) - {12} == want, (name, pattern, config)
                assert all(0 <= int(e) <= 12 for e in fan)
                rows_checked += 1
    assert rows_checked > 700
    # every table of fans was visited through some pattern
    assert {n for fans in FANS_OF_CASE.values() for n, _ in fans} == {n for n in T if n.startswith("TILING")}
