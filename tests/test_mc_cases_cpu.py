"""The plain port of Lewiner's case analysis (tests/mc_cases_ref.py) against the host mesher, and the census of the fan bank
(tests/golden/mc_fan_bank.npz, written by tools/make_mc_fan_bank.py).

The port earns its trust here: for a 2x2x2 volume the host mesh's faces must be the fan row the port names, edges numbered by
first appearance and every triangle reversed, and the vertex count the number of distinct edges of that row.  If the two
disagree, one of them is wrong.  The GPU tests (tests/test_gpu_mcdevice.py) then use the port to say what their volumes reach."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_cases_ref as R  # noqa: E402

BANK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc_fan_bank.npz")

# ---- the census: conditions, not measurements ------------------------------------------------------------------------------------
# the fans the bank must reach: (table, sub-index or None)
SUBS = {"TILING7_2": 3, "TILING7_3": 3, "TILING13_2": 6, "TILING13_2_": 6, "TILING13_3": 12, "TILING13_3_": 12, "TILING13_4": 4,
        "TILING13_5_1": 4}
REQUIRED_FANS = {(n, None) for n in (
    "TILING1", "TILING2", "TILING3_1", "TILING3_2", "TILING4_1", "TILING4_2", "TILING5", "TILING6_1_1", "TILING6_1_2", "TILING6_2",
    "TILING7_1", "TILING7_4_1", "TILING7_4_2", "TILING8", "TILING9", "TILING10_1_1", "TILING10_1_1_", "TILING10_1_2", "TILING10_2",
    "TILING10_2_", "TILING11", "TILING12_1_1", "TILING12_1_1_", "TILING12_2", "TILING12_2_", "TILING13_1", "TILING13_1_", "TILING14")}
REQUIRED_FANS |= {(n, s) for n, subs in SUBS.items() for s in range(subs)}
# The five fans of the 83 that are not reached by the search (384 000 mixed-magnitude draws), nor by any other input tried:
#     TILING12_1_2                   not reached by the search
#     TILING13_5_2[0], [1], [2], [3] not reached by the search
# For cases 12 and 13 test_interior has only ever left through test == 1 or test == 5 with the product below TINY, and both
# return s > 0; the fans look dead by construction.  They are NOT asserted unreachable: a search that reaches one adds it above.
NOT_REACHED = {("TILING12_1_2", None)} | {("TILING13_5_2", s) for s in range(4)}
# the exits of test_interior the bank must reach: (case, exit), exits as mc_cases_ref names them
REQUIRED_EXITS = {(4, e) for e in ("t", "0", "1", "2", "4", "5a", "5b", "7", "8", "10a", "10b", "11", "13", "14", "15")}
REQUIRED_EXITS |= {(6, e) for e in ("1", "3", "5a", "7", "9", "11", "13", "15")}
REQUIRED_EXITS |= {(7, e) for e in ("1", "3", "5a", "9", "11")}
REQUIRED_EXITS |= {(10, e) for e in ("t", "0", "1", "2", "3", "4", "5a", "5b", "6", "8", "9", "10a", "10b", "12")}
REQUIRED_EXITS |= {(12, "1"), (12, "5a"), (13, "5a")}


def host(volume, classic=False, level=0.0):
    from surfd_amd import mcubes
    return mcubes._run(np.ascontiguousarray(volume, np.float32), None, 1, level, classic)


def assert_port_is_the_host(cube, classic, what):
    """cube: fp32 [8] in marching-cubes order, level 0"""
    a = R.analyse(cube.astype(np.float64), classic)
    faces, nv = R.expected_mesh(a)
    v, f, n, s = host(R.cube_volume(cube), classic)
    assert f.shape == faces.shape and np.array_equal(f, faces), (what, cube.tolist(), a, f.tolist(), faces.tolist())
    assert len(v) == nv == len(n) == len(s), (what, cube.tolist(), a, len(v), nv)
    return a


@pytest.fixture(scope="module")
def bank():
    cubes = np.load(BANK, allow_pickle=False)["cubes"]
    assert cubes.dtype == np.float32 and cubes.ndim == 2 and cubes.shape[1] == 8 and np.isfinite(cubes).all()
    return cubes


def test_required_lists_are_the_78_and_45_of_the_83_fans():
    T = R.tables()
    every = set()
    for name, t in T.items():
        if name.startswith("TILING"):
            every |= {(name, s) for s in range(len(t[0]))} if isinstance(t[0][0], list) else {(name, None)}
    assert len(every) == 83 and len(REQUIRED_FANS) == 78 and len(NOT_REACHED) == 5 and len(REQUIRED_EXITS) == 45
    assert REQUIRED_FANS | NOT_REACHED == every and not REQUIRED_FANS & NOT_REACHED


@pytest.mark.parametrize("classic", [False, True])
def test_port_equals_host_on_every_bank_cube(bank, classic):
    for i, cube in enumerate(bank):
        assert_port_is_the_host(cube, classic, f"bank cube {i}")


def test_bank_meets_the_census(bank):
    analyses = [R.analyse(c.astype(np.float64)) for c in bank]
    fans = {(a.fan[0], a.fan[1]) for a in analyses if a.fan[0] is not None}
    exits = {(a.case, a.interior) for a in analyses if a.interior is not None}
    assert not REQUIRED_FANS - fans, sorted(REQUIRED_FANS - fans, key=str)
    assert not REQUIRED_EXITS - exits, sorted(REQUIRED_EXITS - exits)
    assert {a.pattern for a in analyses} == set(range(256))
    # should a later search reach one of the five, it belongs in REQUIRED_FANS
    assert not fans & NOT_REACHED, sorted(fans & NOT_REACHED, key=str)
    # every face test of every case went all three ways: tie, true, false
    slots = {3: 1, 6: 1, 7: 3, 10: 2, 12: 2, 13: 6}
    seen = {(a.case, slot, outcome) for a in analyses for slot, (_, outcome) in enumerate(a.face_tests)}
    assert seen == {(c, s, o) for c, n in slots.items() for s in range(n) for o in ("tie", "true", "false")}
    # and the census helpers of the GPU tests count the same thing
    assert R.census(bank.astype(np.float64)) == (fans, exits)


def test_port_equals_host_on_20000_mixed_magnitude_draws():
    """the generator's own mixture (log-uniform, a discrete set from 1e-12 to 1e6, U(0,1)^4 + 1e-9) under another seed; patterns in
    turn, so every pattern gets 78 draws"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_mc_fan_bank as G
    rng = np.random.default_rng(77)
    fans = set()
    for i in range(20000):
        cube = G.draw(rng, i % 256, (i // 256) % 3)
        a = assert_port_is_the_host(cube, False, f"draw {i}")
        fans.add(a.fan[:2])
        if i % 16 == 0:
            assert_port_is_the_host(cube, True, f"draw {i}, classic")
    assert len(fans) > 36          # the draws were not tame: U(0.05, 1) magnitudes over all patterns reach 36 fans


def test_cubes_of_orders_corners_as_cube_volume_does(bank):
    for cube in bank[:40]:
        got = R.cubes_of(R.cube_volume(cube), 0.0)
        assert got.shape == (1, 8) and np.array_equal(got[0], cube.astype(np.float64))
    assert np.array_equal(R.cubes_of(R.cube_volume(bank[0]), 0.25)[0], bank[0].astype(np.float64) - 0.25)
