"""Lewiner's case analysis, restated plainly in Python fp64 from csrc/mcubes.cpp (test_face, test_interior, choose): which fan a
cube ends in, and by which way through the tests it got there.  Python floats are IEEE doubles and nothing here is contracted,
so every comparison below is the host's own.  The tables come from the library (`surfd_amd.mcubes.lut_tables()`); the only
constants restated are TINY and the corner table P of test_interior.

  analyse(v)            v: the eight corner values MINUS THE LEVEL, fp64, marching-cubes corner order -> Analysis
  expected_mesh(...)    the faces and vertex count the host mesher gives for a 2x2x2 volume that holds this one cube
  cube_volume(v)        the 2x2x2 volume whose only cube has corners v

tests/test_mc_cases_cpu.py ties this file to the host mesher, face for face."""
import collections
import functools

import numpy as np

TINY = 2.220446049250313e-16
P = ((0, 1, 3, 2, 7, 6, 4, 5), (1, 2, 0, 3, 4, 7, 5, 6), (2, 3, 1, 0, 5, 4, 6, 7), (3, 0, 2, 1, 6, 5, 7, 4),
     (4, 5, 7, 6, 3, 2, 0, 1), (5, 6, 4, 7, 0, 3, 1, 2), (6, 7, 5, 4, 1, 0, 2, 3), (7, 4, 6, 5, 2, 1, 3, 0),
     (0, 4, 3, 7, 2, 6, 1, 5), (1, 5, 0, 4, 3, 7, 2, 6), (2, 6, 1, 5, 0, 4, 3, 7), (3, 7, 2, 6, 1, 5, 0, 4))
# test_face: the corners A, B, C, D of faces 1 .. 6
FACE_CORNERS = {1: (0, 4, 5, 1), 2: (1, 5, 6, 2), 3: (2, 6, 7, 3), 4: (3, 7, 4, 0), 5: (0, 3, 2, 1), 6: (4, 7, 6, 5)}

# Analysis.fan: (table name, sub-index or None, config); face_tests: [(face as the TEST table names it, "tie" | "true" | "false")] in
# the order made; interior: None where no interior test ran, "t" where t left [0, 1] (cases 4 and 10), else "0" .. "15" with "5a" /
# "10a" where the product test of 5 / 10 held (-> s > 0) and "5b" / "10b" where it did not (-> false)
Analysis = collections.namedtuple("Analysis", "pattern case config fan nt face_tests interior")


@functools.lru_cache(maxsize=None)
def tables():
    from surfd_amd.mcubes import lut_tables
    return {k: v.tolist() for k, v in lut_tables().items()}


def _div(a, b):
    """a / b as the hardware divides: no exception at b == 0"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return float("nan")
    neg = (a < 0.0) != (np.signbit(b))
    return float("-inf") if neg else float("inf")


def pattern_of(v):
    return sum(1 << k for k in range(8) if v[k] > 0.0)


def test_face(v, face, log):
    a, b, c, d = (v[k] for k in FACE_CORNERS[abs(face)])
    q = a * c - b * d
    if -TINY < q < TINY:
        log.append((face, "tie"))
        return face >= 0
    r = face * a * q >= 0
    log.append((face, "true" if r else "false"))
    return r


test_face.__test__ = False          # (not a pytest test, whatever its name)


def test_interior(v, T, mc_case, config, subconfig, s):
    """-> (result, exit)"""
    At = Bt = Ct = Dt = 0.0
    if mc_case in (4, 10):
        a = (v[4] - v[0]) * (v[6] - v[2]) - (v[7] - v[3]) * (v[5] - v[1])
        b = v[2] * (v[4] - v[0]) + v[0] * (v[6] - v[2]) - v[1] * (v[7] - v[3]) - v[3] * (v[5] - v[1])
        t = _div(-b, 2 * a + TINY)
        if t < 0 or t > 1:
            return s > 0, "t"
        At = v[0] + (v[4] - v[0]) * t
        Bt = v[3] + (v[7] - v[3]) * t
        Ct = v[2] + (v[6] - v[2]) * t
        Dt = v[1] + (v[5] - v[1]) * t
    else:
        edge = -1
        if mc_case == 6:
            edge = T["TEST6"][config][2]
        elif mc_case == 7:
            edge = T["TEST7"][config][4]
        elif mc_case == 12:
            edge = T["TEST12"][config][3]
        elif mc_case == 13:
            edge = T["TILING13_5_1"][config][subconfig][0]
        if 0 <= edge < 12:
            p = P[edge]
            t = _div(v[p[0]], v[p[0]] - v[p[1]] + TINY)
            At = 0.0
            Bt = v[p[2]] + (v[p[3]] - v[p[2]]) * t
            Ct = v[p[4]] + (v[p[5]] - v[p[4]]) * t
            Dt = v[p[6]] + (v[p[7]] - v[p[6]]) * t
    test = (1 if At >= 0 else 0) + (2 if Bt >= 0 else 0) + (4 if Ct >= 0 else 0) + (8 if Dt >= 0 else 0)
    if test == 5:
        return (s > 0, "5a") if At * Ct - Bt * Dt < TINY else (False, "5b")
    if test == 10:
        return (s > 0, "10a") if At * Ct - Bt * Dt >= TINY else (False, "10b")
    if test in (7, 11, 13, 14, 15):
        return s < 0, str(test)
    return s > 0, str(test)


test_interior.__test__ = False


def choose(v, T, mc_case, config):
    """-> (table name, sub or None, triangles, face log, interior exit or None)"""
    log = []

    def face(f):
        return test_face(v, f, log)

    def interior(sub, s):
        return test_interior(v, T, mc_case, config, sub, s)

    def out(name, sub, nt, exit_=None):
        return name, sub, nt, log, exit_

    if mc_case == 1:
        return out("TILING1", None, 1)
    if mc_case == 2:
        return out("TILING2", None, 2)
    if mc_case == 3:
        return out("TILING3_2", None, 4) if face(T["TEST3"][config]) else out("TILING3_1", None, 2)
    if mc_case == 4:
        r, e = interior(0, T["TEST4"][config])
        return out("TILING4_1", None, 2, e) if r else out("TILING4_2", None, 6, e)
    if mc_case == 5:
        return out("TILING5", None, 3)
    if mc_case == 6:
        if face(T["TEST6"][config][0]):
            return out("TILING6_2", None, 5)
        r, e = interior(0, T["TEST6"][config][1])
        return out("TILING6_1_1", None, 3, e) if r else out("TILING6_1_2", None, 9, e)
    if mc_case == 7:
        sub = 0
        for k in range(3):
            if face(T["TEST7"][config][k]):
                sub += 1 << k
        if sub == 7:
            r, e = interior(7, T["TEST7"][config][3])
            return out("TILING7_4_2", None, 9, e) if r else out("TILING7_4_1", None, 5, e)
        return {0: out("TILING7_1", None, 3), 1: out("TILING7_2", 0, 5), 2: out("TILING7_2", 1, 5), 3: out("TILING7_3", 0, 9),
                4: out("TILING7_2", 2, 5), 5: out("TILING7_3", 1, 9), 6: out("TILING7_3", 2, 9)}[sub]
    if mc_case == 8:
        return out("TILING8", None, 2)
    if mc_case == 9:
        return out("TILING9", None, 4)
    if mc_case in (10, 12):
        n = str(mc_case)
        f0 = face(T["TEST" + n][config][0])
        f1 = face(T["TEST" + n][config][1])           # made on both branches
        if f0:
            return out(f"TILING{n}_1_1_", None, 4) if f1 else out(f"TILING{n}_2", None, 8)
        if f1:
            return out(f"TILING{n}_2_", None, 8)
        r, e = interior(0, T["TEST" + n][config][2])
        return out(f"TILING{n}_1_1", None, 4, e) if r else out(f"TILING{n}_1_2", None, 8, e)
    if mc_case == 11:
        return out("TILING11", None, 4)
    if mc_case == 13:
        sub = 0
        for k in range(6):
            if face(T["TEST13"][config][k]):
                sub += 1 << k
        sub = T["SUBCONFIG13"][sub]
        if sub == 0:
            return out("TILING13_1", None, 4)
        if sub <= 6:
            return out("TILING13_2", sub - 1, 6)
        if sub <= 18:
            return out("TILING13_3", sub - 7, 10)
        if sub <= 22:
            return out("TILING13_4", sub - 19, 12)
        if sub <= 26:
            k = sub - 23
            r, e = interior(k, T["TEST13"][config][6])
            return out("TILING13_5_1", k, 6, e) if r else out("TILING13_5_2", k, 10, e)
        if sub <= 38:
            return out("TILING13_3_", sub - 27, 10)
        if sub <= 44:
            return out("TILING13_2_", sub - 39, 6)
        if sub == 45:
            return out("TILING13_1_", None, 4)
        return out(None, None, 0)
    if mc_case == 14:
        return out("TILING14", None, 4)
    return out(None, None, 0)


def analyse(v, classic=False):
    """v: eight corner values minus the level (fp64), marching-cubes order"""
    T = tables()
    v = [float(x) for x in v]
    pattern = pattern_of(v)
    if classic:
        row = T["CASESCLASSIC"][pattern]
        return Analysis(pattern, None, None, ("CASESCLASSIC", None, pattern), row.index(-1) // 3, [], None)
    mc_case, config = T["CASES"][pattern]
    if mc_case <= 0:
        return Analysis(pattern, mc_case, config, (None, None, config), 0, [], None)
    name, sub, nt, log, exit_ = choose(v, T, mc_case, config)
    return Analysis(pattern, mc_case, config, (name, sub, config), nt, log, exit_)


def fan_row(a):
    """the edges of the fan an Analysis names, three per triangle"""
    name, sub, index = a.fan
    if name is None:
        return []
    row = tables()[name][index]
    if sub is not None:
        row = row[sub]
    return [int(e) for e in row[:3 * a.nt]]


def expected_mesh(a):
    """(faces [nt, 3] int32, vertex count) of the host mesher on a volume that holds this one cube: edges numbered by first
    appearance in the fan, every triangle reversed as surfd_mc_copy hands them out"""
    row = fan_row(a)
    ids = {}
    for e in row:
        ids.setdefault(e, len(ids))
    faces = np.array([[ids[row[3 * k + 2]], ids[row[3 * k + 1]], ids[row[3 * k]]] for k in range(a.nt)], np.int32).reshape(-1, 3)
    return faces, len(ids)


def cube_volume(v):
    """corner k of the marching-cubes order sits at (x, y, z) = (((k + 1) >> 1) & 1, (k >> 1) & 1, k >> 2)"""
    vol = np.empty((2, 2, 2), np.float32)
    for k in range(8):
        vol[k >> 2, (k >> 1) & 1, ((k + 1) >> 1) & 1] = v[k]
    return vol


def cubes_of(volume, level=0.0):
    """the corner values minus the level (fp64 [cubes, 8], marching-cubes order) of every cube of a volume, in scan order"""
    d = np.asarray(volume, np.float32).astype(np.float64) - float(level)
    nz, ny, nx = d.shape
    out = np.empty((nz - 1, ny - 1, nx - 1, 8))
    for k in range(8):
        ox, oy, oz = ((k + 1) >> 1) & 1, (k >> 1) & 1, k >> 2
        out[..., k] = d[oz:oz + nz - 1, oy:oy + ny - 1, ox:ox + nx - 1]
    return out.reshape(-1, 8)


def keys_of(a):
    """what a cube contributes to a census: ("fan", table, sub), ("interior", case, exit), ("face", case, slot, outcome)"""
    keys = []
    if a.fan[0] is not None:
        keys.append(("fan", a.fan[0], a.fan[1]))
    if a.interior is not None:
        keys.append(("interior", a.case, a.interior))
    for slot, (_, outcome) in enumerate(a.face_tests):
        keys.append(("face", a.case, slot, outcome))
    return keys


def census(cubes):
    """(fans reached, interior exits reached) over fp64 cubes [n, 8]: sets of (table, sub) and (case, exit).  Cubes whose
    pattern is 0 or 255 are skipped without a look at the tables."""
    fans, exits = set(), set()
    cubes = np.asarray(cubes, np.float64)
    above = (cubes > 0.0).sum(axis=1)
    for v in cubes[(above != 0) & (above != 8)].tolist():
        a = analyse(v)
        if a.fan[0] is not None:
            fans.add((a.fan[0], a.fan[1]))
        if a.interior is not None:
            exits.add((a.case, a.interior))
    return fans, exits
