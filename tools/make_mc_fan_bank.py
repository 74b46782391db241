#!/usr/bin/env python3
"""Writes tests/golden/mc_fan_bank.npz: single cubes that drive Lewiner's case analysis (csrc/mcubes.cpp: choose, test_face,
test_interior; restated on the device in csrc/mcdevice.hip) down every way a seeded search finds.

The search loops over all 256 sign patterns and cycles the corner magnitudes through three draws:
    0  log-uniform over [1e-6, 1e3]
    1  a discrete set {1e-12, 1e-6, 1e-3, 0.1, 0.5, 1, 2, 10, 1e3, 1e6}
    2  U(0, 1)^4 + 1e-9
Draws of the patterns whose case has one fan need no look at the tests once that fan has its cubes.  Every other draw is meshed
by the host mesher of the library, through ctypes, as a 2x2x2 volume at level 0, and classified by the plain port
tests/mc_cases_ref.py, whose fan must give the host's faces: a disagreement stops the search.  For every
distinct key — (fan table, sub), (case, interior exit), (case, face-test slot, outcome, ties included), and the pattern itself —
the first three cubes seen are kept (the first one for a pattern).  The result is data: fp32 [n, 8], corner values in
marching-cubes order.

    python tools/make_mc_fan_bank.py [--rounds 500] [--seed 2024]

prints the census (tests/test_mc_cases_cpu.py holds it as a condition)."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

DISCRETE = np.array([1e-12, 1e-6, 1e-3, 0.1, 0.5, 1, 2, 10, 1e3, 1e6])
KEEP = 3
ONE_FAN_CASES = (1, 2, 5, 8, 9, 11, 14)


def magnitudes(rng, kind):
    if kind == 0:
        return 10.0 ** rng.uniform(-6.0, 3.0, size=8)
    if kind == 1:
        return rng.choice(DISCRETE, size=8)
    return rng.uniform(0.0, 1.0, size=8) ** 4 + 1e-9


def draw(rng, pattern, kind):
    """fp32 [8]: the signs of `pattern`, magnitudes of draw `kind`"""
    sign = np.array([1.0 if (pattern >> k) & 1 else -1.0 for k in range(8)])
    return (sign * magnitudes(rng, kind)).astype(np.float32)


def search(rounds, seed):
    import mc_cases_ref as R
    from surfd_amd import mcubes
    T = R.tables()
    rng = np.random.default_rng(seed)
    kept, index, count = [], {}, {}
    draws = classified = 0

    def keep(cube, keys):
        for key in keys:
            limit = 1 if key[0] == "pattern" else KEEP
            if count.get(key, 0) >= limit:
                continue
            count[key] = count.get(key, 0) + 1
            b = cube.tobytes()
            if b not in index:
                index[b] = len(kept)
                kept.append(cube)

    for _ in range(rounds):
        for kind in range(3):
            for pattern in range(256):
                cube = draw(rng, pattern, kind)
                draws += 1
                if count.get(("pattern", pattern), 0) == 0:
                    keep(cube, [("pattern", pattern)])
                mc_case = T["CASES"][pattern][0]
                if mc_case <= 0:
                    continue
                if mc_case in ONE_FAN_CASES and count.get(("fan", "TILING%d" % mc_case, None), 0) >= KEEP:
                    continue
                _, faces, _, _ = mcubes._run(R.cube_volume(cube), None, 1, 0.0, False)
                a = R.analyse(cube.astype(np.float64))
                classified += 1
                want, _ = R.expected_mesh(a)
                if not np.array_equal(faces, want):
                    raise SystemExit(f"the port and the host mesher disagree on {cube.tolist()}: {a}")
                keep(cube, R.keys_of(a))
    return np.stack(kept), count, draws, classified


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=500, help="rounds of 3 draws x 256 patterns (500: 384 000 draws)")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "mc_fan_bank.npz"))
    args = ap.parse_args()
    cubes, count, draws, classified = search(args.rounds, args.seed)
    fans = sorted((k[1], -1 if k[2] is None else k[2]) for k in count if k[0] == "fan")
    exits = sorted((k[1], k[2]) for k in count if k[0] == "interior")
    faces = sorted(k[1:] for k in count if k[0] == "face")
    print(f"{draws} draws, {classified} classified, {len(cubes)} cubes kept")
    print(f"{len(fans)} fans: {fans}")
    print(f"{len(exits)} interior exits: {exits}")
    print(f"{len(faces)} face-test outcomes: {faces}")
    np.savez_compressed(args.out, cubes=cubes, seed=np.int64(args.seed), rounds=np.int64(args.rounds))
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
