#!/usr/bin/env python3
"""Device-event timing of the self-intersection test (surfd_amd.meshintersect, csrc/meshintersect.hip) after warm-up, on the
16 896-face torus of the tests, on the same torus with a shifted copy that cuts through it, and on a torus refined to about
4 * 10^5 faces (the size of a marching-cubes mesh at 512^3): the create time and, for surfd_isect_self in its counting form and
with the pair list, the culled and the brute-force call (median of repeated calls, events on one stream), the (wave, tile)
visits that culling skipped and their total, and pair tests per second (F (F - 1) / 2 pairs over the brute-force time; the
culled time over the same number is an equivalent rate, not a count of evaluated predicates).

    python tools/meshintersect_time.py [--out profiles/meshintersect_time.json] [--reps 10]

The faces are in Morton order of their centroids, as surfd_amd.meshintersect hands them to the library; the wrapper's own
work (sorting, mapping back, the degenerate flags) is timed separately as "python_wrapper_ms".  Per-kernel times:
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import meshintersect_ref as MR  # noqa: E402
import raycast_ref as RR  # noqa: E402
from surfd_amd import _native as N  # noqa: E402
from surfd_amd.meshintersect import IntersectionScene, lattice_for  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshintersect_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--large", type=int, nargs=2, default=(480, 420), metavar=("NU", "NV"), help="the refined torus: 2 NU NV faces")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshintersect_time.py measures on the GPU"
    L = N.lib()
    torus = RR.torus(96, 88)
    meshes = [("torus 96 x 88", torus),
              ("torus 96 x 88 and a copy shifted by (0.25, 0.125, 0.0625)", MR.concatenated(torus, MR.shifted(torus, (0.25, 0.125, 0.0625)))),
              (f"torus {a.large[0]} x {a.large[1]}", RR.torus(*a.large))]
    rows = []
    for name, (v, f) in meshes:
        vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        F = len(f)
        lat = lattice_for(vd)
        r = {"mesh": name, "triangles": F, "lattice_log2": lat, "pairs": F * (F - 1) // 2}
        r["create_ms"] = timed(lambda: IntersectionScene(vd, fd, lat), a.reps)
        scene = IntersectionScene(vd, fd, lat)
        hits = torch.empty(F, device="cuda", dtype=torch.int32)
        count = torch.empty(1, device="cuda", dtype=torch.int64)
        cap = 1 << 22
        keys = torch.empty(cap, device="cuda", dtype=torch.int64)

        def call(flags, with_pairs):
            N.check(L.surfd_isect_self(scene._handle, flags, N.ptr(hits), N.ptr(keys) if with_pairs else None, cap if with_pairs else 0,
                                       N.ptr(count), N.stream()))
        for form, with_pairs in (("counting", False), ("with_pairs", True)):
            w = {}
            w["brute_force_ms"] = timed(lambda: call(1, with_pairs), max(3, a.reps // 3))
            brute = (hits.clone(), int(count), torch.sort(keys[:min(cap, int(count))]).values.clone() if with_pairs else None)
            w["culled_ms"] = timed(lambda: call(0, with_pairs), a.reps)
            same = torch.equal(hits, brute[0]) and int(count) == brute[1]
            if with_pairs:
                same = same and torch.equal(torch.sort(keys[:min(cap, int(count))]).values, brute[2])
            w["culled_equals_brute_force"] = bool(same)
            w["brute_force_pair_tests_per_s"] = r["pairs"] / (w["brute_force_ms"]["median_ms"] * 1e-3)
            w["culled_pair_tests_per_s_equivalent"] = r["pairs"] / (w["culled_ms"]["median_ms"] * 1e-3)
            w["culled_over_brute_force"] = w["brute_force_ms"]["median_ms"] / w["culled_ms"]["median_ms"]
            r[form] = w
        call(2, False)
        s, tot = N.C.c_int64(), N.C.c_int64()
        N.check(L.surfd_isect_skipped(scene._handle, N.C.byref(s), N.C.byref(tot), N.stream()))
        r["skipped_tile_visits"], r["total_tile_visits"], r["skipped_share"] = s.value, tot.value, s.value / tot.value
        r["intersecting_pairs"] = int(count)
        r["intersecting_faces"] = int((hits > 0).sum())
        r["python_wrapper_ms"] = timed(lambda: scene.self_intersections(), a.reps)
        rows.append(r)
        print(json.dumps(r), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
