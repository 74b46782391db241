#!/usr/bin/env python3
"""Device-event timing of generalized winding numbers (surfd_amd.winding, csrc/winding.hip) after warm-up: surfd_winding_eval
on the 16 896-face torus of the tests and on the torus refined to 403 200 faces (the meshes of tools/meshintersect_time.py) for
Q = 4 096, 32^3 and 64^3 uniform queries (median of repeated calls, events on one stream) and the (query, triangle) pairs per
second; voxelize_winding at R = 64 on the first torus; and, asserted nowhere, the number the feature exists for: the IoU at
R = 64 of the holed sphere of tests/winding_ref.py against the closed one, through voxelize_winding and through voxelize_solid.

    python tools/winding_time.py [--out profiles/winding_time.json] [--reps 10]

Every triangle contributes to every query: there is no culled path to compare with.  Per-kernel times: `rocprofv3
--kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import raycast_ref as RR  # noqa: E402
import winding_ref as WR  # noqa: E402
from surfd_amd import _native as N  # noqa: E402
from surfd_amd import voxelize  # noqa: E402
from surfd_amd.winding import WindingScene  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
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
    ap.add_argument("--out", default=os.path.join("profiles", "winding_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--large", type=int, nargs=2, default=(480, 420), metavar=("NU", "NV"), help="the refined torus: 2 NU NV faces")
    ap.add_argument("--queries", type=int, nargs="+", default=[4096, 32 ** 3, 64 ** 3])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "winding_time.py measures on the GPU"
    L = N.lib()
    rows = []
    first = RR.torus(96, 88)
    for name, (v, f) in (("torus 96 x 88", first), (f"torus {a.large[0]} x {a.large[1]}", RR.torus(*a.large))):
        vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        F = len(f)
        r = {"mesh": name, "triangles": F, "create_ms": timed(lambda: WindingScene(vd, fd), a.reps), "eval": []}
        scene = WindingScene(vd, fd)
        for Q in a.queries:
            q = (torch.rand(Q, 3, generator=torch.Generator().manual_seed(7)) * 2 - 1).cuda()
            w = torch.empty(Q, device="cuda", dtype=torch.float64)
            reps = a.reps if F * Q < 10 ** 10 else max(3, a.reps // 3)             # the largest calls take seconds
            t = timed(lambda: N.check(L.surfd_winding_eval(scene._handle, N.ptr(q), Q, 0, N.ptr(w), N.stream())), reps, warm=1)
            e = {"queries": Q, "pairs": F * Q, "eval_ms": t, "pairs_per_s": F * Q / (t["median_ms"] * 1e-3),
                 "inside_share": float((w.abs() >= 0.5).double().mean())}
            r["eval"].append(e)
            print(json.dumps({"mesh": name, **e}), flush=True)
        rows.append(r)
    vd, fd = torch.from_numpy(first[0]).cuda(), torch.from_numpy(first[1]).cuda()
    vox = {"mesh": "torus 96 x 88", "resolution": 64, "voxelize_winding_ms": timed(lambda: voxelize.voxelize_winding(vd, fd, 64), a.reps),
           "voxelize_solid_ms": timed(lambda: voxelize.voxelize_solid(vd, fd, 64), a.reps)}
    print(json.dumps(vox), flush=True)
    hv, hf, _ = WR.holed_sphere()
    cv, cf = RR.icosphere(3)
    hv, hf, cv, cf = (torch.from_numpy(x).cuda() for x in (hv, hf, cv, cf))
    solid_h, odd = voxelize.voxelize_solid(hv, hf, 64)
    iou = {"resolution": 64, "holed_faces": int(hf.shape[0]), "closed_faces": int(cf.shape[0]),
           "winding_holed_vs_winding_closed": float(voxelize.voxel_iou(voxelize.voxelize_winding(hv, hf, 64), voxelize.voxelize_winding(cv, cf, 64))),
           "solid_holed_vs_solid_closed": float(voxelize.voxel_iou(solid_h, voxelize.voxelize_solid(cv, cf, 64)[0])),
           "winding_closed_vs_solid_closed": float(voxelize.voxel_iou(voxelize.voxelize_winding(cv, cf, 64), voxelize.voxelize_solid(cv, cf, 64)[0])),
           "odd_columns_of_the_holed_sphere": int(odd)}
    print(json.dumps(iou), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "voxelize": vox, "holed_sphere_iou": iou}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
