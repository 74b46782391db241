#!/usr/bin/env python3
"""Device-event timing of the fast winding numbers (surfd_winding_eval_fast, csrc/winding.hip) against the
exact path of the same library, after warm-up, median of repeated calls with events on one stream:

  the tori of 16 896 and 403 200 faces at Q = 4 096 unsorted uniform queries, and at the 32^3 and 64^3 voxel centres of [-1, 1]^3
  (x slowest: neighbouring lanes are neighbouring voxels), and 64^3 unsorted uniform queries for the comparison of the two orders;
  one marching-cubes shell (a sphere of radius 0.95 on a 512^3 grid, surfd_amd.mcubes.marching_cubes_device) at Q = 500 000
  unsorted uniform queries and at the 128^3 voxel centres.

Per row: the exact path's time (one call where it takes seconds), the fast path's at beta = 2 and 3, the ratio, the cluster and
triangle terms per query, and the maximum |w_fast - w_exact| over the row's queries against the exact GPU values.  Per mesh: the
time of surfd_winding_build_bvh (the hierarchy and its moments) on a fresh handle.

    python tools/winding_fast_time.py [--out profiles/winding_fast_time.json] [--reps 10] [--shell 512]

Per-kernel times: `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import raycast_ref as RR  # noqa: E402
from surfd_amd import mcubes  # noqa: E402
from surfd_amd.winding import WindingScene  # noqa: E402

BETAS = (2.0, 3.0)


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


def uniform(Q, seed=7):
    return (torch.rand(Q, 3, generator=torch.Generator().manual_seed(seed)) * 2 - 1).cuda()


def grid(R):
    c = -1.0 + (torch.arange(R, dtype=torch.float32, device="cuda") + 0.5) * (2.0 / R)
    return torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()


def shell(n, radius=0.95):
    """a sphere through marching cubes on an n^3 grid, scaled into [-1, 1]^3"""
    c = torch.linspace(-1, 1, n, device="cuda")
    z, y, x = torch.meshgrid(c, c, c, indexing="ij")
    vol = (x * x + y * y + z * z).sqrt_() - radius
    v, f = mcubes.marching_cubes_device(vol.contiguous(), 0.0)[:2]
    return (v * (2.0 / (n - 1)) - 1.0).contiguous(), f.long().contiguous()


def measure(name, vd, fd, queries, reps):
    F = int(fd.shape[0])
    build = timed(lambda: WindingScene(vd, fd)._build_bvh(), max(3, reps // 2), warm=1)
    create = timed(lambda: WindingScene(vd, fd), max(3, reps // 2), warm=1)
    scene = WindingScene(vd, fd, accel="bvh")
    out = {"mesh": name, "triangles": F, "levels": len(scene.read_bvh()["level_sizes"]), "create_ms": create,
           "create_and_build_bvh_ms": build, "build_bvh_ms_by_difference": build["median_ms"] - create["median_ms"], "rows": []}
    for kind, q in queries:
        Q = int(q.shape[0])
        heavy = F * Q >= 10 ** 12                                              # the exact path takes seconds: one call, no warm-up
        box = {}
        exact = timed(lambda: box.__setitem__("w", scene.winding_number(q, accel="exact")), 1 if heavy else reps, warm=0 if heavy else 1)
        row = {"queries": Q, "order": kind, "pairs": F * Q, "exact_ms": exact, "exact_pairs_per_s": F * Q / (exact["median_ms"] * 1e-3), "fast": []}
        for beta in BETAS:
            t = timed(lambda: scene.winding_number(q, beta=beta), reps)
            w = scene.winding_number(q, beta=beta, count_visits=True)
            ncl, ntri = scene.last_visits
            row["fast"].append({"beta": beta, "fast_ms": t, "exact_over_fast": exact["median_ms"] / t["median_ms"],
                                "cluster_terms_per_query": ncl / Q, "triangle_terms_per_query": ntri / Q,
                                "max_abs_error": float((w - box["w"]).abs().max()),
                                "occupancy_changes": int(((w.abs() >= 0.5) != (box["w"].abs() >= 0.5)).sum())})
        out["rows"].append(row)
        print(json.dumps({"mesh": name, "triangles": F, **row}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "winding_fast_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shell", type=int, default=512, help="the grid of the marching-cubes shell (0: leave it out)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "winding_fast_time.py measures on the GPU"
    meshes = []
    small = [("uniform, unsorted", uniform(4096)), ("grid 32^3", grid(32)), ("grid 64^3", grid(64)), ("uniform, unsorted", uniform(64 ** 3))]
    for name, (v, f) in (("torus 132 x 64", RR.torus(132, 64)), ("torus 480 x 420", RR.torus(480, 420))):
        meshes.append(measure(name, torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), small, a.reps))
    if a.shell:
        vd, fd = shell(a.shell)
        meshes.append(measure(f"marching-cubes sphere, {a.shell}^3", vd, fd, [("uniform, unsorted", uniform(500_000)), ("grid 128^3", grid(128))],
                              max(3, a.reps // 2)))
    out = {"device": torch.cuda.get_device_name(0), "betas": list(BETAS), "meshes": meshes}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
