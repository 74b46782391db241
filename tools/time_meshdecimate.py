#!/usr/bin/env python3
"""Times the edge-collapse decimation on the device (surfd_amd.meshsimplify.simplify_quadric_decimation, csrc/meshdecimate.hip)
beside vertex clustering at the same face count.  Inputs: the shells of tools/time_meshsimplify.py,

  shell(256)     marching_cubes_device on the sphere-shell field min(| |p| - 0.6 |, 0.1) at 256^3, level 0.01: 441 304 faces
  shell(456)     the same field at 456^3: about 1.4 million faces

each decimated to the face counts that simplify_vertex_clustering(cells=64) and (cells=128) give.  Before anything is timed the
device result is compared with tests/meshdecimate_ref.py for equal bits and order (vertices, faces, map, counts) on shell(--check),
a size the restatement can do, or the run stops.  Columns per entry: decimation's output sizes, rounds, stop reason and device time
as a consumer calls it (float64 vertices and int64 faces on the device; the narrowing of the faces and the call's host reads, two
per round, lie inside the bracket), median of --reps calls after --warmup, by events on the stream; clustering's time measured the
same way at the matched face count; both outputs' largest and mean distance from the analytic shell (the two spheres of radius
0.6 +- 0.01: || p | - 0.6 | - 0.01 |, in the field's units, the cube [-1, 1]^3); ``roof_ms``, the time to stream the call's input and output bytes once (24 V + 12 F in,
24 V' + 12 F' out) at 8 TB/s.  No ratio is fixed beforehand and none is asserted; entries at which decimation is the slower of the
two are listed under "decimation_slower_than_clustering", a call that stalled above its target under "stalled".

The measurement runs in one child process under a time limit; the parent only waits and reports.

    python tools/time_meshdecimate.py [--out profiles/meshdecimate_time.json] [--reps 20] [--warmup 3] [--shells 256 456] [--check 96] [--limit 900]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROOF_BYTES_PER_MS = 8e12 / 1e3


def shell_distance(p, n):
    p = p * (2.0 / (n - 1)) - 1.0                              # the meshes are in voxel-index units
    r = (p * p).sum(dim=1).sqrt()
    d = ((r - 0.6).abs() - 0.01).abs()
    return {"max": float(d.max()), "mean": float(d.mean())} if len(d) else {"max": None, "mean": None}


def check(n):
    import numpy as np
    import torch
    import meshdecimate_ref as R
    from surfd_amd.meshsimplify import DECIMATE_STOPS, simplify_quadric_decimation
    from time_meshclean import shell
    v, f = shell(n)
    target = len(f) // 8
    wv, wf, wm, wc = R.decimate(v, f, target)
    gv, gf, gm, gc = simplify_quadric_decimation(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), target, return_map=True, return_stats=True)
    gc["stop"] = DECIMATE_STOPS.index(gc["stop"])
    equal = (gc == wc and np.array_equal(gv.cpu().numpy().view(np.int64), wv.view(np.int64)) and np.array_equal(gf.cpu().numpy(), wf)
             and np.array_equal(gm.cpu().numpy(), wm))
    assert equal, f"shell({n}) to {target} faces: the device differs from the restatement ({gc} / {wc})"
    return {"mesh": f"shell({n})", "faces": len(f), "target": target, "counts": wc, "equal_to_restatement": True}


def measure(n, v, f, cells, a):
    name = f"shell({n})"
    import torch
    from surfd_amd.meshsimplify import simplify_quadric_decimation, simplify_vertex_clustering
    from time_meshclean import timed
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    kv, kf, kc = simplify_vertex_clustering(vd, fd, cells=cells, return_stats=True)
    target = len(kf)
    dv, df, dc = simplify_quadric_decimation(vd, fd, target, return_stats=True)
    nbytes = 24 * len(v) + 12 * len(f) + 24 * len(dv) + 12 * len(df)
    dec = timed(lambda: simplify_quadric_decimation(vd, fd, target), a.reps, a.warmup)
    clu = timed(lambda: simplify_vertex_clustering(vd, fd, cells=cells), a.reps, a.warmup)
    return {"mesh": name, "faces": len(f), "vertices": len(v), "target_faces": target, "matched_cells": cells, "decimation_counts": dc,
            "decimation_ms": dec, "clustering_ms": clu, "clustering_counts": kc, "decimation_distance": shell_distance(dv, n), "clustering_distance": shell_distance(kv, n),
            "bytes": nbytes, "roof_ms": nbytes / ROOF_BYTES_PER_MS, "decimation_over_roof": dec["median_ms"] / (nbytes / ROOF_BYTES_PER_MS),
            "decimation_over_clustering": dec["median_ms"] / clu["median_ms"], "ms_per_round": dec["median_ms"] / max(dc["rounds"], 1)}


def child(a):
    import torch
    from time_meshclean import shell
    assert torch.cuda.is_available(), "time_meshdecimate.py measures on the GPU"
    checked = check(a.check)
    print(json.dumps(checked), flush=True)
    rows = []
    for n in a.shells:
        v, f = shell(n)
        for cells in a.cells:
            rows.append(measure(n, v, f, cells, a))
            print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/time_meshdecimate.py", "device": torch.cuda.get_device_name(0),
           "what": f"decimation_ms / clustering_ms: medians of {a.reps} calls of simplify_quadric_decimation(target_faces) / simplify_vertex_clustering(cells=K) "
                   f"after {a.warmup} warm-up calls, by events on the stream (host reads included), target_faces being clustering's face count; distances: "
                   "of the output vertices from the two spheres of radius 0.6 +- 0.01; roof_ms: decimation's input and output bytes streamed once at 8 TB/s",
           "checked_first": checked, "rows": rows,
           "decimation_slower_than_clustering": [f"{r['mesh']} to {r['target_faces']}" for r in rows if r["decimation_over_clustering"] > 1.0],
           "stalled": [f"{r['mesh']} to {r['target_faces']}: {r['decimation_counts']['faces']} faces" for r in rows if r["decimation_counts"]["stop"] != "target"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshdecimate_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shells", type=int, nargs="*", default=[256, 456])
    ap.add_argument("--cells", type=int, nargs="*", default=[64, 128])
    ap.add_argument("--check", type=int, default=96, help="the shell on which the device is compared with the restatement first")
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", a.out, "--reps", str(a.reps), "--warmup", str(a.warmup), "--check", str(a.check),
           "--shells"] + [str(x) for x in a.shells] + ["--cells"] + [str(x) for x in a.cells]
    try:
        r = subprocess.run(cmd, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the measurement did not finish within {a.limit} s")
    raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
