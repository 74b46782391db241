#!/usr/bin/env python3
"""Times the mesh simplification on the device (surfd_amd.meshsimplify, csrc/meshsimplify.hip).  Inputs:

  shell(256)     marching_cubes_device on the sphere-shell field min(| |p| - 0.6 |, 0.1) at 256^3, level 0.01 (the field of
                 tools/time_mcdevice.py and tools/time_meshclean.py): 441 304 faces
  shell(456)     the same field at 456^3: about 1.4 million faces

at ``cells`` 64, 128 and 256 along the largest extent, for both representatives.  Before anything is timed the device mesh is
compared with tests/meshsimplify_ref.py at every setting: equal bits and order (vertices, faces, map, counts), or the run stops.
Columns per setting: the output sizes; the device time of simplify_vertex_clustering as a consumer calls it (float64 vertices and
int64 faces on the device; the narrowing of the faces, the read of the extent and the call's own host reads lie inside the
bracket), median of --reps calls after --warmup, by events on the stream; the numpy RESTATEMENT on one core of the same box, mesh
already on the host (median of --host_reps runs after one warm-up: it is the contract written for clarity, one rounding per numpy
operation, not a tuned host library, and no such library is installed to stand in for one); and ``roof_ms``, the time to stream
the call's input and output bytes once (24 V + 12 F in, 24 V' + 12 F' out) at 8 TB/s.  No ratio is fixed beforehand and none is
asserted; settings at which the restatement is faster are listed under "host_wins".

The measurement runs in one child process under a time limit; the parent only waits and reports.

    python tools/time_meshsimplify.py [--out profiles/meshsimplify_time.json] [--reps 20] [--warmup 3] [--host_reps 5] [--shells 256 456] [--limit 900]
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


def measure(name, v, f, cells, rep, a):
    import numpy as np
    import torch
    import meshsimplify_ref as R
    from surfd_amd.meshsimplify import simplify_vertex_clustering
    from time_meshclean import host_timed, timed
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    cell = float(torch.from_numpy(v).max(dim=0).values.sub(torch.from_numpy(v).min(dim=0).values).max()) / cells      # every vertex of a shell is referenced
    wv, wf, wm, wc = R.simplify(v, f, cell, representative=rep)
    gv, gf, gm, gc = simplify_vertex_clustering(vd, fd, cells=cells, representative=rep, return_map=True, return_stats=True)
    equal = (gc == wc and np.array_equal(gv.cpu().numpy().view(np.int64), wv.view(np.int64)) and np.array_equal(gf.cpu().numpy(), wf)
             and np.array_equal(gm.cpu().numpy(), wm))
    assert equal, f"{name} cells={cells} {rep}: the device differs from the restatement ({gc} / {wc})"
    nbytes = 24 * len(v) + 12 * len(f) + 24 * wc["vertices"] + 12 * wc["faces"]
    dev = timed(lambda: simplify_vertex_clustering(vd, fd, cells=cells, representative=rep), a.reps, a.warmup)
    host = host_timed(lambda: R.simplify(v, f, cell, representative=rep), a.host_reps, 1)
    return {"mesh": name, "faces": len(f), "vertices": len(v), "cells": cells, "cell": cell, "representative": rep, "counts": wc, "equal_to_restatement": True,
            "device_ms": dev, "restatement_one_core_ms": host, "bytes": nbytes, "roof_ms": nbytes / ROOF_BYTES_PER_MS,
            "device_over_roof": dev["median_ms"] / (nbytes / ROOF_BYTES_PER_MS), "restatement_over_device": host["median_ms"] / dev["median_ms"]}


def child(a):
    import torch
    from time_meshclean import shell
    assert torch.cuda.is_available(), "time_meshsimplify.py measures on the GPU"
    torch.set_num_threads(1)                                  # the restatement on one core
    rows = []
    for n in a.shells:
        v, f = shell(n)
        for cells in a.cells:
            for rep in ("mean", "quadric"):
                rows.append(measure(f"shell({n})", v, f, cells, rep, a))
                print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/time_meshsimplify.py", "device": torch.cuda.get_device_name(0),
           "what": f"device_ms: medians of {a.reps} calls of simplify_vertex_clustering(cells=K) after {a.warmup} warm-up calls, by events on the stream (host "
                   f"reads included); restatement_one_core_ms: tests/meshsimplify_ref.py (a numpy restatement written for clarity, not a tuned host library) "
                   f"on one core, medians of {a.host_reps} runs after 1 by wall clock, the mesh already on the host; roof_ms: the call's input and output "
                   "bytes streamed once at 8 TB/s",
           "rows": rows, "host_wins": [f"{r['mesh']} cells={r['cells']} {r['representative']}" for r in rows if r["restatement_over_device"] < 1.0]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshsimplify_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host_reps", type=int, default=5)
    ap.add_argument("--shells", type=int, nargs="*", default=[256, 456])
    ap.add_argument("--cells", type=int, nargs="*", default=[64, 128, 256])
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", a.out, "--reps", str(a.reps), "--warmup", str(a.warmup), "--host_reps", str(a.host_reps),
           "--shells"] + [str(x) for x in a.shells] + ["--cells"] + [str(x) for x in a.cells]
    try:
        r = subprocess.run(cmd, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the measurement did not finish within {a.limit} s")
    raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
