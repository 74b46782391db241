#!/usr/bin/env python3
"""Times the hole filling on the device (surfd_amd.meshfill, csrc/meshfill.hip): the plan (border pass, loop discovery, binning)
and the run (triangulation, caps) separately, beside the stage it extends and its own restatement.  Inputs:

  sheet(500)     the 500 x 500 sheet of quads with a seeded 5 % of its faces removed that tools/time_meshclean.py uses
                 (tests/meshclean_ref.sheet, about 475 000 faces), at max_edges 32, 128 and 1024
  ring(n)        one loop of n = 32, 128, 512 and 1024 edges (tests/meshfill_ref.ring): the three classes of the kernel alone

Before anything is timed the device result is compared with the restatement tests/meshfill_ref.py (faces, cap_loop and counts:
equal bits and order, or the run stops), except ring(1024), where only the counts are looked at.  Every device figure is the
median of --reps calls after --warmup calls, by events on the stream (the host reads of a call lie inside the bracket).  Beside
each: meshclean.fill_small_holes on the same mesh, the stage this one extends, from the same library; and the restatement on one
core by wall clock, once: a RESTATEMENT written to be read, not a tuned host library.  `gtri_per_s` is the rate of the run against
the n (n - 1) (n - 2) / 6 triangle evaluations of its loops' tables.  No figure is fixed beforehand and none is asserted.

The measurement runs in one child process under a time limit; the parent only waits and reports.

    python tools/time_meshfill.py [--out profiles/meshfill_time.json] [--reps 20] [--warmup 3] [--sheet 500] [--rings 32 128 512 1024] [--limit 900]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_meshclean import timed  # noqa: E402


def measure(name, v, f, max_edges, reps, warm, compare=True):
    import numpy as np
    import torch
    import meshfill_ref as R
    from surfd_amd import meshclean as MC, meshfill as MF
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    gf, gl, st = MF.fill_holes(vd, fd, max_edges=max_edges, return_cap_loop=True, return_stats=True)
    row = {"mesh": name, "max_edges": max_edges, "faces": len(f), "vertices": len(v), "counts": st}
    if compare:
        t = time.perf_counter()
        wf, wl, ws = R.fill_holes(v, f, max_edges)
        row["restatement_one_core_ms"] = (time.perf_counter() - t) * 1e3
        assert st == ws and np.array_equal(gf.cpu().numpy(), wf) and np.array_equal(gl.cpu().numpy(), wl), f"{name}: the device differs from the restatement"
        row["equal_to_restatement"] = True
    plan = MF._Fill(vd, fd, max_edges)
    sizes = plan.sizes().tolist()
    row["triangle_evaluations"] = sum(n * (n - 1) * (n - 2) // 6 for n in sizes if n <= max_edges)
    row["plan_ms"] = timed(lambda: MF._Fill(vd, fd, max_edges), reps, warm)
    row["run_ms"] = timed(plan.run, reps, warm)
    row["fill_holes_ms"] = timed(lambda: MF.fill_holes(vd, fd, max_edges=max_edges), reps, warm)
    row["gtri_per_s"] = row["triangle_evaluations"] / row["run_ms"]["median_ms"] / 1e6
    row["fill_small_holes_ms"] = timed(lambda: MC.fill_small_holes(vd, fd), reps, warm)
    return row


def child(a):
    import torch
    import meshclean_ref
    import meshfill_ref as R
    assert torch.cuda.is_available(), "time_meshfill.py measures on the GPU"
    torch.set_num_threads(1)                                  # the restatement on one core
    rows = []

    def add(*args, **kw):
        rows.append(measure(*args, **kw))
        print(json.dumps(rows[-1]), flush=True)
    if a.sheet:
        v, f = meshclean_ref.sheet(a.sheet)
        for m in (32, 128, 1024):
            add(f"sheet({a.sheet})", v, f, m, a.reps, a.warmup)
    for n in a.rings:
        v, f = R.ring(n, seed=n)
        add(f"ring({n})", v, f, 1024, a.reps, a.warmup, compare=n <= 512)
    out = {"tool": "tools/time_meshfill.py", "device": torch.cuda.get_device_name(0),
           "what": f"medians of {a.reps} calls after {a.warmup} warm-up calls by events on the stream (host reads included): plan and run of one "
                   "handle separately, fill_holes as a caller sees it (plan + run + the concatenation), fill_small_holes on the same mesh; the "
                   "restatement tests/meshfill_ref.py on one core, once, by wall clock (a restatement, not a tuned host library); gtri_per_s = "
                   "the triangle evaluations of the filled loops' tables, n (n - 1) (n - 2) / 6 each, over the run's time",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshfill_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sheet", type=int, default=500, help="0: skip the sheet")
    ap.add_argument("--rings", type=int, nargs="*", default=[32, 128, 512, 1024])
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", a.out, "--reps", str(a.reps), "--warmup", str(a.warmup), "--sheet", str(a.sheet),
           "--rings"] + [str(x) for x in a.rings]
    try:
        r = subprocess.run(cmd, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the measurement did not finish within {a.limit} s")
    raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
