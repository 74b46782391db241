#!/usr/bin/env python3
"""Times the level-set mesher of the watertight path on the sphere-shell field min(| |p| - 0.6 |, 0.1) over [-1, 1]^3 at level
0.01, classic table:

  (a) host_path_ms      today's path: udf.cpu().numpy() (pageable) + mcubes.marching_cubes on one core (host clock; ends in the copy's sync)
  (b) device_path_ms    mcubes.marching_cubes_device, its one host read included (events on the stream)
  (c) classify_ms       the classify pass alone (events), next to the time to stream the volume once at the HBM peak and at the
                        achievable rate of MI355X_MICROARCH.md

Median of --runs timed runs after --warmup warm-up runs, per size.  Every size runs in a child process of its own under a time
limit; the first failure ends the run.  Before anything is timed the device mesh is compared with the host mesh (all bits).
Writes one JSON document (default profiles/mcdevice_time.json) with V, F and the active cubes of every size.

    python tools/time_mcdevice.py [--sizes 128 256 512] [--runs 20] [--warmup 3] [--out profiles/mcdevice_time.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_TBS, HBM_ACHIEVABLE_TBS = 8.0, 6.3            # MI355X_MICROARCH.md: spec; measured float4 copy


def measure(n: int, runs: int, warmup: int) -> dict:
    import numpy as np
    import torch

    from surfd_amd import mcubes
    if not torch.cuda.is_available():
        raise SystemExit("time_mcdevice: no GPU (a timing from anywhere else says nothing)")
    ax = torch.linspace(-1.0, 1.0, n, device="cuda", dtype=torch.float32)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    udf = torch.clamp((torch.sqrt(x * x + y * y + z * z) - 0.6).abs(), max=0.1).contiguous()
    del x, y, z
    level = 0.01

    hv, hf = mcubes.marching_cubes(udf.cpu().numpy(), level, classic=True)
    dv, df = mcubes.marching_cubes_device(udf, level, classic=True)
    same = bool(np.array_equal(dv.cpu().numpy().view(np.uint32), hv.astype(np.float32).view(np.uint32)) and np.array_equal(df.cpu().numpy(), hf))
    if not same:
        raise SystemExit(f"time_mcdevice: the device mesh differs from the host mesh at {n}^3")
    mesher = mcubes._last_mesher[1]
    active = mesher.active_cubes

    def events(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    def host_path():
        return mcubes.marching_cubes(udf.cpu().numpy(), level, classic=True)

    for _ in range(min(warmup, 2)):
        host_path()
    host_ms, copy_ms = [], []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        u = udf.cpu().numpy()
        t1 = time.perf_counter()
        mcubes.marching_cubes(u, level, classic=True)
        t2 = time.perf_counter()
        host_ms.append((t2 - t0) * 1e3)
        copy_ms.append((t1 - t0) * 1e3)
    dev_ms = events(lambda: mcubes.marching_cubes_device(udf, level, classic=True))
    full_ms = events(lambda: mcubes.marching_cubes_device(udf, level, classic=True, return_normals=True, return_values=True))
    cls_ms = events(lambda: mesher.classify_only(udf, level, True))
    nbytes = 4 * n ** 3
    med = statistics.median
    return {"n": n, "level": level, "classic": True, "vertices": int(len(hv)), "faces": int(len(hf)), "active_cubes": int(active),
            "bits_equal_host": same, "runs": runs, "warmup": warmup,
            "host_path_ms": med(host_ms), "host_path_copy_ms": med(copy_ms), "host_path_ms_min_max": [min(host_ms), max(host_ms)],
            "device_path_ms": med(dev_ms), "device_path_ms_min_max": [min(dev_ms), max(dev_ms)],
            "device_path_with_normals_values_ms": med(full_ms),
            "classify_ms": med(cls_ms), "classify_ms_min_max": [min(cls_ms), max(cls_ms)],
            "volume_bytes": nbytes, "stream_once_at_hbm_peak_ms": nbytes / (HBM_PEAK_TBS * 1e12) * 1e3,
            "stream_once_at_hbm_achievable_ms": nbytes / (HBM_ACHIEVABLE_TBS * 1e12) * 1e3,
            "classify_over_hbm_peak": med(cls_ms) / (nbytes / (HBM_PEAK_TBS * 1e12) * 1e3),
            "host_over_device": med(host_ms) / med(dev_ms)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcdevice_time.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    if a.child:
        print(json.dumps(measure(a.child, a.runs, a.warmup)))
        return 0
    results = []
    for n in a.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--runs", str(a.runs), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"time_mcdevice: {n}^3 did not finish within {a.limit} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"time_mcdevice: {n}^3 failed with status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    doc = {"tool": "tools/time_mcdevice.py", "field": "min(| |p| - 0.6 |, 0.1) on [-1, 1]^3", "statistic": f"median of {a.runs} runs after {a.warmup} warm-up runs",
           "hbm_tb_per_s": {"peak": HBM_PEAK_TBS, "achievable": HBM_ACHIEVABLE_TBS}, "sizes": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
