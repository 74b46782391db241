#!/usr/bin/env python3
"""Times the mesh cleaning on the device (surfd_amd.meshclean, csrc/meshclean.hip) against the path it replaces: meshproc.
clean_until_stable on one core of the same box, with the two copies a mesh that lives on the device needs (vertices and faces to
the host, the result back).  Inputs:

  sheet(n)       an n x n sheet of quads with a seeded 5 % of its faces removed (tests/meshclean_ref.sheet): thousands of
                 one- and two-triangle holes that get capped, so every step of the sequence and a second pass run;
                 n = 500 (about 475 000 faces) and two smaller sizes, so that a crossover shows if there is one
  shell(256)     marching_cubes_device on the sphere-shell field min(| |p| - 0.6 |, 0.1) at 256^3, level 0.01 (the field of
                 tools/time_mcdevice.py): a closed mesh, the fast return of clean_until_stable

Before anything is timed the device result is compared with meshproc's at every size: equal bits and order, or the run stops.
Every figure is the median of --reps calls after --warmup calls, by events on the stream for the device (the host reads of a
call lie inside the bracket) and by wall clock for the host.  Per step (on meshproc's own intermediate meshes): the device time,
the bytes the step must stream once (`bytes`: its inputs read once, its outputs written once) and `x_stream`, its time over the
time to move those bytes at the bandwidth a device-to-device copy reaches here.  No ratio is fixed beforehand and none is
asserted; inputs at which the host path is faster are listed under "host_wins".

The measurement runs in one child process under a time limit; the parent only waits and reports.

    python tools/time_meshclean.py [--out profiles/meshclean_time.json] [--reps 20] [--warmup 3] [--sheets 64 128 500] [--shell 256] [--limit 900]
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


def stats(times):
    times = sorted(times)
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": len(times)}


def timed(fn, reps, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return stats(times)


def host_timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); times.append((time.perf_counter() - t) * 1e3)
    return stats(times)


def copy_bandwidth():
    """bytes per millisecond moved by a device-to-device copy of 256 MiB (read + write)"""
    import torch
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src), 10, 2)
    return 2 * src.numel() / t["median_ms"], t


def shell(n):
    import torch
    from surfd_amd import mcubes
    ax = torch.linspace(-1.0, 1.0, n, device="cuda", dtype=torch.float32)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    udf = torch.clamp((torch.sqrt(x * x + y * y + z * z) - 0.6).abs(), max=0.1).contiguous()
    v, f = mcubes.marching_cubes_device(udf, 0.01, classic=True)
    return v.double().cpu().numpy(), f.long().cpu().numpy()


def measure(name, v, f, reps, warm, bytes_per_ms):
    import numpy as np
    import torch
    from surfd_amd import meshclean as MC, meshproc as mp
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    # meshproc's own chain: the reference of every comparison and the inputs of the per-step timings
    v1, f0 = mp.cull_and_merge(v, f)
    fdup = mp.drop_duplicate_faces(f0)
    fdeg = mp.drop_degenerate_faces(v1, fdup)
    fcap = mp.fill_small_holes(v1, fdeg)
    cv, cf = mp.clean_until_stable(v, f)
    gv, gf, st = MC.clean_until_stable(vd, fd, return_stats=True)

    def same(got, want):
        got = got.cpu().numpy()
        return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.int64), want.view(np.int64))
    v1d, f0d, fdupd, fdegd = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (v1, f0, fdup, fdeg))
    checks = {"clean_until_stable": same(gv, cv) and same(gf, cf), "cull_and_merge": all(same(g, w) for g, w in zip(MC.cull_and_merge(vd, fd), (v1, f0))),
              "drop_duplicate_faces": same(MC.drop_duplicate_faces(f0d), fdup), "drop_degenerate_faces": same(MC.drop_degenerate_faces(v1d, fdupd), fdeg),
              "fill_small_holes": same(MC.fill_small_holes(v1d, fdegd), fcap)}
    assert all(checks.values()), f"{name}: the device differs from meshproc: {checks}"
    row = {"mesh": name, "faces": len(f), "vertices": len(v), "faces_out": len(cf), "vertices_out": len(cv), "stats": st, "equal_to_meshproc": sorted(checks)}

    # the steps on int32 faces, as clean_until_stable chains them (no widening to int64 in between)
    f32 = {k: t.to(torch.int32) for k, t in (("f", fd), ("f0", f0d), ("fdup", fdupd), ("fdeg", fdegd))}
    V, F, V1, F0, F1, F2 = len(v), len(f), len(v1), len(f0), len(fdup), len(fdeg)
    steps = {"cull_and_merge": (lambda: MC._cull(vd, f32["f"], 1e-8), 24 * V + 12 * F + 24 * V1 + 12 * F0),
             "drop_duplicate_faces": (lambda: MC._dedup(f32["f0"]), 12 * F0 + 12 * F1),
             "drop_degenerate_faces": (lambda: MC._degen(v1d, f32["fdup"], 1e-8), 24 * V1 + 12 * F1 + 12 * F2),
             "fill_small_holes": (lambda: MC._fill(v1d, f32["fdeg"]), 12 * F2 + 12 * (len(fcap) - F2))}
    row["steps"] = {}
    for k, (fn, nbytes) in steps.items():
        t = timed(fn, reps, warm)
        row["steps"][k] = dict(t, bytes=nbytes, stream_ms=nbytes / bytes_per_ms, x_stream=t["median_ms"] / (nbytes / bytes_per_ms))
    row["device_clean_until_stable_ms"] = timed(lambda: MC.clean_until_stable(vd, fd), reps, warm)

    def host():
        hv, hf = vd.cpu().numpy(), fd.cpu().numpy()
        ov, of = mp.clean_until_stable(hv, hf)
        out = torch.from_numpy(ov).cuda(), torch.from_numpy(of).cuda()
        torch.cuda.synchronize()
        return out
    row["host_clean_until_stable_with_copies_ms"] = host_timed(host, reps if len(f) < 100_000 else max(3, reps // 4), 1)
    row["host_clean_until_stable_alone_ms"] = host_timed(lambda: mp.clean_until_stable(v, f), 3, 0)
    row["host_over_device"] = row["host_clean_until_stable_with_copies_ms"]["median_ms"] / row["device_clean_until_stable_ms"]["median_ms"]
    return row


def child(a):
    import torch
    import meshclean_ref as R
    assert torch.cuda.is_available(), "time_meshclean.py measures on the GPU"
    torch.set_num_threads(1)                                  # the host path on one core
    bytes_per_ms, copy = copy_bandwidth()
    rows = []
    for n in a.sheets:
        rows.append(measure(f"sheet({n})", *R.sheet(n), a.reps, a.warmup, bytes_per_ms))
        print(json.dumps(rows[-1]), flush=True)
    if a.shell:
        rows.append(measure(f"shell({a.shell})", *shell(a.shell), a.reps, a.warmup, bytes_per_ms))
        print(json.dumps(rows[-1]), flush=True)
    out = {"tool": "tools/time_meshclean.py", "device": torch.cuda.get_device_name(0),
           "what": f"medians of {a.reps} calls after {a.warmup} warm-up calls; device rows by events on the stream (host reads included), host rows by wall "
                   "clock on one core with the copies of a device mesh; x_stream = a step's time over the time to stream its bytes once at the "
                   "bandwidth of a device-to-device copy",
           "copy_256MiB": copy, "copy_GB_per_s": bytes_per_ms / 1e6, "rows": rows,
           "host_wins": [r["mesh"] for r in rows if r["host_over_device"] < 1.0]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshclean_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sheets", type=int, nargs="*", default=[64, 128, 500])
    ap.add_argument("--shell", type=int, default=256, help="0: skip the marching-cubes mesh")
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", a.out, "--reps", str(a.reps), "--warmup", str(a.warmup), "--shell", str(a.shell),
           "--sheets"] + [str(x) for x in a.sheets]
    try:
        r = subprocess.run(cmd, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the measurement did not finish within {a.limit} s")
    raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
