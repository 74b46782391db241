#!/usr/bin/env python3
"""Device-event timing of the mesh smoothing and the vertex normals (surfd_amd.meshsmooth, csrc/meshsmooth.hip) after warm-up, on
noisy icospheres of 20 480, 81 920, 327 680 and 1 310 720 faces, each with one open 200 x 200 sheet appended so that the border
paths have work: the build, one sweep of every kind (Laplacian with cotangent and with uniform weights; the umbrella over all
half-edges and over the border), the three calls at
their defaults (laplacian 3 steps, smooth_borders 20 iterations, taubin 10 steps) and both kinds of normals; each the median of
repeated calls with events on one stream.  Before anything is timed the device results are compared with the restatement
(tests/meshsmooth_ref.py): equal bits, or the run stops.

Next to them: meshproc's functions on the same mesh and the same box (wall clock), with the copies a mesh that lives on the
device would need (positions and faces to the host, positions back); and `roof_ms`, the time to stream 48 V + 12 F bytes (read
the positions once, write them once, read the faces once) at the bandwidth a device-to-device copy reaches here: how far a
sweep is from moving its data once.  No ratio is fixed beforehand and none is asserted; sizes at which the host is faster are
listed under "host_wins".

The measurement runs in one child process under a time limit; the parent only waits and reports.

    python tools/time_meshsmooth.py [--out profiles/meshsmooth_time.json] [--reps 10] [--levels 5 6 7 8] [--limit 900]
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


def timed(fn, reps, warm=2):
    import torch
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


def host_timed(fn, reps):
    times = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); times.append((time.perf_counter() - t) * 1e3)
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def copy_bandwidth():
    """bytes per millisecond moved by a device-to-device copy of 256 MiB (read + write)"""
    import torch
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src), 10)
    return 2 * src.numel() / t["median_ms"], t


def mesh(level):
    import numpy as np
    import meshsmooth_ref as R
    v, f = R.icosphere(level, noise=0.2 * 2.0 ** -level, seed=level)
    sv, sf = R.sheet(200, 0.1, seed=level, shuffle=False)
    sv = sv * (1.0 / 200) + np.array([2.0, 0.0, 0.0])
    return np.concatenate([v, sv]), np.concatenate([f, sf + len(v)])


def measure(level, reps, bytes_per_ms):
    import numpy as np
    import torch
    import meshsmooth_ref as R
    from surfd_amd import meshproc
    from surfd_amd.meshsmooth import MeshSmoother
    v, f = mesh(level)
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    s = MeshSmoother(fd, len(v))
    row = {"mesh": f"icosphere({level}) + sheet(200)", "faces": len(f), "vertices": len(v), "border_halfedges": s.num_border_halfedges,
           "border_vertices": s.num_border_vertices, "roof_ms": (48 * len(v) + 12 * len(f)) / bytes_per_ms}
    # equality with the restatement first
    assert (s.num_border_halfedges, s.num_border_vertices) == R.counts(f)
    lap = R.laplacian(v, f)
    checks = {"laplacian": (s.laplacian(vd), lap),
              "smooth_borders": (s.smooth_borders(vd), R.smooth_borders(v, f)), "taubin(2)": (s.taubin(vd, 2), R.taubin(v, f, 2)),
              "normals_area": (s.vertex_normals(vd, "area"), R.vertex_normals(v, f, "area")[0])}
    for k, (got, want) in checks.items():
        assert np.array_equal(got.cpu().numpy(), want), f"{k} differs from the restatement at level {level}"
    row["equal_to_restatement"] = sorted(checks)
    row["normals_angle_max_diff"] = float(np.abs(s.vertex_normals(vd, "angle").cpu().numpy() - R.vertex_normals(v, f, "angle")[0]).max())
    # the device
    row["build_ms"] = timed(lambda: MeshSmoother(fd, len(v)), reps)
    row["sweep_laplacian_cotangent_ms"] = timed(lambda: s.laplacian(vd, 1), reps)
    row["sweep_laplacian_uniform_ms"] = timed(lambda: s.laplacian(vd, 1, cotangent=False), reps)
    row["sweep_umbrella_all_ms"] = timed(lambda: s.umbrella(vd, 0.5), reps)
    row["sweep_umbrella_border_ms"] = timed(lambda: s.umbrella(vd, 0.3, neighbours="border"), reps)
    row["copy_positions_ms"] = timed(lambda: s.laplacian(vd, 0), reps)                     # what every call pays besides its sweeps
    row["laplacian_default_ms"] = timed(lambda: s.laplacian(vd), reps)
    row["smooth_borders_default_ms"] = timed(lambda: s.smooth_borders(vd), reps)
    row["taubin_default_ms"] = timed(lambda: s.taubin(vd), reps)
    row["normals_angle_ms"] = timed(lambda: s.vertex_normals(vd, "angle"), reps)
    row["normals_area_ms"] = timed(lambda: s.vertex_normals(vd, "area"), reps)
    # the host, with the copies a device mesh needs
    hreps = 3 if len(f) < 500_000 else 1

    def host(fn):
        def run():
            hv, hf = vd.cpu().numpy(), fd.cpu().numpy()
            out = torch.from_numpy(fn(hv, hf)).cuda()
            torch.cuda.synchronize()
            return out
        return run
    row["host_laplacian_smooth_ms"] = host_timed(host(lambda a, b: meshproc.laplacian_smooth(a, b, steps=3)), hreps)
    row["host_smooth_borders_ms"] = host_timed(host(meshproc.smooth_borders), hreps)
    row["host_vertex_normals_by_angle_ms"] = host_timed(host(meshproc.vertex_normals_by_angle), hreps)
    pairs = (("host_laplacian_smooth_ms", "laplacian_default_ms"), ("host_smooth_borders_ms", "smooth_borders_default_ms"),
             ("host_vertex_normals_by_angle_ms", "normals_angle_ms"))
    row["host_wins"] = [h for h, d in pairs if row[h]["median_ms"] < row[d]["median_ms"]]
    return row


def child(a):
    import torch
    assert torch.cuda.is_available(), "time_meshsmooth.py measures on the GPU"
    bytes_per_ms, copy = copy_bandwidth()
    rows = []
    for level in a.levels:
        rows.append(measure(level, a.reps, bytes_per_ms))
        print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0),
           "what": "medians of repeated calls after warm-up; device rows by events on the stream, host rows by wall clock with the copies of a device mesh; "
                   "roof_ms = (48 V + 12 F) bytes at the bandwidth of a device-to-device copy",
           "copy_256MiB": copy, "copy_GB_per_s": bytes_per_ms / 1e6, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshsmooth_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--levels", type=int, nargs="+", default=[5, 6, 7, 8])
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", a.out, "--reps", str(a.reps), "--levels"] + [str(x) for x in a.levels]
    try:
        r = subprocess.run(cmd, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the measurement did not finish within {a.limit} s")
    raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
