#!/usr/bin/env python3
"""Times the voxeliser (surfd_amd/voxelize.py, csrc/voxel.hip) on a closed ~220 000-vertex mesh (a torus of 470 x 470 vertices,
441 800 triangles) at R = 64 and R = 256:

  calls     every public call with device events (median of --repeats runs after a warm-up)
  kernels   the split of those calls into the vx_* kernels: the tool starts itself once per resolution under
            `rocprofv3 --kernel-trace --stats` (a child process; `--workload R` runs each call --trace-calls times) and reads the
            average duration of every vx_* kernel from the kernel statistics
  torch     a chunked pure-torch restatement of the surface rule (13-axis test over every triangle's box), of the solid rule
            (edge functions, top-left rule, first k by floor division, parity by a difference array) and of the point and IoU
            stages, on the same GPU and inputs; its grids must equal the library's

    python tools/voxelize_time.py --output profiles/voxelize_time.json
The restatements live only in this tool.  Not measured: the share of the atomics against the box loops inside a kernel."""
import argparse
import csv
import glob
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RESOLUTIONS = (64, 256)
LO, HI = -1.0, 1.0


def torus(n=470, R0=0.6, r0=0.25, device="cuda"):
    a = torch.arange(n, dtype=torch.float64) * (2 * math.pi / n)
    u, v = torch.meshgrid(a, a, indexing="ij")
    p = torch.stack([(R0 + r0 * torch.cos(v)) * torch.cos(u), (R0 + r0 * torch.cos(v)) * torch.sin(u), r0 * torch.sin(v)], -1).reshape(-1, 3)
    i = torch.arange(n)
    a00 = (i[:, None] * n + i[None]).reshape(-1)
    a10 = (((i + 1) % n)[:, None] * n + i[None]).reshape(-1)
    a01 = (i[:, None] * n + ((i + 1) % n)[None]).reshape(-1)
    a11 = (((i + 1) % n)[:, None] * n + ((i + 1) % n)[None]).reshape(-1)
    f = torch.cat([torch.stack([a00, a10, a11], 1), torch.stack([a00, a11, a01], 1)])
    return p.float().to(device).contiguous(), f.int().to(device).contiguous()


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


# ---- the torch restatement ----------------------------------------------------------------------------------------------------------
def t_snap(x, R):
    s = torch.tensor(256.0 * R / (HI - LO), dtype=torch.float32, device=x.device)
    r = torch.round((x - LO) * s)
    return r.long(), r.abs() <= 2 ** 19


def t_triangles(v, f, R):
    q, ok = t_snap(v, R)
    f = f.long()
    return q[f], ok[f].all(-1).all(-1)                         # [F, 3, 3] int64, [F]


def _offsets(ext, device):
    g = torch.meshgrid(*(torch.arange(int(e), device=device) for e in ext), indexing="ij")
    return torch.stack([x.reshape(-1) for x in g], -1)         # [n, len(ext)]


def t_surface(v, f, R, chunk=1 << 14):
    tri, ok = t_triangles(v, f, R)
    dense = torch.zeros(R, R, R, dtype=torch.bool, device=v.device)
    for s in range(0, len(tri), chunk):
        q = tri[s:s + chunk]
        e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
        n = torch.cross(e1, e2, dim=-1)
        lo = ((q.amin(1) - 1) >> 8).clamp(min=0)
        hi = (q.amax(1) >> 8).clamp(max=R - 1)
        keep = ok[s:s + chunk] & (n != 0).any(-1) & (lo <= hi).all(-1)
        q, n, lo, hi = q[keep], n[keep], lo[keep], hi[keep]
        if not len(q):
            continue
        idx = lo[:, None, :] + _offsets((hi - lo).amax(0) + 1, v.device)[None]                # [T, n, 3]
        inbox = (idx <= hi[:, None, :]).all(-1)
        w = q[:, :, None, :] - (256 * idx + 128)[:, None]                                     # [T, 3, n, 3]
        hit = inbox & ~((w.amin(1) > 128) | (w.amax(1) < -128)).any(-1)
        d = (n[:, None, :] * w[:, 0]).sum(-1)
        r = 128 * n.abs().sum(-1)[:, None]
        hit &= ~((d > r) | (d < -r))
        for e in range(3):
            u, o = w[:, e], w[:, (e + 2) % 3]
            ed = q[:, (e + 1) % 3] - q[:, e]
            for b, c in ((1, 2), (2, 0), (0, 1)):
                eb, ec = ed[:, b, None], ed[:, c, None]
                pu, po = eb * u[..., c] - ec * u[..., b], eb * o[..., c] - ec * o[..., b]
                rr = 128 * (eb.abs() + ec.abs())
                hit &= ~((torch.minimum(pu, po) > rr) | (torch.maximum(pu, po) < -rr))
        h = idx[hit]
        dense[h[:, 0], h[:, 1], h[:, 2]] = True
    return dense


def t_solid_fill(v, f, R, chunk=1 << 15):
    """-> (fill bool [R, R, R], odd columns)"""
    tri, ok = t_triangles(v, f, R)
    diff = torch.zeros(R * R * (R + 1), dtype=torch.int32, device=v.device)
    par = torch.zeros(R * R, dtype=torch.int32, device=v.device)

    def edge(p, q, sx, sy):
        return (q[:, None, 0] - p[:, None, 0]) * (sy - p[:, None, 1]) - (q[:, None, 1] - p[:, None, 1]) * (sx - p[:, None, 0])

    def top_left(p, q):
        dx, dy = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1]
        return (((dy == 0) & (dx > 0)) | (dy < 0))[:, None]

    for s in range(0, len(tri), chunk):
        q = tri[s:s + chunk]
        a2 = (q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0])
        lo = ((q[:, :, :2].amin(1) - 128 + 255) >> 8).clamp(min=0)
        hi = ((q[:, :, :2].amax(1) - 128) >> 8).clamp(max=R - 1)
        keep = ok[s:s + chunk] & (a2 != 0) & (lo <= hi).all(-1)
        q, a2, lo, hi = q[keep], a2[keep], lo[keep], hi[keep]
        if not len(q):
            continue
        sw = (a2 < 0)[:, None]
        A, B, C = q[:, 0], torch.where(sw, q[:, 2], q[:, 1]), torch.where(sw, q[:, 1], q[:, 2])
        a2 = a2.abs()[:, None]
        idx = lo[:, None, :] + _offsets((hi - lo).amax(0) + 1, v.device)[None]                # [T, n, 2]
        sx, sy = 256 * idx[..., 0] + 128, 256 * idx[..., 1] + 128
        e0, e1, e2 = edge(B, C, sx, sy), edge(C, A, sx, sy), edge(A, B, sx, sy)
        cov = (idx <= hi[:, None, :]).all(-1)
        for e, tl in ((e0, top_left(B, C)), (e1, top_left(C, A)), (e2, top_left(A, B))):
            cov &= (e > 0) | ((e == 0) & tl)
        S = e0 * A[:, None, 2] + e1 * B[:, None, 2] + e2 * C[:, None, 2]
        k = (torch.div(S - 128 * a2, 256 * a2, rounding_mode="floor") + 1).clamp(0, R)        # the first k with (256 k + 128) a2 > S
        col = (idx[..., 0] * R + idx[..., 1])[cov]
        one = torch.ones_like(col, dtype=torch.int32)
        diff.index_put_((col * (R + 1) + k[cov],), one, accumulate=True)
        par.index_put_((col,), one, accumulate=True)
    fill = (diff.reshape(R, R, R + 1).cumsum(-1)[..., :R] & 1).bool()
    return fill, int((par & 1).sum())


def t_points(p, R):
    q, ok = t_snap(p, R)
    v = torch.where(q == 256 * R, R - 1, q >> 8)
    ok = ok.all(1) & ((v >= 0) & (v < R)).all(1)
    d = torch.zeros(R, R, R, dtype=torch.bool, device=p.device)
    v = v[ok]
    d[v[:, 0], v[:, 1], v[:, 2]] = True
    return d


# ---- the three parts ----------------------------------------------------------------------------------------------------------------
def workload(R, calls):
    """what the kernel trace sees: every public call `calls` times at one resolution"""
    from surfd_amd import voxelize as VZ
    v, f = torus()
    for _ in range(calls):
        VZ.voxelize_surface(v, f, R)
        ga, _ = VZ.voxelize_solid(v, f, R, include_surface=False)
        VZ.voxelize_points(v, R)
        VZ.voxel_iou(ga, ga)
    torch.cuda.synchronize()


def kernel_split(R, calls):
    """average duration of every vx_* kernel over `calls` calls, from a child process under the kernel trace"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as td:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "kt", "--",
               sys.executable, os.path.abspath(__file__), "--workload", str(R), "--trace-calls", str(calls)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        stats = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not stats:
            return {"error": f"kernel trace failed (exit {r.returncode}): {r.stderr[-300:]}"}
        out = {}
        for row in csv.DictReader(open(stats[0])):
            if "surfd::vx_" in row["Name"]:
                name = row["Name"].split("surfd::")[1].split("(")[0]
                out[name] = {"launches": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
        return out


def measure(a):
    from surfd_amd import voxelize as VZ
    split = {str(R): kernel_split(R, a.trace_calls) for R in RESOLUTIONS}       # children first: this process has not opened the GPU yet
    v, f = torus()
    out = {"device": torch.cuda.get_device_name(0), "vertices": len(v), "triangles": len(f), "repeats": a.repeats,
           "bounds": [LO, HI], "resolutions": {}}
    for R in RESOLUTIONS:
        r = {"kernels_average_us": split[str(R)]}
        for path in (None, "large"):
            r[f"surface_{path or 'default'}_ms"] = timed(lambda: VZ.voxelize_surface(v, f, R, path=path), a.repeats)
        r["solid_fill_only_ms"] = timed(lambda: VZ.voxelize_solid(v, f, R, include_surface=False), a.repeats)
        r["solid_with_surface_ms"] = timed(lambda: VZ.voxelize_solid(v, f, R), a.repeats)
        r["points_ms"] = timed(lambda: VZ.voxelize_points(v, R), a.repeats)
        gs = VZ.voxelize_surface(v, f, R)
        gf, odd = VZ.voxelize_solid(v, f, R, include_surface=False)
        gb, _ = VZ.voxelize_solid(v + 0.05, f, R)
        r["odd_columns"], r["surface_voxels"], r["filled_voxels"] = odd, gs.count(), gf.count()
        r["iou_paired_ms"] = timed(lambda: VZ.voxel_iou(gf, gb), a.repeats)
        iou, inter, union = VZ.voxel_iou(gf, gb, return_counts=True)
        r["iou_of_the_fill_with_a_copy_shifted_by_0.05"] = float(iou)
        reps = max(3, a.repeats // 4)
        r["torch_surface_ms"] = timed(lambda: t_surface(v, f, R), reps)
        r["torch_surface_same_grid"] = bool(torch.equal(t_surface(v, f, R), gs.dense()))
        r["torch_solid_fill_ms"] = timed(lambda: t_solid_fill(v, f, R), reps)
        tf, todd = t_solid_fill(v, f, R)
        r["torch_solid_same_grid_and_odd_columns"] = bool(torch.equal(tf, gf.dense()) and todd == odd)
        r["torch_points_ms"] = timed(lambda: t_points(v, R), reps)
        r["torch_points_same_grid"] = bool(torch.equal(t_points(v, R), VZ.voxelize_points(v, R).dense()))
        da, db = gf.dense(), gb.dense()
        r["torch_iou_on_dense_ms"] = timed(lambda: ((da & db).sum(), (da | db).sum()), reps)
        r["torch_iou_same_counts"] = bool(int(inter) == int((da & db).sum()) and int(union) == int((da | db).sum()))
        r["torch_over_library"] = {"surface": r["torch_surface_ms"] / r["surface_default_ms"], "solid_fill": r["torch_solid_fill_ms"] / r["solid_fill_only_ms"],
                                   "points": r["torch_points_ms"] / r["points_ms"], "iou": r["torch_iou_on_dense_ms"] / r["iou_paired_ms"]}
        r["triangles_per_s_surface_default"] = len(f) / (r["surface_default_ms"] * 1e-3)
        out["resolutions"][str(R)] = r
    out["notes"] = ["call times are device events around the Python call: they include the workspace allocation, the memsets and the counter copies",
                    "kernel times are averages over --trace-calls calls in a child process under the kernel trace; the torch IoU runs on dense bool grids, the library's on packed words",
                    "path='small' is not timed: it is a test switch"]
    out["not_measured"] = ["the share of the atomics against the box loops inside a kernel"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trace-calls", type=int, default=5)
    ap.add_argument("--workload", type=int, default=0, help="internal: run the traced workload at this resolution and exit")
    ap.add_argument("--output", default=None)
    a = ap.parse_args()
    if a.workload:
        return workload(a.workload, a.trace_calls)
    out = measure(a)
    print(json.dumps(out, indent=1))
    if a.output:
        os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
        with open(a.output, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
