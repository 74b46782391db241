#!/usr/bin/env python3
"""Times the isotropic remeshing on the device (surfd_amd.meshremesh.remesh_isotropic, csrc/meshremesh.hip).  Inputs:

  shell(256)              marching_cubes_device on the sphere-shell field min(| |p| - 0.6 |, 0.1) at 256^3, level 0.01: 441 304 faces
  shell(256) decimated    the same shell after simplify_quadric_decimation to 62 976 faces

each remeshed at L = its mean edge length, 5 iterations, without and with ``project``.  Before anything is timed the device result
is compared with tests/meshremesh_ref.py for equal bits and order (vertices, faces, origin, counts) on shell(--check), a size the
restatement can do, or the run stops.  Per case: the call's device time as a consumer calls it (float64 vertices and int64 faces on
the device; the host reads of every round lie inside the bracket), median of --reps calls after --warmup, by events on the stream;
the counts of every iteration; per stage, the time of the stage run alone on a handle (MeshRemesher.iterate with the other stages'
rounds at 0, in the order of an iteration: the same state, checked against the whole call) and that time over the rounds it made;
triangle_quality before and after; the largest and mean distance of the output vertices from the two analytic spheres of radius
0.6 +- 0.01 (in the field's units, the cube [-1, 1]^3); ``roof_ms``, the time to stream the call's input and output bytes once at
8 TB/s.  Nothing is asserted about the times or the quality: a case whose quality gets worse in one of the three measures of
tests/test_meshremesh_cpu.py is listed under "quality_worse", one whose last iteration still split, collapsed or flipped under
"not_settled".

The measurement runs in one child process under a time limit; the parent only waits and reports.

    python tools/time_meshremesh.py [--out profiles/meshremesh_time.json] [--reps 20] [--warmup 3] [--shell 256] [--decimated 62976] [--check 64] [--limit 900]
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
ITERATIONS = 5
STAGES = (("split", (4, 0, 0, 0)), ("collapse", (0, 16, 0, 0)), ("flip", (0, 0, 4, 0)), ("relax", (0, 0, 0, 1)))
ROUNDS_OF = {"split": "split_rounds", "collapse": "collapse_rounds", "flip": "flip_rounds"}


def shell_distance(p, n):
    p = p * (2.0 / (n - 1)) - 1.0                              # the meshes are in voxel-index units
    r = (p * p).sum(dim=1).sqrt()
    d = ((r - 0.6).abs() - 0.01).abs()
    return {"max": float(d.max()), "mean": float(d.mean())} if len(d) else {"max": None, "mean": None}


def check(n):
    import numpy as np
    import torch
    import meshremesh_ref as R
    from surfd_amd.meshremesh import remesh_isotropic
    from time_meshclean import shell
    v, f = shell(n)
    L = R.mean_edge_length(v, f)
    wv, wf, wo, ws = R.remesh(v, f, L, iterations=2)
    gv, gf, go, gs = remesh_isotropic(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), L, iterations=2, return_origin=True, return_stats=True)
    equal = (gs == ws and np.array_equal(gv.cpu().numpy().view(np.int64), wv.view(np.int64)) and np.array_equal(gf.cpu().numpy(), wf)
             and np.array_equal(go.cpu().numpy(), wo))
    assert equal, f"shell({n}) at L = {L}: the device differs from the restatement ({gs} / {ws})"
    return {"mesh": f"shell({n})", "faces": len(f), "L": L, "iterations": 2, "faces_after": len(wf), "equal_to_restatement": True}


def stage_times(vd, fd, L, whole):
    """one handle stepped stage by stage through ITERATIONS iterations, each stage's call timed by events; the state it ends in is
    the whole call's"""
    import torch
    from surfd_amd.meshremesh import MeshRemesher
    r = MeshRemesher(vd, fd, (0.8 * L) * (0.8 * L), (4.0 / 3.0 * L) * (4.0 / 3.0 * L))
    rows = []
    for it in range(ITERATIONS):
        row = {}
        for stage, rounds in STAGES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); c = r.iterate(*rounds); b.record(); torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            made = c[ROUNDS_OF[stage]] if stage in ROUNDS_OF else 1
            row[stage] = {"ms": ms, "rounds": made, "ms_per_round": ms / max(made, 1)}
        rows.append(row)
    gv, gf, _ = r.emit()
    assert torch.equal(gf, whole[1]) and torch.equal(gv.view(torch.int64), whole[0].view(torch.int64)), "the stages alone end elsewhere than the whole call"
    return rows


def measure(name, n, vd, fd, project, a):
    from surfd_amd.meshremesh import mean_edge_length, remesh_isotropic, triangle_quality
    from time_meshclean import timed
    L = mean_edge_length(vd, fd)
    ov, of, stats = remesh_isotropic(vd, fd, L, iterations=ITERATIONS, project=project, return_stats=True)
    nbytes = 24 * len(vd) + 12 * len(fd) + 24 * len(ov) + 12 * len(of)
    ms = timed(lambda: remesh_isotropic(vd, fd, L, iterations=ITERATIONS, project=project), a.reps, a.warmup)
    before, after = triangle_quality(vd, fd, L), triangle_quality(ov, of, L)
    rounds = sum(s["split_rounds"] + s["collapse_rounds"] + s["flip_rounds"] + 1 for s in stats)
    row = {"mesh": name, "faces": len(fd), "vertices": len(vd), "L": L, "project": project, "iterations_made": len(stats), "faces_after": len(of),
           "vertices_after": len(ov), "remesh_ms": ms, "rounds": rounds, "ms_per_round": ms["median_ms"] / max(rounds, 1), "stats": stats,
           "quality_before": before, "quality_after": after, "distance_before": shell_distance(vd, n), "distance_after": shell_distance(ov, n),
           "bytes": nbytes, "roof_ms": nbytes / ROOF_BYTES_PER_MS, "remesh_over_roof": ms["median_ms"] / (nbytes / ROOF_BYTES_PER_MS)}
    if not project:
        row["stages"] = stage_times(vd, fd, L, (ov, of))
    return row


def child(a):
    import torch
    from surfd_amd.meshsimplify import simplify_quadric_decimation
    from time_meshclean import shell
    assert torch.cuda.is_available(), "time_meshremesh.py measures on the GPU"
    checked = check(a.check)
    print(json.dumps(checked), flush=True)
    v, f = shell(a.shell)
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    dv, df = simplify_quadric_decimation(vd, fd, a.decimated)
    rows = []
    for name, mv, mf in ((f"shell({a.shell})", vd, fd), (f"shell({a.shell}) decimated to {len(df)}", dv, df)):
        for project in (False, True):
            rows.append(measure(name, a.shell, mv, mf, project, a))
            print(json.dumps({k: x for k, x in rows[-1].items() if k not in ("stats", "stages")}), flush=True)

    def worse(r):
        b, c = r["quality_before"], r["quality_after"]
        return [k for k, up in (("edges_in_range", True), ("min_angle_mean", True), ("valence_deviation_mean", False)) if (c[k] < b[k]) == up and c[k] != b[k]]
    out = {"tool": "tools/time_meshremesh.py", "device": torch.cuda.get_device_name(0),
           "what": f"remesh_ms: medians of {a.reps} calls of remesh_isotropic(L = the mean edge length, iterations={ITERATIONS}) after {a.warmup} warm-up calls, by "
                   "events on the stream (host reads included); stages: each stage of each iteration alone on one handle, one timed call each; distances: of the "
                   "vertices from the two spheres of radius 0.6 +- 0.01; roof_ms: the call's input and output bytes streamed once at 8 TB/s",
           "checked_first": checked, "rows": rows,
           "quality_worse": [f"{r['mesh']} project={r['project']}: {worse(r)}" for r in rows if worse(r)],
           "not_settled": [f"{r['mesh']} project={r['project']}" for r in rows
                           if r["stats"][-1]["splits"] + r["stats"][-1]["collapses"] + r["stats"][-1]["flips"] > 0]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshremesh_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shell", type=int, default=256)
    ap.add_argument("--decimated", type=int, default=62976, help="the face count the second input is decimated to")
    ap.add_argument("--check", type=int, default=64, help="the shell on which the device is compared with the restatement first")
    ap.add_argument("--limit", type=int, default=900, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--out", a.out, "--reps", str(a.reps), "--warmup", str(a.warmup), "--check", str(a.check),
           "--shell", str(a.shell), "--decimated", str(a.decimated)]
    try:
        r = subprocess.run(cmd, timeout=a.limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"the measurement did not finish within {a.limit} s")
    raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
