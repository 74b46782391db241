#!/usr/bin/env python3
"""Device-event timing of the mesh hierarchy (csrc/meshbvh.hip, accel="bvh") against the tile paths it is an alternative to, in
one process and on one handle per mesh: for 500 000 rays or queries (the generators of tools/raycast_time.py) and wavy sheets
of 10 082, 100 352 and 445 568 triangles (the last is the size of the pipeline's own meshes) it records the build time of the
hierarchy and, for three workloads, the median of repeated calls by tiles and by the hierarchy, whether the outputs are the
same bits, and the hierarchy's box tests and pair tests per ray or query:

  cast     rays from the pipeline's query points in isotropic directions: first hits
  count    +z rays from the same points: the crossing count behind compute_occupancy / compute_signed_distance
  closest  the query points themselves: closest points

    python tools/meshbvh_time.py [--out profiles/meshbvh_time.json] [--reps 10]

The times are those of the C ABI calls on Morton-ordered inputs, as in tools/raycast_time.py and tools/meshprep_time.py."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import mesh_udf_ref as R  # noqa: E402
from surfd_amd import _native as N  # noqa: E402
from surfd_amd import meshprep as M  # noqa: E402
from surfd_amd.raycast import RaycastingScene  # noqa: E402

INF = float("inf")
BVH, VISITS = 4, 8


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


def build_time(make, build, reps):
    """the build alone, on a fresh handle every time"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for i in range(reps + 1):
        obj = make()
        torch.cuda.synchronize()
        a.record(); build(obj); b.record(); torch.cuda.synchronize()
        if i:
            times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshbvh_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rays", type=int, default=500_000)
    ap.add_argument("--sheets", type=int, nargs="+", default=[72, 225, 473])      # 2 (n - 1)^2 = 10 082, 100 352, 445 568 triangles
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshbvh_time.py measures on the GPU"
    L = N.lib()
    rows = []
    share = [a.rays // 2, a.rays * 2 // 5, a.rays // 20]
    for n in a.sheets:
        v, t = R.wavy_sheet(n)
        g = torch.Generator().manual_seed(7)
        pcd = M.sample_points_uniformly(torch.from_numpy(v), torch.from_numpy(t), 100_000, generator=g)
        torch.manual_seed(7)
        q = M.sample_points_around_pcd(pcd, [0.003, 0.01, 0.1], share + [a.rays - sum(share)], (-1.0, 1.0), "cpu")
        dirs = torch.nn.functional.normalize(torch.randn(len(q), 3, generator=g), dim=1)
        up = torch.zeros(len(q), 3)
        up[:, 2] = 1.0
        vd, td = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        F, Rn = len(t), len(q)
        r = {"triangles": F, "rays_or_queries": Rn, "leaf_triangles": 4, "node_children": 4}
        r["build_ms"] = {"rayscene": build_time(lambda: RaycastingScene(vd, td), lambda s: N.check(L.surfd_rayscene_build_bvh(s._handle, N.stream())), a.reps),
                         "mesh": build_time(lambda: M.MeshDistance(vd, td), lambda m: N.check(L.surfd_mesh_build_bvh(m._handle, N.stream())), a.reps)}
        scene = RaycastingScene(vd, td, accel="bvh")
        md = M.MeshDistance(vd, td, accel="bvh")
        r["levels"] = len(scene.read_bvh()["level_sizes"])
        qd = q.cuda()
        order = M.morton_order(qd)
        cnt = torch.empty(Rn, device="cuda", dtype=torch.int32)
        th = torch.empty(Rn, device="cuda")
        tri = torch.empty(Rn, device="cuda", dtype=torch.int32)
        uv = torch.empty(Rn, 2, device="cuda")
        nrm = torch.empty(Rn, 3, device="cuda")
        dist = torch.empty(Rn, device="cuda")
        pts = torch.empty(Rn, 3, device="cuda")
        qs = qd[order].contiguous()
        for work, d in (("cast", dirs), ("count", up), ("closest", None)):
            rs = torch.cat([q, d], 1).cuda()[order].contiguous() if d is not None else None

            def call(flags):
                if work == "count":
                    N.check(L.surfd_rayscene_count(scene._handle, N.ptr(rs), Rn, 0.0, INF, flags, N.ptr(cnt), N.stream()))
                elif work == "cast":
                    N.check(L.surfd_rayscene_cast(scene._handle, N.ptr(rs), Rn, 0.0, INF, flags, N.ptr(th), N.ptr(tri), N.ptr(uv), N.ptr(nrm),
                                                  N.stream()))
                elif flags & BVH:
                    N.check(L.surfd_mesh_closest_bvh(md._handle, N.ptr(qs), Rn, 2 if flags & VISITS else 0, N.ptr(dist), N.ptr(pts), N.ptr(tri),
                                                     None, N.stream()))
                else:
                    N.check(L.surfd_mesh_closest(md._handle, N.ptr(qs), Rn, 0, N.ptr(dist), N.ptr(pts), N.ptr(tri), None, N.stream()))
            outs = {"count": (cnt,), "cast": (th, tri, uv, nrm), "closest": (dist, pts, tri)}[work]
            w = {}
            w["tiles_ms"] = timed(lambda: call(0), a.reps)
            tiles = [x.clone() for x in outs]
            w["bvh_ms"] = timed(lambda: call(BVH), a.reps)
            w["bvh_equals_tiles"] = all(bool(torch.equal(bits(x), bits(y))) for x, y in zip(outs, tiles))
            call(BVH | VISITS)
            b, p = N.C.c_int64(), N.C.c_int64()
            N.check((L.surfd_mesh_visits if work == "closest" else L.surfd_rayscene_visits)((md if work == "closest" else scene)._handle,
                                                                                            N.C.byref(b), N.C.byref(p), N.stream()))
            w["box_tests_per_lane"], w["pair_tests_per_lane"] = b.value / Rn, p.value / Rn
            w["tiles_over_bvh"] = w["tiles_ms"]["median_ms"] / w["bvh_ms"]["median_ms"]
            if work == "cast":
                w["rays_that_hit"] = int((tiles[1] >= 0).sum())
            if work == "count":
                w["rays_that_cross"] = int((tiles[0] > 0).sum())
            r[work] = w
        rows.append(r)
        print(json.dumps(r), flush=True)
        out = {"device": torch.cuda.get_device_name(0), "rows": rows,
               "variants_tried": [{"leaf_triangles": 4, "node_children": 4, "note": "the only pair built: the walk keeps 4 bits per level in one "
                                   "64-bit word and loads a node's boxes as float4 (meshbvh_layout.h static_asserts both)"}]}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                            # after every row: a run that is cut short keeps what it measured
            json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
