#!/usr/bin/env python3
"""Device-event timing of ray casting on a mesh (surfd_amd.raycast, csrc/raycast.hip) after warm-up: for R = 500 000 rays and
procedural meshes of about 10^4 and 10^5 triangles (the shapes of tools/meshprep_time.py) it records the create time and, for
two workloads, the brute-force and the culled call (median of repeated calls, events on one stream), pairs per second and the
share of (wave, tile) visits that culling skipped; beside it, a chunked pure-torch restatement of the same fp64 pair test on
the same GPU as the comparison baseline.  The baseline lives only here: it is not a product path.

  count   +z rays from the pipeline's query points: the crossing count behind compute_occupancy / compute_signed_distance
  cast    rays from the same points in isotropic directions: first hits

    python tools/raycast_time.py [--out profiles/raycast_time.json] [--reps 10]

The times are those of surfd_rayscene_count / surfd_rayscene_cast on Morton-ordered inputs (the sort and the un-permutation
of surfd_amd.raycast are timed separately as "python_wrapper_ms").  Per-kernel times: `rocprofv3 --kernel-trace --stats` in a
run of its own."""
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


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def torch_count(v, t, rays, chunk=512):
    """the kernel's pair test (shear and scale in fp64, edge functions, the top-left rule, t rounded to fp32) as torch ops over
    [chunk, F]: every pair's intermediates go through HBM; -> crossing count [R] for tmin = 0, tmax = inf"""
    P = [v[t[:, k]].double().T.contiguous() for k in range(3)]               # [3, F] each
    o, d = rays[:, :3].double(), rays[:, 3:].double()
    kz = d.abs().argmax(1)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    dz = d.gather(1, kz[:, None])
    swap = dz[:, 0] < 0
    kx, ky = torch.where(swap, ky, kx), torch.where(swap, kx, ky)
    Sx, Sy, Sz = d.gather(1, kx[:, None]) / dz, d.gather(1, ky[:, None]) / dz, 1.0 / dz
    ox, oy, oz = o.gather(1, kx[:, None]), o.gather(1, ky[:, None]), o.gather(1, kz[:, None])
    out = []
    for i in range(0, len(rays), chunk):
        s = slice(i, i + chunk)

        def shear(p):
            z = p[kz[s]] - oz[s]
            return (p[kx[s]] - ox[s]) - Sx[s] * z, (p[ky[s]] - oy[s]) - Sy[s] * z, z
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = shear(P[0]), shear(P[1]), shear(P[2])
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        det = (U + V) + W
        sg = torch.where(det > 0, 1.0, -1.0).double()

        def edge(val, ex, ey):
            val, ex, ey = sg * val, sg * ex, sg * ey
            return (val > 0) | ((val == 0) & ((ey < 0) | ((ey == 0) & (ex < 0))))
        inside = edge(U, Bx - Cx, By - Cy) & edge(V, Cx - Ax, Cy - Ay) & edge(W, Ax - Bx, Ay - By) & (det != 0)
        tt = ((Sz[s] * ((U * Az + V * Bz) + W * Cz)) / det).float()
        out.append((inside & (tt >= 0) & (tt < INF)).sum(1).int())
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "raycast_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rays", type=int, default=500_000)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "raycast_time.py measures on the GPU"
    L = N.lib()
    rows = []
    share = [a.rays // 2, a.rays * 2 // 5, a.rays // 20]
    for n in (72, 225):                                          # 2 (n - 1)^2 = 10 082 and 100 352 triangles
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
        r = {"triangles": F, "rays": Rn, "pairs": F * Rn}
        r["create_ms"] = timed(lambda: RaycastingScene(vd, td), a.reps)
        scene = RaycastingScene(vd, td)
        order = M.morton_order(q.cuda())
        cnt = torch.empty(Rn, device="cuda", dtype=torch.int32)
        th = torch.empty(Rn, device="cuda")
        tri = torch.empty(Rn, device="cuda", dtype=torch.int32)
        uv = torch.empty(Rn, 2, device="cuda")
        nrm = torch.empty(Rn, 3, device="cuda")
        for work, d in (("count", up), ("cast", dirs)):
            rays = torch.cat([q, d], 1).cuda()
            rs = rays[order].contiguous()

            def call(flags):
                if work == "count":
                    N.check(L.surfd_rayscene_count(scene._handle, N.ptr(rs), Rn, 0.0, INF, flags, N.ptr(cnt), N.stream()))
                else:
                    N.check(L.surfd_rayscene_cast(scene._handle, N.ptr(rs), Rn, 0.0, INF, flags, N.ptr(th), N.ptr(tri), N.ptr(uv), N.ptr(nrm),
                                                  N.stream()))
            w = {}
            w["brute_force_ms"] = timed(lambda: call(1), max(3, a.reps // 3))
            brute = [x.clone() for x in (cnt, th, tri, uv, nrm)]
            w["culled_ms"] = timed(lambda: call(0), a.reps)
            w["culled_equals_brute_force"] = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((cnt, th, tri, uv, nrm), brute)) \
                if work == "cast" else bool(torch.equal(cnt, brute[0]))
            call(2)
            s, tot = N.C.c_int64(), N.C.c_int64()
            N.check(L.surfd_rayscene_skipped(scene._handle, N.C.byref(s), N.C.byref(tot), N.stream()))
            w["skipped_tiles"], w["total_tiles"], w["skipped_share"] = s.value, tot.value, s.value / tot.value
            w["python_wrapper_ms"] = timed((lambda: scene.count_intersections(rays)) if work == "count" else (lambda: scene.cast_rays(rays)), a.reps)
            w["brute_force_pairs_per_s"] = F * Rn / (w["brute_force_ms"]["median_ms"] * 1e-3)
            w["culled_pairs_per_s_equivalent"] = F * Rn / (w["culled_ms"]["median_ms"] * 1e-3)
            w["culled_over_brute_force"] = w["brute_force_ms"]["median_ms"] / w["culled_ms"]["median_ms"]
            if work == "count":
                w["rays_that_cross"] = int((brute[0] > 0).sum())
                if not a.no_baseline:
                    nb = 20_000                                  # the torch restatement is timed on a twenty-fifth of the rays
                    with torch.no_grad():
                        w["torch_ms_per_20k_rays"] = timed(lambda: torch_count(vd, td, rs[:nb]), 3)
                        w["torch_equals_kernel"] = bool(torch.equal(torch_count(vd, td, rs[:nb]), brute[0][:nb]))
                    w["torch_pairs_per_s"] = F * nb / (w["torch_ms_per_20k_rays"]["median_ms"] * 1e-3)
                    w["brute_force_over_torch"] = w["brute_force_pairs_per_s"] / w["torch_pairs_per_s"]
            else:
                w["rays_that_hit"] = int((brute[2] >= 0).sum())
            r[work] = w
        rows.append(r)
        print(json.dumps(r), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
