#!/usr/bin/env python3
"""Device-event timing of the mesh closest-point search (surfd_amd.meshprep, csrc/meshdist.hip) after warm-up: for Q = 500 000
pipeline-made queries and procedural meshes of about 10^4 and 10^5 triangles it records the create time, the brute-force and the
culled call (median of repeated calls, events on one stream), pairs per second, the share of (wave, tile) visits that culling
skipped, the VALU instructions per pair of the brute-force kernel's inner loop (from the disassembly) and with it the fraction
of the chip's fp32 VALU issue rate that kernel reaches; beside it, a chunked pure-torch restatement of the same pair test on the
same GPU as the comparison baseline.  The baseline lives only here: it is not a product path.

    python tools/meshprep_time.py [--out profiles/meshprep_time.json] [--reps 10]

The times are those of surfd_mesh_closest on Morton-ordered inputs (the sort and the un-permutation of surfd_amd.meshprep are
timed separately as "python_wrapper_ms").  Per-kernel times: `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import mesh_udf_ref as R  # noqa: E402
from surfd_amd import _native as N  # noqa: E402
from surfd_amd import meshprep as M  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"
# the chip's fp32 VALU issue rate: 256 CUs x 4 SIMDs x 32 lanes per clock (an fma counts once here: instructions, not FLOP)
LANES_PER_CLOCK = 256 * 4 * 32
PEAK_CLOCK_HZ = 2.4e9                  # the clock behind the MI355X's 157.3 TFLOP/s fp32 vector peak (2 FLOP per lane-fma)


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


def inner_loop_valu(lib=None):
    """VALU instructions per (query, triangle) pair: the v_* instructions of the basic block of md_closest_kernel<false> that
    holds the most of them and ends in a backward branch (the loop over the records of a tile; hipcc does not unroll it)"""
    lib = lib or N.LIB_PATH
    with tempfile.TemporaryDirectory() as td:
        loc = os.path.join(td, "lib.so")
        shutil.copy(lib, loc)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", loc], check=True, capture_output=True, cwd=td)
        asm = ""
        for co in sorted(os.listdir(td)):                      # one code object per translation unit
            if "gfx950" in co:
                asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", os.path.join(td, co)], check=True, capture_output=True, text=True).stdout
                if "md_closest_kernelILb0" in asm:
                    break
    m = re.search(r"<_ZN5surfd17md_closest_kernelILb0EE[^>]*>:\n(.*?)(?=\n\n[0-9a-f]+ <|\Z)", asm, re.S)
    if not m:
        return None
    best, cur = 0, 0
    for line in m.group(1).splitlines():
        ins = line.strip().split()
        if not ins:
            continue
        op = ins[0]
        if op.startswith("v_"):
            cur += 1
        elif op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_barrier")):
            if op.startswith("s_cbranch"):
                best = max(best, cur)
            cur = 0
    return best or None


def torch_pair_test(v, t, q, chunk=4096):
    """the kernel's pair test (three edge segments from their own start vertices, and the plane where the query projects inside
    all three edges; normals from an fp64 cross product per triangle) as torch ops over [chunk, F]: every pair's intermediates
    go through HBM; -> squared distance of the nearest triangle [Q]"""
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    ab, ac, bc = (b - a)[None], (c - a)[None], (c - b)[None]
    inv = lambda e: torch.where((e * e).sum(-1) > 0, 1 / (e * e).sum(-1).clamp_min(1e-38), torch.zeros_like(e[..., 0]))
    n = torch.linalg.cross((b - a).double(), (c - a).double())
    nn = (n * n).sum(-1, keepdim=True)
    n = torch.where(nn > 0, n / nn.clamp_min(1e-290).sqrt(), torch.zeros_like(n))
    mab = torch.linalg.cross(n, (b - a).double()).float()[None]
    mbc = torch.linalg.cross(n, (c - b).double()).float()[None]
    mca = torch.linalg.cross(n, (a - c).double()).float()[None]
    n = n.float()[None]
    iab, iac, ibc = inv(ab), inv(ac), inv(bc)

    def seg(r, e, ie, sgn):
        tt = (sgn * (e * r).sum(-1) * ie).clamp(0, 1)
        d = r - (sgn * tt)[..., None] * e
        return (d * d).sum(-1)

    out = []
    for i in range(0, len(q), chunk):
        ra = q[i:i + chunk, None] - a[None]
        rb, rc = ra - ab, ra - ac
        de = torch.minimum(seg(ra, ab, iab, 1.0), torch.minimum(seg(rb, bc, ibc, 1.0), seg(rc, ac, iac, -1.0)))
        h = (n * ra).sum(-1)
        inside = torch.minimum((mab * ra).sum(-1), torch.minimum((mbc * rb).sum(-1), (mca * rc).sum(-1))) > 0
        out.append(torch.where(inside, torch.minimum(de, h * h), de).min(1).values)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshprep_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=500_000)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshprep_time.py measures on the GPU"
    L = N.lib()
    valu = inner_loop_valu()
    rows = []
    share = [a.queries // 2, a.queries * 2 // 5, a.queries // 20]
    for n in (72, 225):                                          # 2 (n - 1)^2 = 10 082 and 100 352 triangles
        v, t = R.wavy_sheet(n)
        g = torch.Generator().manual_seed(7)
        pcd = M.sample_points_uniformly(torch.from_numpy(v), torch.from_numpy(t), 100_000, generator=g)
        torch.manual_seed(7)
        q = M.sample_points_around_pcd(pcd, [0.003, 0.01, 0.1], share + [a.queries - sum(share)], (-1.0, 1.0), "cpu").cuda()
        vd, td = torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()
        F, Q = len(t), len(q)
        r = {"triangles": F, "queries": Q, "pairs": F * Q}
        r["create_ms"] = timed(lambda: M.MeshDistance(vd, td), a.reps)
        md = M.MeshDistance(vd, td)
        qs = q[M.morton_order(q)].contiguous()
        dist = torch.empty(Q, device="cuda")
        pts = torch.empty(Q, 3, device="cuda")
        tri = torch.empty(Q, device="cuda", dtype=torch.int32)
        skipped = torch.zeros(1, device="cuda", dtype=torch.int64)

        def call(flags, sk=None):
            N.check(L.surfd_mesh_closest(md._handle, N.ptr(qs), Q, flags, N.ptr(dist), N.ptr(pts), N.ptr(tri), N.ptr(sk), N.stream()))

        r["brute_force_ms"] = timed(lambda: call(1), max(3, a.reps // 3))
        brute = (dist.clone(), pts.clone(), tri.clone())
        r["culled_ms"] = timed(lambda: call(0), a.reps)
        r["culled_equals_brute_force"] = bool(torch.equal(dist, brute[0]) and torch.equal(pts, brute[1]) and torch.equal(tri, brute[2]))
        call(0, skipped)
        total = ((Q + 63) // 64) * ((F + 31) // 32)
        r["skipped_tiles"], r["total_tiles"] = int(skipped.item()), total
        r["skipped_share"] = r["skipped_tiles"] / total
        r["python_wrapper_ms"] = timed(lambda: md.closest(q), a.reps)
        bf_s = r["brute_force_ms"]["median_ms"] * 1e-3
        r["brute_force_pairs_per_s"] = F * Q / bf_s
        r["culled_pairs_per_s_equivalent"] = F * Q / (r["culled_ms"]["median_ms"] * 1e-3)
        if valu:
            r["valu_per_pair"] = valu
            r["peak_clock_mhz_assumed"] = PEAK_CLOCK_HZ / 1e6
            r["brute_force_fraction_of_fp32_valu_issue_rate"] = (F * Q * valu / bf_s) / (LANES_PER_CLOCK * PEAK_CLOCK_HZ)
        if not a.no_baseline:
            nb = 50_000                                          # the torch restatement is timed on a tenth of the queries
            with torch.no_grad():
                r["torch_ms_per_50k_queries"] = timed(lambda: torch_pair_test(vd, td, qs[:nb]), 3)
                r["torch_max_abs_diff_dist"] = float((torch_pair_test(vd, td, qs[:nb]).sqrt() - brute[0][:nb]).abs().max())
            r["torch_pairs_per_s"] = F * nb / (r["torch_ms_per_50k_queries"]["median_ms"] * 1e-3)
            r["brute_force_over_torch"] = r["brute_force_pairs_per_s"] / r["torch_pairs_per_s"]
        r["culled_over_brute_force"] = r["brute_force_ms"]["median_ms"] / r["culled_ms"]["median_ms"]
        rows.append(r)
        print(json.dumps(r), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
