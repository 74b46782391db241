#!/usr/bin/env python3
"""Device-event timing of the normal estimation (surfd_amd.cloudnormals, csrc/cloudnormals.hip) after warm-up: surfd_cloud_normals
with neighbour indices at (B, N, K) = (64, 2048, 16), (512, 2048, 16), (8, 100000, 32), (64, 2048, 64) (median of 20 calls) as
time, candidate pairs per second (B N^2) and fraction of the chip's fp32 VALU issue rate, computed as tools/cloudmetrics_time.py
and DESIGN.md section 8.3 compute it (VALU instructions per pair of the scan's common trip from the disassembly of the library
that ran; the insertions, the moments and the Jacobi sweeps are not counted, so the fraction is that of the pair tests alone).
Beside it, on the same GPU and the same inputs where K <= 32 and N = 2 048, the existing pieces composed in torch as the
comparison baseline: dgcnn.knn_points + gather + fp64 covariances + torch.linalg.eigh; the ratio of the two times, and whether
the baseline's normals agree with the kernel's up to sign within the bound of tests/test_cloudnormals_cpu.py (32 2^-52 / gap).
The baseline lives only here: it is not a product path.

    python tools/cloudnormals_time.py [--out profiles/cloudnormals_time.json] [--reps 20]

Every shape runs in a child process of its own under its own time limit (--step-timeout); the first step that fails ends the run.
SURFD_LIB selects a differently built library (A/B of build variants); the JSON names the library it measured."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLVM = "/opt/rocm/lib/llvm/bin"
# the chip's fp32 VALU issue rate: 256 CUs x 4 SIMDs x 32 lanes per clock (instructions, not FLOP), as tools/cloudmetrics_time.py
LANES_PER_CLOCK = 256 * 4 * 32
PEAK_CLOCK_HZ = 2.4e9
SHAPES = [(64, 2048, 16), (512, 2048, 16), (8, 100000, 32), (64, 2048, 64)]
ANGLE_BOUND = 32 * 2.0 ** -52
TILE_READS = ("ds_read_b96", "ds_read_b128")     # a candidate of the tile: three floats of a float4


def scan_trip_valu(T, lib=None):
    """(VALU instructions, candidates, the VALU opcodes) of the common trip of cnrm_kernel<T>'s scan: the basic block of the
    kernel that holds the most broadcast reads of the candidate tile (one ds_read_b96 or ds_read_b128 per candidate) and ends in
    a conditional branch (the test whether any of the trip's candidates enters a list)"""
    from surfd_amd import _native as N
    lib = lib or N.LIB_PATH
    asm, tag = "", f"cnrm_kernelILi{T}E"
    with tempfile.TemporaryDirectory() as td:
        loc = os.path.join(td, "lib.so")
        shutil.copy(lib, loc)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", loc], check=True, capture_output=True, cwd=td)
        for co in sorted(os.listdir(td)):                      # one code object per translation unit
            if "gfx950" in co:
                asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", os.path.join(td, co)], check=True, capture_output=True, text=True).stdout
                if tag in asm:
                    break
    m = re.search(r"<_ZN5surfd11" + tag + r"[^>]*>:\n(.*?)(?=\n\n[0-9a-f]+ <|\Z)", asm, re.S)
    if not m:
        raise RuntimeError(f"cnrm_kernel<{T}> not found in the library's gfx950 code objects")
    best, cur = [], []
    for line in m.group(1).splitlines():
        ins = line.strip().split()
        if not ins:
            continue
        cur.append(ins[0])
        if ins[0].startswith(("s_cbranch", "s_branch", "s_endpgm")):
            if ins[0].startswith("s_cbranch") and sum(o in TILE_READS for o in cur) > sum(o in TILE_READS for o in best):
                best = cur
            cur = []
    ops = [o for o in best if o.startswith("v_")]
    cands = sum(o in TILE_READS for o in best)
    if cands == 0:
        raise RuntimeError(f"cnrm_kernel<{T}>: no block with one {' / '.join(TILE_READS)} per candidate found; the scan is compiled "
                           "in a form this counter does not know")
    return len(ops), cands, sorted(set(ops))


def clouds(B, n, seed):
    """B ellipsoid shells of n points with seeded semi-axes, as tools/cloudmetrics_time.py"""
    import torch
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, n, 3, generator=g)
    ax = torch.rand(B, 1, 3, generator=g) * 0.6 + 0.3
    return (v / v.norm(dim=-1, keepdim=True) * ax).float().contiguous().cuda()


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


def torch_composition(x, K):
    """the existing pieces: dgcnn.knn_points, a gather, the covariance of the differences in fp64, torch.linalg.eigh
    -> (normals [B, N, 3] fp64 unsigned, eigenvalues [B, N, 3] fp64 ascending)"""
    import torch
    from surfd_amd.dgcnn import knn_points
    _, idx = knn_points(x, K)
    B, n, _ = x.shape
    nb = x[torch.arange(B, device=x.device)[:, None, None], idx]
    d = (nb - x[:, :, None, :]).double()
    m = d.mean(2)
    C = torch.einsum("bnka,bnkc->bnac", d, d) / K - m[..., :, None] * m[..., None, :]
    lam, vec = torch.linalg.eigh(C)
    return vec[..., 0], lam


def child(B, n, K, reps, baseline):
    import torch
    from surfd_amd import _native as N
    assert torch.cuda.is_available(), "cloudnormals_time.py measures on the GPU"
    L = N.lib()
    x = clouds(B, n, 1)
    normals = torch.empty(B, n, 3, device="cuda")
    eig = torch.empty(B, n, 3, device="cuda")
    idx = torch.empty(B, n, K, device="cuda", dtype=torch.int32)

    def call():
        N.check(L.surfd_cloud_normals(N.ptr(x), B, n, None, K, N.ptr(normals), N.ptr(eig), N.ptr(idx), N.stream()))

    T = 256 if K <= 32 else 128
    r = {"B": B, "N": n, "K": K, "lanes_per_workgroup": T, "pairs": B * n * n}
    r["native_ms"] = timed(call, reps)
    sec = r["native_ms"]["median_ms"] * 1e-3
    r["native_pairs_per_s"] = r["pairs"] / sec
    valu, cands, ops = scan_trip_valu(T)
    r["valu_per_pair"] = valu / cands
    r["scan_trip_valu_opcodes"] = ops
    r["peak_clock_mhz_assumed"] = PEAK_CLOCK_HZ / 1e6
    r["fraction_of_fp32_valu_issue_rate"] = (r["pairs"] * valu / cands / sec) / (LANES_PER_CLOCK * PEAK_CLOCK_HZ)
    if baseline:
        try:
            with torch.no_grad():
                r["torch_ms"] = timed(lambda: torch_composition(x, K), 3, warm=1)
                n_t, lam_t = torch_composition(x, K)
            r["native_over_torch"] = r["torch_ms"]["median_ms"] / r["native_ms"]["median_ms"]
            gap = (lam_t[..., 1] - lam_t[..., 0]) / lam_t[..., 2]
            nn = normals.double()
            angle = torch.atan2(torch.linalg.cross(nn, n_t).norm(dim=-1), (nn * n_t).sum(-1).abs())
            # the kernel's normal is rounded to fp32: half an ulp per component on top of the solvers' bound
            ok = angle <= ANGLE_BOUND / gap + 3 ** 0.5 * 2.0 ** -24
            r["torch_normals_agree_share"] = float(ok.double().mean())
            r["torch_normals_agree"] = bool(ok.all())
            r["torch_largest_angle_rad"] = float(angle.max())
            r["torch_smallest_gap"] = float(gap.min())
        except Exception as e:                                  # recorded, not hidden: the baseline is a comparison, not a product path
            r["torch_error"] = f"{type(e).__name__}: {e}"[:400]
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "cloudnormals_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--child", type=int, nargs=3, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-baseline", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.reps, a.child_baseline)
    rows = []
    for B, n, K in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", str(B), str(n), str(K),
               "--reps", str(a.reps)]
        if K <= 32 and n <= 2048 and not a.no_baseline:
            cmd.append("--child-baseline")
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:                       # nothing more is started after a failed GPU step
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"step (B, N, K) = ({B}, {n}, {K}) failed with exit status {p.returncode}; stopping")
        rows.append(json.loads(res[0][len("RESULT "):]))
        print(json.dumps(rows[-1]), flush=True)
    import torch
    from surfd_amd import _native as N
    out = {"device": torch.cuda.get_device_name(0), "library": os.path.relpath(N.LIB_PATH, ROOT), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
