#!/usr/bin/env python3
"""Device-event timing of the Chamfer-matrix kernel (surfd_amd.cloudmetrics, csrc/cloudnn.hip) after warm-up: one direction
(surfd_cloud_nn_matrix) at N = 2 048 points per cloud for M = R in {64, 512} (median of 20 calls) and once for M = R = 2 000, as
time, point pairs per second and fraction of the chip's fp32 VALU issue rate (VALU instructions per pair of the inner loop from
the disassembly of the library that ran, the way tools/meshprep_time.py and DESIGN.md section 8.2 compute it); beside it, on the
same GPU and the same inputs at M = R = 64, a chunked pure-torch restatement with the same arithmetic as the comparison
baseline.  The baseline lives only here: it is not a product path.

    python tools/cloudmetrics_time.py [--out profiles/cloudmetrics_time.json] [--sizes 64 512] [--once 2000] [--reps 20]

Every size runs in a child process of its own under its own time limit (--step-timeout); the first step that fails ends the run.
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
# the chip's fp32 VALU issue rate: 256 CUs x 4 SIMDs x 32 lanes per clock (instructions, not FLOP), as tools/meshprep_time.py
LANES_PER_CLOCK = 256 * 4 * 32
PEAK_CLOCK_HZ = 2.4e9
N_POINTS = 2048


def inner_loop_valu(lib=None):
    """(VALU instructions, point pairs, the VALU opcodes) of one trip of cn_matrix_kernel<8>'s inner loop: the basic block of the
    kernel that holds the most v_* instructions and ends in a backward branch; a trip reads CN_UNROLL candidates (one
    ds_read per candidate) for the lane's 8 query points"""
    from surfd_amd import _native as N
    lib = lib or N.LIB_PATH
    asm = ""
    with tempfile.TemporaryDirectory() as td:
        loc = os.path.join(td, "lib.so")
        shutil.copy(lib, loc)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", loc], check=True, capture_output=True, cwd=td)
        for co in sorted(os.listdir(td)):                      # one code object per translation unit
            if "gfx950" in co:
                asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", os.path.join(td, co)], check=True, capture_output=True, text=True).stdout
                if "cn_matrix_kernelILi8" in asm:
                    break
    m = re.search(r"<_ZN5surfd16cn_matrix_kernelILi8E[^>]*>:\n(.*?)(?=\n\n[0-9a-f]+ <|\Z)", asm, re.S)
    if not m:
        raise RuntimeError("cn_matrix_kernel<8> not found in the library's gfx950 code objects")
    best, cur = [], []
    for line in m.group(1).splitlines():
        ins = line.strip().split()
        if not ins:
            continue
        cur.append(ins[0])
        if ins[0].startswith(("s_cbranch", "s_branch", "s_endpgm")):
            if ins[0].startswith("s_cbranch") and sum(o.startswith("v_") for o in cur) > sum(o.startswith("v_") for o in best):
                best = cur
            cur = []
    ops = [o for o in best if o.startswith("v_")]
    reads = sum(o.startswith("ds_read") for o in best)
    return len(ops), reads * 8, sorted(set(ops))


def clouds(M, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(M, N_POINTS, 3, generator=g)
    ax = torch.rand(M, 1, 3, generator=g) * 0.6 + 0.3
    return (v / v.norm(dim=-1, keepdim=True) * ax).float().cuda()


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


def torch_directed_means(A, B, rows=8):
    """the kernel's arithmetic as torch ops: (a[:, None] - b[None]).square(), the three coordinates added in the kernel's order,
    amin over the candidates, fp64 mean over the points; `rows` query clouds x one candidate cloud per step, so that the
    [rows, N, N, 3] intermediate (400 MB at 8 x 2 048^2) goes through HBM"""
    import torch
    out = torch.empty(A.shape[0], B.shape[0], device=A.device, dtype=torch.float32)
    for i0 in range(0, A.shape[0], rows):
        a = A[i0:i0 + rows]
        for j in range(B.shape[0]):
            sq = (a[:, :, None, :] - B[j][None, None, :, :]).square()
            d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
            out[i0:i0 + rows, j] = (d2.amin(-1).double().sum(-1) / a.shape[1]).float()
    return out


def child(M, reps, baseline):
    import torch
    from surfd_amd import _native as N
    assert torch.cuda.is_available(), "cloudmetrics_time.py measures on the GPU"
    L = N.lib()
    A, B = clouds(M, 1), clouds(M, 2)
    mean = torch.empty(M, M, device="cuda")
    below = torch.empty(M, M, device="cuda", dtype=torch.int32)

    def call():
        N.check(L.surfd_cloud_nn_matrix(N.ptr(A), M, N_POINTS, N.ptr(B), M, N_POINTS, 1e-4, N.ptr(mean), N.ptr(below), N.stream()))

    r = {"M": M, "R": M, "points": N_POINTS, "pairs": M * M * N_POINTS * N_POINTS}
    r["native_ms"] = timed(call, reps, warm=2 if reps > 1 else 1)
    sec = r["native_ms"]["median_ms"] * 1e-3
    r["native_pairs_per_s"] = r["pairs"] / sec
    valu, pairs, ops = inner_loop_valu()
    r["valu_per_pair"] = valu / pairs
    r["inner_loop_valu_opcodes"] = ops
    r["peak_clock_mhz_assumed"] = PEAK_CLOCK_HZ / 1e6
    r["fraction_of_fp32_valu_issue_rate"] = (r["pairs"] * valu / pairs / sec) / (LANES_PER_CLOCK * PEAK_CLOCK_HZ)
    if baseline:
        with torch.no_grad():
            r["torch_ms"] = timed(lambda: torch_directed_means(A, B), 3, warm=1)
            ref = torch_directed_means(A, B)
        r["torch_equals_native_bitwise_share"] = float((ref == mean).double().mean())
        r["torch_max_rel_diff"] = float(((ref - mean).abs() / mean).max())
        r["torch_pairs_per_s"] = r["pairs"] / (r["torch_ms"]["median_ms"] * 1e-3)
        r["native_over_torch"] = r["torch_ms"]["median_ms"] / r["native_ms"]["median_ms"]
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "cloudmetrics_time.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 512])
    ap.add_argument("--once", type=int, nargs="*", default=[2000], help="sizes timed with a single call after one warm-up call")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-at", type=int, default=64)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--child-reps", type=int, default=20, help=argparse.SUPPRESS)
    ap.add_argument("--child-baseline", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.child_reps, a.child_baseline)
    rows, device = [], None
    for M, reps in [(m, a.reps) for m in a.sizes] + [(m, 1) for m in a.once]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", str(M), "--child-reps", str(reps)]
        if M == a.baseline_at:
            cmd.append("--child-baseline")
        p = subprocess.run(cmd, capture_output=True, text=True)
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:                       # nothing more is started after a failed GPU step
            print(p.stdout[-2000:], p.stderr[-2000:], file=sys.stderr)
            raise SystemExit(f"step M = {M} failed with exit status {p.returncode}; stopping")
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
