#!/usr/bin/env python3
"""Device-event timing of the farthest point sampling (surfd_amd.cloudsample, csrc/cloudfps.hip) after warm-up: the library
call surfd_cloud_fps at (B, N, K) = (1, 2048, 512), (64, 2048, 512), (256, 8192, 2048) (resident tier) and (8, 100000, 2048)
(streamed tier), median of 20 calls, as time and as microseconds per round (time / K: the rounds of one cloud are serial, the
clouds of a batch run side by side).  Beside it, on the same GPU and the same inputs, the loop a user would otherwise write: K
rounds of torch calls with the same arithmetic and the same tie rule, all clouds of the batch per call; its indices are
compared with the library's.  The baseline lives only here: it is not a product path.

    python tools/cloudsample_time.py [--out profiles/cloudsample_time.json] [--reps 20] [--shapes B,N,K ...]

Every shape runs in a child process of its own under its own time limit (--step-timeout); the first step that fails ends the
run.  SURFD_LIB selects a differently built library (A/B of build variants); the JSON names the library it measured."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 2048, 512), (64, 2048, 512), (256, 8192, 2048), (8, 100000, 2048)]


def clouds(B, n, seed):
    """B ellipsoid shells of n points, seeded"""
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


def torch_fps(x, K):
    """the kernel's loop as torch ops on the whole batch: d = p - p_s per coordinate, d2 = (dx dx + dy dy) + dz dz, minimum,
    then the arg-max with the lower index on ties spelled out (the largest value, then the smallest index that holds it)"""
    import torch
    B, n, _ = x.shape
    px, py, pz = x[..., 0].contiguous(), x[..., 1].contiguous(), x[..., 2].contiguous()
    mind = torch.full((B, n), float("inf"), device=x.device)
    ar = torch.arange(n, device=x.device)[None, :]
    s = torch.zeros(B, 1, dtype=torch.long, device=x.device)
    idx = torch.empty(B, K, dtype=torch.long, device=x.device)
    cover2 = torch.empty(B, K, device=x.device)
    for k in range(K):
        idx[:, k] = s[:, 0]
        dx, dy, dz = px - px.gather(1, s), py - py.gather(1, s), pz - pz.gather(1, s)
        mind = torch.minimum(mind, (dx * dx + dy * dy) + dz * dz)
        best = mind.amax(1, keepdim=True)
        s = torch.where(mind == best, ar, n).amin(1, keepdim=True)
        cover2[:, k] = best[:, 0]
    return idx, cover2


def child(B, n, K, reps):
    import torch
    from surfd_amd import _native as N
    assert torch.cuda.is_available(), "cloudsample_time.py measures on the GPU"
    L = N.lib()
    x = clouds(B, n, 1)
    idx = torch.empty(B, K, device="cuda", dtype=torch.int32)
    cover2 = torch.empty(B, K, device="cuda")
    nbytes = int(L.surfd_cloud_fps_workspace_bytes(B, n))
    work = torch.empty(max(nbytes // 4, 1), device="cuda")

    def call():
        N.check(L.surfd_cloud_fps(N.ptr(x), B, n, None, None, K, N.ptr(idx), N.ptr(cover2), N.ptr(work) if nbytes else None, N.stream()))

    r = {"B": B, "N": n, "K": K, "tier": "resident" if n <= 8192 else "streamed", "workspace_bytes": nbytes}
    r["native_ms"] = timed(call, reps)
    r["native_us_per_round"] = r["native_ms"]["median_ms"] * 1e3 / K
    with torch.no_grad():
        r["torch_ms"] = timed(lambda: torch_fps(x, K), 3, warm=1)
        ref_idx, ref_cover2 = torch_fps(x, K)
    r["torch_us_per_round"] = r["torch_ms"]["median_ms"] * 1e3 / K
    r["torch_indices_equal_share"] = float((ref_idx == idx.long()).double().mean())
    r["torch_cover2_bitwise_equal_share"] = float((ref_cover2.view(torch.int32) == cover2.view(torch.int32)).double().mean())
    r["native_over_torch"] = r["torch_ms"]["median_ms"] / r["native_ms"]["median_ms"]
    print("RESULT " + json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "cloudsample_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--shapes", nargs="*", default=None, metavar="B,N,K", help="shapes to time instead of the four listed above")
    ap.add_argument("--child", type=int, nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.reps)
    rows = []
    for B, n, K in (SHAPES if not a.shapes else [tuple(int(v) for v in sh.split(",")) for sh in a.shapes]):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", str(B), str(n), str(K),
               "--reps", str(a.reps)]
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
