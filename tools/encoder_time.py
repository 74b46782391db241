#!/usr/bin/env python3
"""Device-event timing of the point-cloud encoder (surfd_amd.dgcnn) after warm-up: Dgcnn.forward and knn_points alone at
B in {1, 8}, N = 10 000, size_latent in {32, 64}; beside it, a pure-torch restatement on the GPU (cdist + topk, gather,
Linear) as the comparison baseline.  The baseline lives only here: it is not a product path.

    python tools/encoder_time.py [--out profiles/encoder_time.json] [--reps 20]

Per-kernel times: run the same command under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from surfd_amd import synth  # noqa: E402
from surfd_amd.dgcnn import Dgcnn, knn_points  # noqa: E402


def cloud(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, N, 3, generator=g)
    v = v / v.norm(dim=-1, keepdim=True) * torch.tensor([0.6, 0.4, 0.5])
    return (v + torch.randn(B, N, 3, generator=g) * 0.01).float().cuda()


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def torch_knn(x, k):
    d = torch.cdist(x, x) ** 2
    return torch.topk(d, k, dim=-1, largest=False)


def torch_dgcnn(sd, x, k=20):
    """the reference's arithmetic restated in torch (per-edge Linear on the B x N x K x 2D tensor), eval-mode BN"""
    _, idx = torch_knn(x, k)
    bidx = torch.arange(x.shape[0], device=x.device)[:, None, None]
    feats, f = [], x
    for i in range(1, 5):
        nb = f[bidx, idx]
        ctr = f[:, :, None, :].expand_as(nb)
        e = F.linear(torch.cat((nb - ctr, ctr), -1), sd[f"conv_{i}.weight"])
        e = F.batch_norm(e.reshape(-1, e.shape[-1]), sd[f"bn_{i}.running_mean"], sd[f"bn_{i}.running_var"], sd[f"bn_{i}.weight"],
                         sd[f"bn_{i}.bias"], False, 0.0, 1e-5).reshape(e.shape)
        f = F.leaky_relu(e, 0.2).max(2).values
        feats.append(f)
    x5 = F.linear(torch.cat(feats, -1), sd["conv_5.weight"])
    x5 = F.batch_norm(x5.reshape(-1, x5.shape[-1]), sd["bn_5.running_mean"], sd["bn_5.running_var"], sd["bn_5.weight"], sd["bn_5.bias"],
                      False, 0.0, 1e-5).reshape(x5.shape)
    return F.leaky_relu(x5, 0.2).max(1).values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "encoder_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "encoder_time.py measures on the GPU"
    rows = []
    N = 10000
    for B in (1, 8):
        x = cloud(B, N, B)
        r = {"B": B, "N": N, "knn_ms": timed(lambda: knn_points(x, 20), a.reps)}
        if not a.no_baseline:
            r["torch_knn_ms"] = timed(lambda: torch_knn(x, 20), a.reps)
        for L in (32, 64):
            sd = synth.synth_dgcnn_state_dict(L, seed=0)
            m = Dgcnn(L)
            m.load_state_dict(sd, strict=True)
            m = m.cuda().eval()
            r[f"dgcnn_L{L}_ms"] = timed(lambda: m(x), a.reps)
            if not a.no_baseline:
                sdc = {k: v.cuda() for k, v in sd.items()}
                with torch.no_grad():
                    r[f"torch_dgcnn_L{L}_ms"] = timed(lambda: torch_dgcnn(sdc, x), max(3, a.reps // 4))
                    r[f"torch_dgcnn_L{L}_max_abs_diff"] = float((torch_dgcnn(sdc, x) - m(x)).abs().max())
        rows.append(r)
        print(json.dumps(r), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "k": 20, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
