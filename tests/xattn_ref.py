"""TEST INFRASTRUCTURE — fp64 restatement of the a19 attention stack (CrossAttention, BasicTransformerBlock, SpatialTransformer:
reference modules/attention.py:37-64, 152-261) as functions of a state dict, written out with elementary tensor ops and
independent of oracle/attention.py, plus builders of inputs whose output is known exactly (small integers in fp32, so that
every sum is an integer below 2^24 in any summation order).  No GPU, never imported by the product path.

The *_f32 functions restate the two wrappers in fp32 with library ops around the fp32 oracle: they only measure how far a
plain fp32 evaluation lies from fp64 (the `e_ref` of the GPU tests' bound), they judge nothing by themselves."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

U32 = 2.0 ** -24                       # unit roundoff of fp32
F64 = torch.float64


# ------------------------------------------------------------------------------------ fp64 reference
def _d(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else t.detach().to("cpu", F64)


def _sub(sd: Dict[str, Tensor], prefix: str) -> Dict[str, Tensor]:
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def attention_logits_f64(sd, heads: int, x: Tensor, context: Optional[Tensor] = None) -> Tensor:
    """Unmasked logits [b, heads, n, m] in fp64 (the tests use them to report how peaked a case is)."""
    x = _d(x)
    ctx = x if context is None else _d(context)
    q = torch.einsum("bnc,ic->bni", x, _d(sd["to_q.weight"]))
    k = torch.einsum("bmc,ic->bmi", ctx, _d(sd["to_k.weight"]))
    b, n, inner = q.shape
    d = inner // heads
    q = q.reshape(b, n, heads, d)
    k = k.reshape(b, k.shape[1], heads, d)
    return torch.einsum("bnhd,bmhd->bhnm", q, k) / math.sqrt(d)


def cross_attention_f64(sd, heads: int, x: Tensor, context: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> Tensor:
    """x [b,n,cq], context [b,m,cc] (None: x), mask [b, ...] flattening to [b,m], non-zero = attend (None: all) -> [b,n,cq], fp64."""
    x = _d(x)
    ctx = x if context is None else _d(context)
    sim = attention_logits_f64(sd, heads, x, ctx)
    b, h, n, m = sim.shape
    d = sd["to_q.weight"].shape[0] // heads
    if mask is not None:
        keep = mask.detach().cpu().reshape(b, -1).ne(0)
        assert keep.shape[1] == m
        # the reference fills with -finfo(dtype).max, not -inf: a sample with no key left attends to all of them equally
        sim = torch.where(keep[:, None, None, :], sim, torch.full_like(sim, -torch.finfo(F64).max))
    e = torch.exp(sim - sim.amax(dim=-1, keepdim=True))
    p = e / e.sum(dim=-1, keepdim=True)
    v = torch.einsum("bmc,ic->bmi", ctx, _d(sd["to_v.weight"])).reshape(b, m, heads, d)
    o = torch.einsum("bhnm,bmhd->bnhd", p, v).reshape(b, n, heads * d)
    return torch.einsum("bni,ci->bnc", o, _d(sd["to_out.0.weight"])) + _d(sd["to_out.0.bias"])


def _layer_norm_f64(x: Tensor, w: Tensor, b: Tensor, eps: float = 1e-5) -> Tensor:
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * _d(w) + _d(b)


def _gelu_f64(x: Tensor) -> Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def basic_transformer_block_f64(sd, heads: int, x: Tensor, context: Optional[Tensor] = None) -> Tensor:
    """Pre-norm self-attention, cross-attention (self when context is None) and GEGLU feed-forward, each with a residual."""
    x = _d(x)
    x = cross_attention_f64(_sub(sd, "attn1."), heads, _layer_norm_f64(x, sd["norm1.weight"], sd["norm1.bias"])) + x
    x = cross_attention_f64(_sub(sd, "attn2."), heads, _layer_norm_f64(x, sd["norm2.weight"], sd["norm2.bias"]), context) + x
    y = _layer_norm_f64(x, sd["norm3.weight"], sd["norm3.bias"])
    y = torch.einsum("bnc,oc->bno", y, _d(sd["ff.net.0.proj.weight"])) + _d(sd["ff.net.0.proj.bias"])
    half = y.shape[-1] // 2
    y = y[..., :half] * _gelu_f64(y[..., half:])
    return torch.einsum("bni,ci->bnc", y, _d(sd["ff.net.2.weight"])) + _d(sd["ff.net.2.bias"]) + x


def _depth(sd) -> int:
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("transformer_blocks."))


def spatial_transformer_f64(sd, heads: int, x: Tensor, context: Optional[Tensor] = None) -> Tensor:
    """GroupNorm(32, eps 1e-6) -> 1x1 conv -> tokens [b, h*w, c] -> blocks -> map -> 1x1 conv -> + input; x [b,c,h,w]."""
    x = _d(x)
    b, c, h, w = x.shape
    g = x.reshape(b, 32, -1)
    mu = g.mean(dim=-1, keepdim=True)
    var = ((g - mu) ** 2).mean(dim=-1, keepdim=True)
    t = ((g - mu) / torch.sqrt(var + 1e-6)).reshape(b, c, h * w)
    t = t * _d(sd["norm.weight"])[None, :, None] + _d(sd["norm.bias"])[None, :, None]
    w_in = _d(sd["proj_in.weight"]).reshape(-1, c)
    t = torch.einsum("bcp,ic->bpi", t, w_in) + _d(sd["proj_in.bias"])                      # b (h w) inner
    for i in range(_depth(sd)):
        t = basic_transformer_block_f64(_sub(sd, f"transformer_blocks.{i}."), heads, t, context)
    w_out = _d(sd["proj_out.weight"]).reshape(c, -1)
    y = torch.einsum("bpi,ci->bcp", t, w_out) + _d(sd["proj_out.bias"])[None, :, None]
    return y.reshape(b, c, h, w) + x


# ------------------------------------------------------------------------------------ plain fp32 evaluations (for e_ref only)
def basic_transformer_block_f32(sd, heads: int, x: Tensor, context: Optional[Tensor] = None) -> Tensor:
    from oracle.attention import cross_attention
    F = torch.nn.functional
    dim = x.shape[-1]
    x = cross_attention(_sub(sd, "attn1."), heads, F.layer_norm(x, (dim,), sd["norm1.weight"], sd["norm1.bias"])) + x
    x = cross_attention(_sub(sd, "attn2."), heads, F.layer_norm(x, (dim,), sd["norm2.weight"], sd["norm2.bias"]), context) + x
    a, g = F.linear(F.layer_norm(x, (dim,), sd["norm3.weight"], sd["norm3.bias"]), sd["ff.net.0.proj.weight"], sd["ff.net.0.proj.bias"]).chunk(2, dim=-1)
    return F.linear(a * F.gelu(g), sd["ff.net.2.weight"], sd["ff.net.2.bias"]) + x


def spatial_transformer_f32(sd, heads: int, x: Tensor, context: Optional[Tensor] = None) -> Tensor:
    F = torch.nn.functional
    b, c, h, w = x.shape
    t = F.conv2d(F.group_norm(x, 32, sd["norm.weight"], sd["norm.bias"], eps=1e-6), sd["proj_in.weight"], sd["proj_in.bias"])
    t = t.flatten(2).transpose(1, 2)
    for i in range(_depth(sd)):
        t = basic_transformer_block_f32(_sub(sd, f"transformer_blocks.{i}."), heads, t, context)
    t = t.transpose(1, 2).reshape(b, -1, h, w)
    return F.conv2d(t, sd["proj_out.weight"], sd["proj_out.bias"]) + x


# ------------------------------------------------------------------------------------ cases with an exactly known output
def _ints(g: torch.Generator, shape, lo: int, hi: int) -> Tensor:
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def _expected(v: Tensor, wo: Tensor, bias: Tensor) -> Tensor:
    """v [b, n, inner] int64 (the attended values), integer out-projection -> fp32 of the exact int64 result."""
    out = torch.einsum("bni,ci->bnc", v, wo) + bias
    assert int(out.abs().max()) < 2 ** 24 and int(v.abs().max()) < 2 ** 24
    return out.to(torch.float32)


def selection_case(b: int, n: int, m: int, heads: int, d: int, qd: int, cd: int, seed: int = 0) -> dict:
    """Every (sample, head, query) attends to exactly one key drawn at random: each key carries a distinct +-1 code in its
    first d context features, to_k copies the code into every head, the query holds 2048 x the code of its pick, so the
    pick leads every other logit by >= 2 * 2048 / sqrt(d) >= 362 and all other probabilities are exactly 0 in fp32.
    The picks of a sample are drawn from a random half of its keys, so the other half is never picked.
    Returns sd, x, context, mask (switches off exactly the keys that no query of the sample picked; must not change the
    result), expect (fp32 of gather(v, pick) Wo^T + b evaluated in int64) and pick [b, heads, n]."""
    inner = heads * d
    nb = min(d, 12)
    assert qd >= inner and cd >= d and m <= 2 ** nb
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(2 ** nb, generator=g)[:m] for _ in range(b)])              # [b, m] distinct per sample
    code = torch.ones(b, m, d, dtype=torch.int64)
    code[..., :nb] = 2 * ((ids[..., None] >> torch.arange(nb)) & 1) - 1
    context = _ints(g, (b, m, cd), -3, 3)
    context[..., :d] = code
    live = torch.stack([torch.randperm(m, generator=g)[:(m + 1) // 2] for _ in range(b)])        # half the keys are never picked
    pick = torch.gather(live[:, None].expand(b, heads, -1), 2, _ints(g, (b, heads, n), 0, live.shape[1] - 1))
    x = _ints(g, (b, n, qd), -3, 3)
    x[..., :inner] = torch.gather(code[:, None].expand(b, heads, m, d), 2, pick[..., None].expand(b, heads, n, d)) \
        .permute(0, 2, 1, 3).reshape(b, n, inner)
    wq = torch.zeros(inner, qd, dtype=torch.int64)
    wq[:, :inner] = 2048 * torch.eye(inner, dtype=torch.int64)
    wk = torch.zeros(inner, cd, dtype=torch.int64)
    for h in range(heads):
        wk[h * d:(h + 1) * d, :d] = torch.eye(d, dtype=torch.int64)
    wv, wo, bias = _ints(g, (inner, cd), -4, 4), _ints(g, (qd, inner), -4, 4), _ints(g, (qd,), -8, 8)
    v = torch.einsum("bmc,ic->bmi", context, wv).reshape(b, m, heads, d)
    got = torch.gather(v.permute(0, 2, 1, 3), 2, pick[..., None].expand(b, heads, n, d))         # [b, heads, n, d]
    mask = torch.zeros(b, m, dtype=torch.bool)
    mask.scatter_(1, pick.reshape(b, -1), True)
    f = lambda t: t.to(torch.float32)
    sd = {"to_q.weight": f(wq), "to_k.weight": f(wk), "to_v.weight": f(wv), "to_out.0.weight": f(wo), "to_out.0.bias": f(bias)}
    return {"sd": sd, "heads": heads, "x": f(x), "context": f(context), "mask": mask, "pick": pick,
            "expect": _expected(got.permute(0, 2, 1, 3).reshape(b, n, inner), wo, bias)}


def uniform_case(b: int, n: int, m: int, keep: int, heads: int, d: int, qd: int, cd: int, seed: int = 0) -> dict:
    """to_q = 0: every logit is 0 and each query averages the values of the `keep` keys (a power of two, scattered over
    [0, m), drawn per sample) that the mask leaves on; to_v holds multiples of `keep`, so v / keep is an integer and
    the average is exact in any order.  mask is None when keep == m."""
    assert keep & (keep - 1) == 0 and 1 <= keep <= m
    inner = heads * d
    g = torch.Generator().manual_seed(seed)
    context = _ints(g, (b, m, cd), -3, 3)
    x = _ints(g, (b, n, qd), -3, 3)
    wv, wo, bias = keep * _ints(g, (inner, cd), -4, 4), _ints(g, (qd, inner), -4, 4), _ints(g, (qd,), -8, 8)
    kept = torch.stack([torch.randperm(m, generator=g)[:keep] for _ in range(b)])
    mask = torch.zeros(b, m, dtype=torch.bool)
    mask.scatter_(1, kept, True)
    v = torch.einsum("bmc,ic->bmi", context, wv)
    tot = (v * mask[..., None]).sum(dim=1)                                                       # [b, inner]
    assert int(tot.abs().max()) < 2 ** 24 and bool((tot % keep == 0).all())
    f = lambda t: t.to(torch.float32)
    sd = {"to_q.weight": torch.zeros(inner, qd), "to_k.weight": f(_ints(g, (inner, cd), -4, 4)), "to_v.weight": f(wv),
          "to_out.0.weight": f(wo), "to_out.0.bias": f(bias)}
    return {"sd": sd, "heads": heads, "x": f(x), "context": f(context), "mask": None if keep == m else mask,
            "expect": _expected((tot // keep)[:, None, :].expand(b, n, inner), wo, bias)}


# ------------------------------------------------------------------------------------ the case tables of the GPU tests
SELECTION_SHAPES = [   # b, n, m, heads, d, qd, cd
    (2, 130, 97, 3, 96, 300, 100), (2, 129, 65, 2, 128, 260, 130), (1, 40, 33, 1, 65, 70, 66), (3, 7, 2, 4, 1, 5, 3),
    (2, 64, 256, 3, 32, 96, 40), (1, 257, 160, 2, 127, 254, 127), (2, 33, 129, 4, 16, 64, 48)]
# b, n, m, keep, heads, d, qd, cd: n crosses one 128-query block at d = 96, query / context widths no multiple of 32
UNIFORM_SHAPES = [(2, 37 if d == 28 else 130, m, keep, 2, d, 11, 5) for (m, keep) in ((64, 64), (97, 64), (129, 32), (33, 1)) for d in (28, 96)]
TOLERANCE_SHAPES = [   # b, n, m, qd, cd (None: self-attention), heads, dh
    (2, 130, 97, 72, 40, 3, 96), (2, 129, 65, 50, 50, 2, 128), (1, 40, 33, 33, 17, 1, 65), (3, 7, 31, 24, 9, 4, 1),
    (2, 64, 64, 96, None, 3, 32), (1, 257, 160, 36, 20, 2, 127)]
X_SCALES = (1, 4, 12)
MASKS = ("none", "mixed", "dead_mid")


def tolerance_mask(kind: str, b: int, m: int, g: torch.Generator) -> Optional[Tensor]:
    """none | mixed: rand > 0.25, sample 0 fully masked, a dead leading 32-key block in the last sample where m > 40 |
    dead_mid: keys [32, 64) of the last sample masked, a dead block after a live one (needs m >= 64)."""
    if kind == "none":
        return None
    if kind == "mixed":
        mask = torch.rand(b, m, generator=g) > 0.25
        mask[0] = False
        if m > 40:
            mask[-1, :32] = False
        return mask
    assert kind == "dead_mid" and m >= 64
    mask = torch.ones(b, m, dtype=torch.bool)
    mask[-1, 32:64] = False
    return mask


def tolerance_cases():
    """Yields (id, shape tuple, x scale, mask kind) for every tolerance case: each shape at every scale, unmasked and with
    the mixed mask, and the two shapes with m >= 64 and a ragged tail also with the dead middle block."""
    for i, shp in enumerate(TOLERANCE_SHAPES):
        for sc in X_SCALES:
            for kind in MASKS:
                if kind == "dead_mid" and i not in (0, 5):
                    continue
                yield f"s{i}-x{sc}-{kind}", shp, sc, kind


def tolerance_inputs(shp, scale: int, kind: str):
    """sd, heads, x, context, mask of one tolerance case (weights of synth_cross_attention_state_dict, seeded inputs)."""
    from surfd_amd import synth
    b, n, m, qd, cd, heads, dh = shp
    sd = synth.synth_cross_attention_state_dict(qd, cd or qd, heads, dh, seed=n)
    g = torch.Generator().manual_seed(n * 7 + m)
    x = torch.randn(b, n, qd, generator=g) * scale
    ctx = None if cd is None else torch.randn(b, m, cd, generator=g)
    return sd, heads, x, ctx, tolerance_mask(kind, b, m if cd is not None else n, g)


def per_sample_max(t: Tensor) -> Tensor:
    return t.abs().reshape(t.shape[0], -1).amax(dim=1)
