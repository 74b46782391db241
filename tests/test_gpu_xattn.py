"""a19 — the native attention kernels (csrc/xattn.hip: xa_linear_kernel, xa_core_kernel) and the modules on top of them
(surfd_amd/attention.py), pinned against tests/xattn_ref.py, which tests/test_xattn_ref_cpu.py validates on the CPU:

  (a) inputs with an exactly known output (torch.equal): every query selects one key / averages a power-of-two set of keys
  (b) synthetic weights at three logit scales against fp64, per sample, bounded by a multiple of the fp32 oracle's own error
  (c) BasicTransformerBlock / SpatialTransformer against their fp64 restatements
  (d) handle and plumbing: workspace reuse, re-binding, streams, input forms, refusals, stability, batch independence
  (e) more than 65 535 row tiles in the projections

K_RATIO: the kernel and the oracle are two fp32 evaluations of the same sums in different orders, and the maximum runs over
at most 1e5 outputs, so the kernel's error may exceed the oracle's by a small factor but not by an order of magnitude.
Measured on an MI355X (profiles/xattn_error_ratios.json): ratios 0 .. 1.39 over the 47 cases of (b) and (c), so k = 3 stands."""
import ctypes as C
import json
import os

import pytest
import torch

import xattn_ref as R
from oracle import attention as oatt
from surfd_amd import synth

pytestmark = pytest.mark.gpu

K_RATIO = 3.0
FLOOR = 4 * R.U32                      # x max|ref64|: a few roundings of the output itself, for samples where e_ref is ~0
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_report():
    """SURFD_XATTN_RATIOS=<path>: write the per-case error ratios measured by this run (the source of profiles/xattn_error_ratios.json)."""
    yield
    path = os.environ.get("SURFD_XATTN_RATIOS")
    if path and _RATIOS:
        finite = [v["ratio"] for v in _RATIOS.values() if v["ratio"] != float("inf")]
        with open(path, "w") as f:
            json.dump({"bound": "e_gpu[b] <= k * e_ref[b] + 4 * 2^-24 * max|ref64[b]|; ratio = max_b (e_gpu[b] - floor[b])+ / e_ref[b]",
                       "k": K_RATIO, "max_ratio": max(finite) if finite else None, "device": torch.cuda.get_device_name(0),
                       "cases": _RATIOS}, f, indent=1)


def _module(sd, heads):
    from surfd_amd.attention import CrossAttention
    inner, qd = sd["to_q.weight"].shape
    mod = CrossAttention(qd, sd["to_k.weight"].shape[1], heads=heads, dim_head=inner // heads)
    mod.load_state_dict(sd, strict=True)
    return mod.cuda().eval()


def _cu(t):
    return None if t is None else t.cuda()


def _run(mod, x, ctx=None, mask=None):
    return mod(_cu(x), _cu(ctx), _cu(mask)).cpu()


def _check_bound(cid, y, y32, ref, per_sample=True):
    """e_gpu <= K_RATIO * e_ref + FLOOR * max|ref64|, per sample or over the whole output; prints and records the ratio."""
    assert y.dtype == torch.float32 and y.shape == ref.shape
    assert bool(torch.isfinite(y).all()), cid
    if not per_sample:
        y, y32, ref = y[None], y32[None], ref[None]
    e_gpu, e_ref, scale = R.per_sample_max(y.double() - ref), R.per_sample_max(y32.double() - ref), R.per_sample_max(ref)
    excess = (e_gpu - FLOOR * scale).clamp_min(0)
    ratio = max(0.0 if ex == 0 else (float("inf") if er == 0 else ex / er) for ex, er in zip(excess.tolist(), e_ref.tolist()))
    _RATIOS[cid] = {"ratio": ratio, "e_gpu_rel": (e_gpu / scale).tolist(), "e_ref_rel": (e_ref / scale).tolist()}
    print(f"{cid}: ratio {ratio:.3f}  e_gpu/max|ref| {[f'{v:.2e}' for v in (e_gpu / scale).tolist()]}  e_ref/max|ref| {[f'{v:.2e}' for v in (e_ref / scale).tolist()]}")
    ok = e_gpu <= K_RATIO * e_ref + FLOOR * scale
    assert bool(ok.all()), (cid, ratio, e_gpu.tolist(), e_ref.tolist())


# ------------------------------------------------------------------------------------ (a) exact cases
@pytest.mark.parametrize("shape", R.SELECTION_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_selection_exact(shape):
    """ctn = 1..4 output tiles, odd d, d = 1 and 128, n on both sides of 128 and 256, m = 2 .. 256, ragged projections.
    A wrong head offset, fragment row or key block picks another key's values: an integer mismatch, not a rounding error."""
    c = R.selection_case(*shape, seed=sum(shape))
    mod = _module(c["sd"], c["heads"])
    for mask in (None, c["mask"]):
        y = _run(mod, c["x"], c["context"], mask)
        bad = (y != c["expect"]).nonzero()
        assert torch.equal(y, c["expect"]), (shape, mask is not None, bad[:8].tolist(), len(bad))


@pytest.mark.parametrize("shape", R.UNIFORM_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_uniform_exact(shape):
    """All logits 0: the exact mean over the kept keys, which lie scattered over all key blocks (dead blocks, masked tails)."""
    c = R.uniform_case(*shape, seed=sum(shape))
    y = _run(_module(c["sd"], c["heads"]), c["x"], c["context"], c["mask"])
    bad = (y != c["expect"]).nonzero()
    assert torch.equal(y, c["expect"]), (shape, bad[:8].tolist(), len(bad))


# ------------------------------------------------------------------------------------ (b) tolerance cases against fp64
@pytest.mark.parametrize("cid,shp,scale,kind", list(R.tolerance_cases()), ids=[c[0] for c in R.tolerance_cases()])
def test_vs_f64_per_sample(cid, shp, scale, kind):
    """x scaled by 1, 4, 12: from a soft softmax to a nearly one-hot one whose running maximum changes across key blocks;
    masks with a fully masked sample, a dead leading block, a dead block after a live one, and masked ragged tails."""
    sd, heads, x, ctx, mask = R.tolerance_inputs(shp, scale, kind)
    ref = R.cross_attention_f64(sd, heads, x, ctx, mask)
    y32 = oatt.cross_attention(sd, heads, x, ctx, mask)
    _check_bound(cid, _run(_module(sd, heads), x, ctx, mask), y32, ref)


# ------------------------------------------------------------------------------------ (c) wrappers
def _like(mod, seed):
    sd = synth.synth_like({k: tuple(v.shape) for k, v in mod.state_dict().items()}, seed=seed, tag="gpu_xattn")
    mod.load_state_dict(sd, strict=True)
    return sd, mod.cuda().eval()


@pytest.mark.parametrize("dim,heads,dh,ctx_shape", [(96, 3, 32, (40, 20)), (96, 3, 32, None), (130, 2, 65, (40, 20))],
                         ids=["d96-ctx", "d96-self", "d130-ctx"])
def test_basic_transformer_block_vs_f64(dim, heads, dh, ctx_shape):
    from surfd_amd.attention import BasicTransformerBlock
    sd, mod = _like(BasicTransformerBlock(dim, heads, dh, context_dim=ctx_shape[1] if ctx_shape else None), seed=dim + heads)
    g = torch.Generator().manual_seed(dim)
    x = torch.randn(2, 37, dim, generator=g)
    ctx = torch.randn(2, *ctx_shape, generator=g) if ctx_shape else None
    y = mod(x.cuda(), context=_cu(ctx)).cpu()
    _check_bound(f"block-{dim}-{'ctx' if ctx_shape else 'self'}", y, R.basic_transformer_block_f32(sd, heads, x, ctx),
                 R.basic_transformer_block_f64(sd, heads, x, ctx), per_sample=False)


@pytest.mark.parametrize("depth,ctx_shape", [(2, (9, 20)), (1, None)], ids=["depth2-ctx", "depth1-self"])
def test_spatial_transformer_vs_f64(depth, ctx_shape):
    """Non-square map (h, w = 5, 7), proj_out with non-zero weights (zero-initialised, the output would be the input)."""
    from surfd_amd.attention import SpatialTransformer
    heads, dh = 2, 24
    sd, mod = _like(SpatialTransformer(64, heads, dh, depth=depth, context_dim=ctx_shape[1] if ctx_shape else None), seed=depth)
    assert float(sd["proj_out.weight"].abs().max()) > 0
    g = torch.Generator().manual_seed(depth)
    x = torch.randn(2, 64, 5, 7, generator=g)
    ctx = torch.randn(2, *ctx_shape, generator=g) if ctx_shape else None
    y = mod(x.cuda(), context=_cu(ctx)).cpu()
    ref = R.spatial_transformer_f64(sd, heads, x, ctx)
    assert float((ref - x.double()).abs().max()) > 0.1          # the blocks do contribute
    _check_bound(f"spatial-depth{depth}", y, R.spatial_transformer_f32(sd, heads, x, ctx), ref, per_sample=False)


# ------------------------------------------------------------------------------------ (d) handle and plumbing (bitwise)
QD, CD, HEADS, DH = 33, 17, 1, 65       # tolerance shape 3: nothing a multiple of a tile


def _sd(seed=40):
    return synth.synth_cross_attention_state_dict(QD, CD, HEADS, DH, seed=seed)


def _inputs(b, n, m, seed=0, qd=QD, cd=CD):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(b, n, qd, generator=g).cuda(), torch.randn(b, m, cd, generator=g).cuda(), (torch.rand(b, m, generator=g) > 0.3).cuda()


def _fresh(x, ctx=None, mask=None, sd=None):
    """The same call on a module (and native handle) of its own, default stream."""
    return _module(sd or _sd(), HEADS)(x, ctx, mask)


def test_workspace_grows_and_is_reused():
    mod = _module(_sd(), HEADS)
    for i, (b, n, m) in enumerate([(1, 40, 33), (2, 130, 97), (1, 40, 33)]):          # small, large, small again
        x, ctx, mask = _inputs(b, n, m, seed=i)
        assert torch.equal(mod(x, ctx, mask), _fresh(x, ctx, mask)), (i, b, n, m)


def test_rebinds_after_weight_updates():
    x, ctx, mask = _inputs(2, 40, 33)
    mod = _module(_sd(), HEADS)
    y0 = mod(x, ctx, mask)
    with torch.no_grad():
        mod.to_q.weight.mul_(2)
    sd2 = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    assert torch.equal(sd2["to_q.weight"], _sd()["to_q.weight"] * 2)
    y1 = mod(x, ctx, mask)
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, _fresh(x, ctx, mask, sd=sd2))
    mod.load_state_dict(_sd(seed=41), strict=True)
    y2 = mod(x, ctx, mask)
    assert not torch.equal(y2, y1)
    assert torch.equal(y2, _fresh(x, ctx, mask, sd=_sd(seed=41)))


def test_side_stream():
    x, ctx, mask = _inputs(2, 130, 97)
    want = _fresh(x, ctx, mask)
    mod = _module(_sd(), HEADS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = mod(x, ctx, mask)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(y, want)


def test_input_forms():
    mod = _module(_sd(), HEADS)
    x, ctx, mask = _inputs(2, 40, 65)
    want = _fresh(x, ctx, mask)
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)                              # same values, strides of [b, c, n]
    assert not xt.is_contiguous() and torch.equal(xt, x)
    assert torch.equal(mod(xt, ctx, mask), want)
    xh, ch = x.half(), ctx.half()
    yh = mod(xh, ch, mask)
    assert yh.dtype == torch.float32 and torch.equal(yh, _fresh(xh.float(), ch.float(), mask))
    assert torch.equal(mod(x, ctx, mask.reshape(2, 5, 13)), want)                    # 'b ... -> b (...)'
    assert torch.equal(mod(x, ctx, mask.reshape(2, 5, 13).float()), want)            # any dtype, non-zero = attend


def test_refusals():
    from surfd_amd.attention import CrossAttention
    mod = _module(_sd(), HEADS)
    x, ctx, mask = _inputs(2, 40, 65)
    with pytest.raises(ValueError):
        mod(x, ctx, mask[:, :64])
    with pytest.raises(ValueError):
        mod(x, ctx, torch.ones(2, 5, 14, dtype=torch.bool).cuda())
    with pytest.raises(RuntimeError, match="context_dim == query_dim"):
        mod(x)                                                                        # no context, context_dim 17 != query_dim 33
    assert torch.equal(mod(x, ctx, mask), _fresh(x, ctx, mask))                       # the handle is still good
    # more token rows than one launch can cover: refused from the sizes alone, before anything is allocated or read
    from surfd_amd import _native as N
    one = CrossAttention(1, 1, heads=1, dim_head=1).cuda().eval()
    L, h = one._native()
    t = torch.zeros(4, device="cuda")
    rc = L.surfd_xattn_forward(h, C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr()), None, C.c_void_p(t.data_ptr()), 32768, 32769, 1, N.stream())
    assert rc != 0 and b"token rows" in L.surfd_last_error()


def test_bit_stable_run_to_run():
    mod = _module(_sd(), HEADS)
    x, ctx, mask = _inputs(2, 130, 97)
    first = mod(x, ctx, mask)
    for _ in range(19):
        assert torch.equal(mod(x, ctx, mask), first)


def test_batch_independent():
    """n = 40: the 64-row tiles of the projections straddle the samples of the batch."""
    mod = _module(_sd(), HEADS)
    x, ctx, mask = _inputs(3, 40, 33)
    y = mod(x, ctx, mask)
    for b in range(3):
        assert torch.equal(mod(x[b:b + 1], ctx[b:b + 1], mask[b:b + 1]), y[b:b + 1]), b


# ------------------------------------------------------------------------------------ (e) many rows
def test_more_than_65535_row_tiles():
    """b * n = 65 535 * 64 + 1 rows: one row tile more than a grid's y dimension holds (the row tiles ride on grid.x).
    One key, so the softmax is 1 whatever the query: every row is v * wo + b exactly."""
    n = 65535 * 64 + 1
    sd = {"to_q.weight": torch.tensor([[3.0]]), "to_k.weight": torch.tensor([[2.0]]), "to_v.weight": torch.tensor([[-5.0]]),
          "to_out.0.weight": torch.tensor([[7.0]]), "to_out.0.bias": torch.tensor([11.0])}
    x = torch.randint(-3, 4, (1, n, 1), generator=torch.Generator().manual_seed(0)).float().cuda()
    ctx = torch.tensor([[[3.0]]]).cuda()
    y = _module(sd, 1)(x, ctx)
    assert y.shape == (1, n, 1)
    want = 3.0 * -5.0 * 7.0 + 11.0
    bad = (y != want).nonzero()
    assert len(bad) == 0, (len(bad), bad[:4].tolist(), bad[-4:].tolist())
