"""csrc/meshclean.hip on the GPU against surfd_amd.meshproc: vertices and faces bit for bit and in the same
order, no tolerance anywhere.  The shapes are the smallest at which each rule can go wrong (meshclean_ref.shapes); the stats of
clean_until_stable are compared with the sequential restatement, which tests/test_meshclean_cpu.py pins to meshproc.

The second half runs the meshes at size (meshclean_ref.big_shapes: classes of a merge that lie tens of thousands of indices apart,
negative keys, a long run of vertices that take no part, duplicates among 18 661 faces), the hole pass at every width of its sort
key, the loops in every rotation, 400 random soups, and the C ABI itself with sentinels behind its outputs."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshclean_ref as R  # noqa: E402

from surfd_amd import meshproc as mp  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = R.shapes()
NAMES = sorted(SHAPES)
BIG = R.big_shapes()
MESHES = {**SHAPES, **BIG}


def cu(x, dtype=None):
    t = torch.from_numpy(np.array(x))                         # a copy: the shared references are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def same_v(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), f"{int((got.view(np.int64) != want.view(np.int64)).sum())} entries differ"


def same_f(got, want):
    assert got.dtype == torch.int64 and got.is_cuda
    want = torch.from_numpy(np.array(want).reshape(-1, 3))
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert torch.equal(got.cpu(), want), f"{int((got.cpu() != want).any(dim=1).sum())} faces differ"


def host_of(v, f):
    """host() of a mesh that has no name"""
    with np.errstate(all="ignore"):
        v1, f0 = mp.cull_and_merge(v, f)
        fd = mp.drop_duplicate_faces(f0)
        fg = mp.drop_degenerate_faces(v1, fd)
        fh = mp.fill_small_holes(v1, fg)
        cv, cf = mp.clean_until_stable(v, f)
        raw = (mp.drop_duplicate_faces(f), mp.drop_degenerate_faces(v, f), mp.fill_small_holes(v, f))
    return dict(v1=v1, f0=f0, fd=fd, fg=fg, fh=fh, cv=cv, cf=cf, raw=raw, stats=R.clean_until_stable(v, f)[2])


@functools.lru_cache(maxsize=None)
def host(name):
    """meshproc's own chain on a fixture, worked out once and shared (callers do not write to it): the cull, then the duplicate
    pass, the height test and the caps, each on the result before it; and the whole clean_until_stable with the restatement's stats"""
    out = host_of(*MESHES[name])
    for a in [out[k] for k in ("v1", "f0", "fd", "fg", "fh", "cv", "cf")] + list(out["raw"]):
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_cull_and_merge(name):
    from surfd_amd import meshclean as MC
    v, f = SHAPES[name]
    gv, gf = MC.cull_and_merge(cu(v), cu(f))
    same_v(gv, host(name)["v1"]); same_f(gf, host(name)["f0"])


@pytest.mark.parametrize("name", NAMES)
def test_drop_duplicate_faces(name):
    from surfd_amd import meshclean as MC
    h = host(name)
    same_f(MC.drop_duplicate_faces(cu(h["f0"])), h["fd"])
    same_f(MC.drop_duplicate_faces(cu(SHAPES[name][1])), h["raw"][0])


@pytest.mark.parametrize("name", NAMES)
def test_drop_degenerate_faces(name):
    from surfd_amd import meshclean as MC
    h = host(name)
    same_f(MC.drop_degenerate_faces(cu(h["v1"]), cu(h["fd"])), h["fg"])
    v, f = SHAPES[name]                                      # the raw mesh: NaN coordinates, repeated indices, coincident vertices
    same_f(MC.drop_degenerate_faces(cu(v), cu(f)), h["raw"][1])


@pytest.mark.parametrize("name", NAMES)
def test_fill_small_holes(name):
    from surfd_amd import meshclean as MC
    h = host(name)
    same_f(MC.fill_small_holes(cu(h["v1"]), cu(h["fg"])), h["fh"])
    v, f = SHAPES[name]
    same_f(MC.fill_small_holes(cu(v), cu(f)), h["raw"][2])


@pytest.mark.parametrize("name", NAMES)
def test_clean_until_stable(name):
    from surfd_amd import meshclean as MC
    v, f = SHAPES[name]
    h = host(name)
    gv, gf, st = MC.clean_until_stable(cu(v), cu(f), return_stats=True)
    same_v(gv, h["cv"]); same_f(gf, h["cf"])
    assert st == h["stats"], (st, h["stats"])
    gv, gf = MC.clean_until_stable(cu(v), cu(f, torch.int32))
    same_v(gv, h["cv"]); same_f(gf, h["cf"])


def test_heights_on_random_triangles():
    """the height test on triangles of every scale down to its thresholds, slivers among them: the same faces as meshproc keeps"""
    from surfd_amd import meshclean as MC
    rng = np.random.default_rng(11)
    v = rng.standard_normal((3000, 3)) * 10.0 ** rng.integers(-9, 3, size=(3000, 1))
    f = rng.integers(0, len(v), size=(4000, 3))
    thin = np.arange(0, 3000 - 3, 3)
    v[thin + 2] = v[thin] + (v[thin + 1] - v[thin]) * rng.random((len(thin), 1)) + rng.standard_normal((len(thin), 3)) * 1e-8
    f = np.vstack([f, np.stack([thin, thin + 1, thin + 2], axis=1)])
    want = mp.drop_degenerate_faces(v, f)
    assert 0 < len(want) < len(f)
    same_f(MC.drop_degenerate_faces(cu(v), cu(f)), want)


def test_repeated_runs_are_bit_identical():
    from surfd_amd import meshclean as MC
    v, f = cu(SHAPES["sheet64"][0]), cu(SHAPES["sheet64"][1])
    v0, f0 = MC.clean_until_stable(v, f)
    for _ in range(9):
        v1, f1 = MC.clean_until_stable(v, f)
        assert torch.equal(f0, f1) and torch.equal(v0.view(torch.int64), v1.view(torch.int64))


@pytest.mark.parametrize("name", ["soup", "octahedron_minus_one"])
def test_float32_input_is_widened_exactly(name):
    from surfd_amd import meshclean as MC
    v, f = SHAPES[name]
    v32 = v.astype(np.float32)
    with np.errstate(all="ignore"):
        wv, wf = mp.clean_until_stable(v32, f)               # np.asarray(..., float64) of the float32 array
    gv, gf = MC.clean_until_stable(cu(v32), cu(f))
    same_v(gv, wv); same_f(gf, wf)
    gv64, gf64 = MC.clean_until_stable(cu(v32).double(), cu(f))
    assert torch.equal(gf, gf64) and torch.equal(gv.view(torch.int64), gv64.view(torch.int64))


@pytest.mark.parametrize("top", [2 ** 20 - 3, 2 ** 20 - 2, 2 ** 20 - 1, 2 ** 20, 2 ** 21 - 1, 2 ** 21 + 5])
def test_duplicate_order_across_the_packing_boundary(top):
    """meshproc._pack_rows changes its method where an index reaches 2^20 - 1; the order does not, here or there"""
    from surfd_amd import meshclean as MC
    f = np.array([[top, 3, 7], [7, top, 3], [2, top - 1, top], [top, top - 1, 2], [0, 1, 2], [top - 1, 5, 6], [5, 6, top - 1], [1, 0, 2]], dtype=np.int64)
    want = mp.drop_duplicate_faces(f)
    assert len(want) == 4
    same_f(MC.drop_duplicate_faces(cu(f)), want)


def test_refusals():
    from surfd_amd import meshclean as MC
    v, f = SHAPES["octahedron_minus_one"]
    dv, df = cu(v), cu(f)
    calls = [lambda v, f: MC.cull_and_merge(v, f), lambda v, f: MC.drop_degenerate_faces(v, f), lambda v, f: MC.fill_small_holes(v, f),
             lambda v, f: MC.clean_until_stable(v, f)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(torch.from_numpy(v), torch.from_numpy(f))
        with pytest.raises(ValueError):
            call(dv[:, :2], df)
        with pytest.raises(ValueError):
            call(dv, df.reshape(-1))
        with pytest.raises(TypeError):
            call(dv.half(), df)
        with pytest.raises(TypeError):
            call(dv, df.float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MC.drop_duplicate_faces(torch.from_numpy(f))
    with pytest.raises(ValueError):
        MC.drop_duplicate_faces(df[:, :2])
    with pytest.raises(TypeError):
        MC.drop_duplicate_faces(df.double())
    # an index outside [0, V): the library's SURFD_ERR_ARG (-1), raised and not a fault; the device still answers afterwards
    for bad_index in (len(v), -1, 2 ** 31 - 1):
        bad = f.copy(); bad[3, 1] = bad_index
        for call in calls:
            with pytest.raises(RuntimeError, match=r"libsurfd_hip error -1:.*outside \[0, 6\)"):
                call(dv, cu(bad))
    with pytest.raises(RuntimeError, match="libsurfd_hip error -1:.*negative"):
        MC.drop_duplicate_faces(cu(np.array([[0, 1, 2], [0, -1, 2], [2, 1, 0]])))
    # a finite coordinate beyond the 64-bit keys, whether or not a face names the vertex
    for row in (1, 5):
        far = v.copy(); far[row, 2] = -2.0 ** 62 / 1e8
        with pytest.raises(RuntimeError, match="libsurfd_hip error -1:.*2\\^62"):
            MC.cull_and_merge(cu(far), cu(f[:3] if row == 5 else f))          # f[:3] names the vertices 0 - 4 only
    far = v.copy(); far[1, 2] = 2.0 ** 61 / 1e8
    gv, gf = MC.cull_and_merge(cu(far), df)
    wv, wf = mp.cull_and_merge(far, f)
    same_v(gv, wv); same_f(gf, wf)
    gv, gf = MC.clean_until_stable(dv, df)
    same_f(gf, host("octahedron_minus_one")["cf"])


def test_empty_meshes():
    from surfd_amd import meshclean as MC
    v, f = SHAPES["tetrahedron"]
    no_v, no_f = cu(np.zeros((0, 3))), cu(np.zeros((0, 3), dtype=np.int64))
    for dv, df in ((no_v, no_f), (cu(v), no_f), (no_v, cu(f))):
        gv, gf = MC.cull_and_merge(dv, df)
        assert tuple(gv.shape) == (0, 3) and tuple(gf.shape) == (0, 3) and gv.dtype == torch.float64 and gf.dtype == torch.int64
        gv, gf, st = MC.clean_until_stable(dv, df, return_stats=True)
        assert tuple(gv.shape) == (0, 3) and tuple(gf.shape) == (0, 3) and st["rounds"] == 1
    assert tuple(MC.drop_duplicate_faces(no_f).shape) == (0, 3)
    assert tuple(MC.drop_degenerate_faces(cu(v), no_f).shape) == (0, 3)
    assert tuple(MC.fill_small_holes(cu(v), no_f).shape) == (0, 3)
    same_f(MC.fill_small_holes(cu(v), cu(f[:2])), f[:2])     # fewer than three faces: the input


def test_get_mesh_from_udf_device_clean_is_bit_identical():
    """the decoder, latent seed and arguments of test_get_mesh_from_udf_device_post_is_bit_identical (tests/test_gpu_meshsmooth.py)"""
    from surfd_amd import synth
    from surfd_amd.cbndec import CbnDecoder, make_udf_func
    from surfd_amd.meshudf import get_mesh_from_udf
    from surfd_amd.spec import DecoderConfig
    dec = CbnDecoder(63, 32, 512, 5)
    dec.load_state_dict(synth.synth_decoder_state_dict(DecoderConfig(latent_dim=32)), strict=True)
    dec = dec.cuda().eval()
    lat = (torch.randn(1, 32, generator=torch.Generator().manual_seed(2)) * 0.8).cuda()
    field = make_udf_func(dec, lat)
    kw = dict(coords_range=(-1, 1), max_dist=0.1, N=64, max_batch=2 ** 16)
    v0, t0 = get_mesh_from_udf(field, differentiable=False, **kw)
    v1, t1 = get_mesh_from_udf(field, differentiable=False, device_clean=True, **kw)
    assert len(t0) > 0 and v1.dtype == torch.float32 and t1.dtype == torch.int64
    assert torch.equal(t0, t1) and torch.equal(v0, v1)
    v2, t2 = get_mesh_from_udf(field, differentiable=False, smooth_borders=False, device_clean=True, **kw)
    assert torch.equal(t0, t2) and torch.equal(v2, get_mesh_from_udf(field, differentiable=False, smooth_borders=False, **kw)[0])
    v3, t3 = get_mesh_from_udf(field, differentiable=True, device_clean=True, **kw)
    assert torch.equal(t0, t3)
    np.testing.assert_allclose(v3.detach().cpu().numpy(), v0.cpu().numpy(), atol=1e-6)


# ---- at size, at every key width, in every rotation, on random soups, through the C ABI ----------------------------------------------
def check_chain(MC, v, f, h):
    """every function on one mesh against meshproc's chain h: the cull, each later step on meshproc's own intermediate result and
    on the raw mesh, the loop with its stats.  Returns the device's cull."""
    dv, df = cu(v), cu(f)
    gv, gf = MC.cull_and_merge(dv, df)
    same_v(gv, h["v1"]); same_f(gf, h["f0"])
    dv1 = cu(h["v1"])
    same_f(MC.drop_duplicate_faces(cu(h["f0"])), h["fd"])
    same_f(MC.drop_degenerate_faces(dv1, cu(h["fd"])), h["fg"])
    same_f(MC.fill_small_holes(dv1, cu(h["fg"])), h["fh"])
    same_f(MC.drop_duplicate_faces(df), h["raw"][0])
    same_f(MC.drop_degenerate_faces(dv, df), h["raw"][1])
    same_f(MC.fill_small_holes(dv, df), h["raw"][2])
    cv, cf, st = MC.clean_until_stable(dv, df, return_stats=True)
    same_v(cv, h["cv"]); same_f(cf, h["cf"])
    assert st == h["stats"], (st, h["stats"])
    return gv, gf


@pytest.mark.parametrize("name", ["torus_soup", "torus_soup_jitter", "fan"])
def test_merges_at_size(name):
    """classes whose members lie anywhere in 50 688 (18 500) indices: the three radix sorts, the heads, the running maximum and the
    two sums over many tiles.  torus_soup: 70 % negative keys, six copies per vertex; the jitter splits classes at the rounding
    edge and leaves lone faces, which are capped and removed again; fan: one class of 5 000, a run of 3 500 vertices that take no
    part between the classes of positive and of negative x, the last of them a copy of the vertex that follows the run."""
    from surfd_amd import meshclean as MC
    from surfd_amd import meshtopo
    v, f = BIG[name]
    gv, gf = check_chain(MC, v, f, host(name))
    ov, of = gv.cpu().numpy(), gf.cpu().numpy()
    if name == "torus_soup":                                 # what holds without meshproc: every corner keeps its bits, the torus is whole again
        assert np.array_equal(ov[of].view(np.int64), v[f].view(np.int64))
        assert len(ov) == R.TORUS_VERTICES and len(np.unique(ov, axis=0)) == R.TORUS_VERTICES
        assert meshtopo.is_closed(gf, R.TORUS_VERTICES)
    if name == "fan":
        assert np.isfinite(ov).all()
        assert np.array_equal(np.unique(of), np.arange(len(ov)))
        assert (ov == np.array(R.FAN_APEX)).all(axis=1).sum() == 1 and len(ov) == 5001 and len(of) == 5000
        assert (of == np.nonzero((ov == np.array(R.FAN_APEX)).all(axis=1))[0][0]).any(axis=1).all()      # every face names the apex


def test_duplicates_at_size():
    """18 661 faces, every one of sheet64's two or three times, rotated and reversed: both sorts of the duplicate pass over several
    tiles with something to remove.  The expected order and survivors come from the input alone."""
    from surfd_amd import meshclean as MC
    _, f = BIG["doubled_sheet"]
    got = MC.drop_duplicate_faces(cu(f))
    same_f(got, mp.drop_duplicate_faces(f))
    s = np.sort(f, axis=1)
    order = np.lexsort((np.arange(len(f)), s[:, 0], s[:, 1], s[:, 2]))        # by (largest, middle, smallest index, face)
    head = np.ones(len(f), dtype=bool)
    head[1:] = (s[order][1:] != s[order][:-1]).any(axis=1)
    same_f(got, f[order[head]])                              # the lowest face of every class, with its own winding
    g = np.sort(got.cpu().numpy(), axis=1)
    key = (g[:, 2] << 42) | (g[:, 1] << 21) | g[:, 0]        # indices below 4 225
    assert (np.diff(key) > 0).all() and len(g) == len(R.sheet(64)[1]) < len(f) / 2


@pytest.mark.parametrize("V", R.PAD_SIZES)
@pytest.mark.parametrize("name", R.PAD_NAMES)
def test_hole_keys_at_every_index_width(name, V):
    """the hole pass sorts 2 b key bits, b the bits of an index below V: a 3-hole and a 4-hole whose loops sit at V - 1, V - 2, ...
    on both sides of 2^8 and 2^16.  First with the whole solid at the top; then with two edges that differ in the highest key bit
    alone (meshclean_ref.padded, split), which a sort one bit short tears apart."""
    from surfd_amd import meshclean as MC
    v0, f0 = SHAPES[name]
    caps = mp.fill_small_holes(v0, f0)[len(f0):]
    assert len(caps) == (1 if name == "octahedron_minus_one" else 2)
    for split in (False, True):
        v, f, new = R.padded(name, V, split=split)
        want = mp.fill_small_holes(v, f)
        assert np.array_equal(want, np.vstack([f, new[caps]]))          # the solid's caps, re-indexed
        same_f(MC.fill_small_holes(cu(v), cu(f)), want)
        same_f(MC.fill_small_holes(cu(v), cu(f, torch.int32)), want)
        wv, wf = mp.clean_until_stable(v, f)
        gv, gf = MC.clean_until_stable(cu(v), cu(f))
        same_v(gv, wv); same_f(gf, wf)


def test_loops_in_every_rotation():
    """the 4-loop in each of its six rank patterns and the 3-loop in both (asserted in tests/test_meshclean_cpu.py), alone and as
    80 components of one mesh: side by side, and with all labels shuffled, so that other loops' slots lie between the two caps of
    a 4-loop"""
    from surfd_amd import meshclean as MC
    every = R.relabellings()
    meshes = [(v, f) for _, _, v, f in every]
    for name, seed, v, f in every + [("side by side", None) + R.side_by_side(meshes), ("side by side, shuffled", 0) + R.side_by_side(meshes, 0)]:
        try:
            want = mp.fill_small_holes(v, f)
            assert len(want) > len(f)
            same_f(MC.fill_small_holes(cu(v), cu(f)), want)
            wv, wf = mp.clean_until_stable(v, f)
            gv, gf = MC.clean_until_stable(cu(v), cu(f))
            same_v(gv, wv); same_f(gf, wf)
        except AssertionError as e:
            raise AssertionError(f"{name}, seed {seed}: {e}") from e


SOUP_SEED, SOUPS = 7, 400


def test_random_soups_on_the_device():
    """the soups of tests/test_meshclean_cpu.py (vertices that coincide and faces that are collinear around the tolerance, NaN and
    Inf coordinates, repeated indices): every function on the raw soup and on meshproc's intermediate results, the loop with its
    stats.  What these 400 hold is asserted in test_first_400_soups_take_every_path."""
    from surfd_amd import meshclean as MC
    for i, (v, f) in enumerate(R.first_soups(SOUPS, SOUP_SEED)):
        h = host_of(v, f)                                    # meshproc refuses none of them: an exception here fails the test
        try:
            check_chain(MC, v, f, h)
        except AssertionError as e:
            raise AssertionError(f"soup {i} of random_soup(default_rng({SOUP_SEED})): {e}") from e


SENT32, SENT64, TAIL = -0x5A5A5A5B, 0x7FF85A5A5A5A5A5A, 16   # no index is negative; no vertex is this NaN


class Raw:
    """the C ABI as it is: outputs of the input's size and TAIL rows more, filled with a sentinel; every call checks its return
    code, that nothing was written behind the count it reports, that every row before it was, and that the inputs are untouched"""

    def __init__(self):
        from surfd_amd import _native as N
        self.N, self.lib = N, N.lib()

    def _done(self, rc, inputs, outs):
        torch.cuda.synchronize()
        self.N.check(rc)
        for t, before in inputs:
            assert torch.equal(t.view(torch.int64) if t.dtype == torch.float64 else t, before), "an input was written to"
        for buf, n, sentinel in outs:
            buf = buf.cpu()
            assert bool((buf[n:] == sentinel).all()), f"rows behind the count {n} were written"
            assert bool((buf[:n] != sentinel).all()), f"rows before the count {n} were not written"

    @staticmethod
    def _in(v=None, f=None):
        out = []
        if v is not None:
            v = cu(np.asarray(v, dtype=np.float64).reshape(-1, 3))
            out += [v, (v, v.view(torch.int64).clone())]
        if f is not None:
            f = cu(np.asarray(f).reshape(-1, 3), torch.int32)
            out += [f, (f, f.clone())]
        return out

    def cull(self, v, f):
        N = self.N
        dv, keep_v, df, keep_f = self._in(v, f)
        ov = torch.full((len(v) + TAIL, 3), SENT64, device="cuda", dtype=torch.int64)
        of = torch.full((len(f) + TAIL, 3), SENT32, device="cuda", dtype=torch.int32)
        c = (C.c_int64 * 5)()
        rc = self.lib.surfd_meshclean_cull_and_merge(N.ptr(dv), len(v), N.ptr(df), len(f), 1.0 / mp.MERGE_TOL, N.ptr(ov), N.ptr(of), c, N.stream())
        self._done(rc, [keep_v, keep_f], [(ov, c[0], SENT64), (of, c[1], SENT32)])
        return ov[:c[0]].view(torch.float64), of[:c[1]].long(), list(c)

    def _faces_out(self, call, f):
        of = torch.full((len(f) + TAIL, 3), SENT32, device="cuda", dtype=torch.int32)
        c = (C.c_int64 * 1)()
        rc, inputs = call(of, c)
        self._done(rc, inputs, [(of, c[0], SENT32)])
        return of[:c[0]].long()

    def dedup(self, f):
        N = self.N
        df, keep_f = self._in(f=f)
        return self._faces_out(lambda of, c: (self.lib.surfd_meshclean_drop_duplicate_faces(N.ptr(df), len(f), N.ptr(of), c, N.stream()), [keep_f]), f)

    def degen(self, v, f):
        N = self.N
        dv, keep_v, df, keep_f = self._in(v, f)
        return self._faces_out(lambda of, c: (self.lib.surfd_meshclean_drop_degenerate_faces(N.ptr(dv), len(v), N.ptr(df), len(f), mp.MERGE_TOL, N.ptr(of),
                                                                                               c, N.stream()), [keep_v, keep_f]), f)

    def fill(self, V, f):
        """(caps, counts); before it, the refusal of a caps buffer one row short of min(V, 3 F / 2), which writes nothing"""
        N = self.N
        df, keep_f = self._in(f=f)
        most = min(V, 3 * len(f) // 2)
        caps = torch.full((most + TAIL, 3), SENT32, device="cuda", dtype=torch.int32)
        c = (C.c_int64 * 3)(-1, -1, -1)
        rc = self.lib.surfd_meshclean_fill_small_holes(N.ptr(df), len(f), V, N.ptr(caps), most - 1, c, N.stream())
        torch.cuda.synchronize()
        assert rc == -1 and list(c) == [0, 0, 0] and bool((caps == SENT32).all())          # SURFD_ERR_ARG
        rc = self.lib.surfd_meshclean_fill_small_holes(N.ptr(df), len(f), V, N.ptr(caps), most, c, N.stream())
        self._done(rc, [keep_f], [(caps, c[0], SENT32)])
        assert c[0] == c[1] + 2 * c[2] <= most
        return caps[:c[0]].long(), list(c)


@pytest.mark.parametrize("name", ["soup", "torus_soup_jitter"])
def test_raw_abi_writes_stop_at_the_counts(name):
    """the wrapper allocates with empty_like and slices: here the buffers carry a sentinel and TAIL rows more than the largest
    result, and every call must leave both alone behind its counts"""
    v, f = MESHES[name]
    h, raw = host(name), Raw()
    gv, gf, c = raw.cull(v, f)
    same_v(gv, h["v1"]); same_f(gf, h["f0"])
    st = R.new_stats()
    R.cull_and_merge(v, f, stats=st)
    assert c[2:] == [st["nonfinite_vertices"], st["unreferenced_vertices"], st["merged_vertices"]], (c, st)
    same_f(raw.dedup(h["f0"]), h["fd"])
    same_f(raw.dedup(f), h["raw"][0])
    same_f(raw.degen(h["v1"], h["fd"]), h["fg"])
    same_f(raw.degen(v, f), h["raw"][1])
    for V, faces, want in ((len(h["v1"]), h["fg"], h["fh"]), (len(v), f, h["raw"][2])):
        assert len(faces) >= 3
        caps, c = raw.fill(V, faces)
        same_f(caps, want[len(faces):])
        st = R.new_stats()
        R.fill_small_holes(None, faces, st)
        assert c[1:] == [st["caps3"], st["caps4"]] and c[0] == len(want) - len(faces), (c, st)      # loops: c[1] + c[2]
    assert name == "soup" or (c[1] > 10000 and len(h["fh"]) > len(h["fg"]))       # every face of the raw soup stands alone: a 3-loop each


def test_streams_handles_and_repeats_at_size():
    """the jittered soup (two rounds, 300 caps) on a stream of its own, ten times over, and as float32 / int32"""
    from surfd_amd import meshclean as MC
    v, f = BIG["torus_soup_jitter"]
    h = host("torus_soup_jitter")
    dv, df = cu(v), cu(f)
    v0, f0, st0 = MC.clean_until_stable(dv, df, return_stats=True)
    same_v(v0, h["cv"]); same_f(f0, h["cf"])
    assert st0 == h["stats"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v1, f1, st1 = MC.clean_until_stable(dv, df, return_stats=True)
        m1 = MC.cull_and_merge(dv, df)
    side.synchronize()
    assert torch.equal(f0, f1) and torch.equal(v0.view(torch.int64), v1.view(torch.int64)) and st0 == st1
    same_v(m1[0], h["v1"]); same_f(m1[1], h["f0"])
    for _ in range(10):
        v1, f1 = MC.clean_until_stable(dv, df)
        assert torch.equal(f0, f1) and torch.equal(v0.view(torch.int64), v1.view(torch.int64))
    v32 = v.astype(np.float32)
    with np.errstate(all="ignore"):
        wv, wf = mp.clean_until_stable(v32, f)               # np.asarray(..., float64) of the float32 array
    gv, gf = MC.clean_until_stable(cu(v32), cu(f, torch.int32))
    same_v(gv, wv); same_f(gf, wf)
    gv64, gf64 = MC.clean_until_stable(cu(v32).double(), df)
    assert torch.equal(gf, gf64) and torch.equal(gv.view(torch.int64), gv64.view(torch.int64))
    assert len(wv) != len(h["cv"])                           # float32 cannot hold the jitter: another mesh, not the same one again
