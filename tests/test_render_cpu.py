"""CPU-side checks of the mesh renderer (surfd_amd/render.py, csrc/raster.hip): the camera helpers against hand-computed
matrices, the fill rule of the numpy restatement (tests/render_ref.py) on its own, the PNG writer and reader, the condition
helpers against surfd_amd/preprocess.py, the exports and their table, the argument checks of the library, and the kernels'
code-object metadata (no spills, no scratch).  Every test here fails on a tree without surfd_amd/render.py or without the
surfd_raster_* symbols."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from surfd_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RASTER_EXPORTS = ("surfd_raster_create", "surfd_raster_destroy", "surfd_raster_render", "surfd_raster_contours")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        from surfd_amd.build import build_library
        build_library()
    return N.lib()


@pytest.fixture(scope="module")
def RD():
    from surfd_amd import render
    return render


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. library -------------------------------------------------------------------------------------------------------------------
def test_exports_bindings_and_table(lib):
    raw = C.CDLL(N.LIB_PATH)
    for sym in RASTER_EXPORTS:
        assert hasattr(raw, sym), sym
        assert sym in N.EXPORTED_SYMBOLS, sym
    assert lib.surfd_abi_version() == 1
    assert "raster.hip" in __import__("surfd_amd.build", fromlist=["SOURCES"]).SOURCES
    rows = {r.split("|")[1].strip(" `"): r for r in _tool("abi_table").table().splitlines()[2:]}
    for sym in RASTER_EXPORTS:
        assert sym in rows, sym
        if sym != "surfd_raster_destroy":
            assert "no reference counterpart (" in rows[sym] and "`surfd_amd/render.py`" in rows[sym], rows[sym]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"| `{s}` |" in doc for s in RASTER_EXPORTS)


def test_argument_errors_are_return_codes(lib):
    h = C.c_void_p()
    for H, W, n in ((0, 8, 1), (8, 0, 1), (2049, 8, 1), (8, 2049, 1), (8, 8, 0), (8, 8, 65), (-1, 8, 1)):
        assert lib.surfd_raster_create(H, W, n, C.byref(h)) == -1, (H, W, n)
        assert b"surfd_raster_create" in lib.surfd_last_error() and not h.value
    assert lib.surfd_raster_create(8, 8, 1, None) == -1
    p = C.c_void_p(16)                                         # never dereferenced: every call below fails its checks first
    cam = (C.c_float * 18)(*R.pixel_camera()[0])
    assert lib.surfd_raster_render(None, p, 3, p, 1, None, cam, 1, 0, None, 0.3, p, p, p, p, p, p, p, None) == -1
    assert b"null handle" in lib.surfd_last_error()
    assert lib.surfd_raster_contours(None, p, p, p, 1, 0.1, 0.5, p, None) == -1
    assert b"null handle" in lib.surfd_last_error()
    lib.surfd_raster_destroy(None)                             # a no-op


def test_kernels_do_not_spill():
    meta = _tool("kernel_regs").kernel_metadata()
    names = sorted(k for k in meta if "surfd::rs_" in k)
    want = ["rs_contour_kernel", "rs_large_kernel", "rs_project_kernel", "rs_resolve_kernel", "rs_small_kernel"]
    assert len(names) == 5 and all(any(w in k for k in names) for w in want), names
    for k in names:
        v = meta[k]
        assert v[".vgpr_spill_count"] == 0 and v[".sgpr_spill_count"] == 0, (k, v)
        assert v[".private_segment_fixed_size"] == 0, (k, v)
        assert v[".group_segment_fixed_size"] == 0, (k, v)                  # no LDS


# ---- 2. cameras -------------------------------------------------------------------------------------------------------------------
def test_look_at_against_hand_computed_matrices(RD):
    m = RD.look_at((0.0, 0.0, 2.0))                            # on the +z axis looking at the origin: x right, y down, z forward
    assert m.dtype == torch.float32 and m.shape == (3, 4)
    assert torch.equal(m, torch.tensor([[1.0, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 2]]))
    m = RD.look_at((3.0, 0.0, 0.0))                            # on the +x axis: right is world -z
    assert torch.equal(m, torch.tensor([[0.0, 0, -1, 0], [0, -1, 0, 0], [-1, 0, 0, 3]]))
    m = RD.look_at((0.0, 5.0, 0.0), up=(0.0, 0.0, -1.0))       # from above, image up = world -z
    assert torch.equal(m, torch.tensor([[1.0, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 5]]))
    m = RD.look_at((1.0, 2.0, 3.0), (1.0, 2.0, 0.0)).double()
    assert torch.allclose(m[:, :3] @ m[:, :3].T, torch.eye(3, dtype=torch.float64), atol=1e-7)
    assert torch.allclose(m[:, :3] @ torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64) + m[:, 3], torch.zeros(3, dtype=torch.float64), atol=1e-6)
    with pytest.raises(ValueError, match="coincide"):
        RD.look_at((1.0, 1.0, 1.0), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="parallel"):
        RD.look_at((0.0, 1.0, 0.0))


def test_orbit_cameras(RD):
    c = RD.orbit_cameras(4, 0.0, 2.0, fov_deg=90.0, size=(100, 200), near=0.1)
    assert c.shape == (4, 18) and c.dtype == torch.float32
    assert torch.equal(c[0, :12].reshape(3, 4), RD.look_at((0.0, 0.0, 2.0)))
    assert torch.allclose(c[1, :12].reshape(3, 4), RD.look_at((2.0, 0.0, 0.0)), atol=1e-6)
    # 90 degrees over the shorter side (100 pixels): f = 50; principal point at the centre
    assert c[0, 12:].tolist() == pytest.approx([0.0, 50.0, 50.0, 100.0, 50.0, 0.1], rel=1e-6)
    o = RD.orbit_cameras(1, 30.0, 3.0, mode="orthographic", ortho_half=2.0, size=64)
    assert o[0, 12:].tolist() == pytest.approx([1.0, 16.0, 16.0, 32.0, 32.0, 0.05], rel=1e-6)
    eye = -(o[0, :12].reshape(3, 4)[:, :3].T @ o[0, :12].reshape(3, 4)[:, 3])
    assert torch.allclose(eye, torch.tensor([0.0, 1.5, 3.0 * 3 ** 0.5 / 2]), atol=1e-6)
    # the origin projects to the image centre, a point above it to a smaller row
    sx, sy, valid, d, xyz = R.project_f32(np.array([[0, 0, 0], [0, 0.5, 0]], np.float32), c[0].numpy())
    assert valid.all() and sx.tolist() == [256 * 100, 256 * 100] and sy[0] == 256 * 50 and sy[1] == 256 * 50 - 256 * 50 // 4
    assert xyz[0].tolist() == [0.0, 0.0, 2.0] and d[0] == np.float32(1) - np.float32(0.1) / np.float32(2)
    with pytest.raises(ValueError, match="mode"):
        RD.orbit_cameras(2, 0.0, 2.0, mode="fisheye")


# ---- 3. the restatement's rules -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w0", [0, 1])
@pytest.mark.parametrize("w1", [0, 1])
@pytest.mark.parametrize("diag", [0, 1])
def test_shared_edge_covers_a_rectangle_once(w0, w1, diag):
    x0, y0, x1, y1 = 2 * 256 + 128, 3 * 256 + 128, 12 * 256 + 77, 11 * 256 + 128         # two corners on pixel centres, a ragged right side
    sx, sy = [x0, x1, x1, x0], [y0, y0, y1, y1]
    t0, t1 = ([0, 1, 2], [0, 2, 3]) if diag == 0 else ([0, 1, 3], [1, 2, 3])
    f = [t0[::-1] if w0 else t0, t1[::-1] if w1 else t1]
    cnt = R.coverage_counts(sx, sy, f, 16, 16)
    j, i = np.mgrid[0:16, 0:16]
    rect = (i >= 2) & (256 * i + 128 < x1) & (j >= 3) & (j <= 10)
    assert np.array_equal(cnt, rect.astype(np.int64))
    # a fan of 7 triangles around an interior vertex on a pixel centre: every pixel of the hexagon's box once at most, the centre once
    ang = np.arange(7) * 2 * np.pi / 7
    fx = [8 * 256 + 128] + [int(round(8.5 * 256 + 1500 * np.cos(a))) for a in ang]
    fy = [8 * 256 + 128] + [int(round(8.5 * 256 + 1500 * np.sin(a))) for a in ang]
    fan = [[0, 1 + k, 1 + (k + 1) % 7][::-1 if (k + w0) % 2 else 1] for k in range(7)]
    cnt = R.coverage_counts(fx, fy, fan, 16, 16)
    assert cnt.max() == 1 and cnt[8, 8] == 1 and cnt.sum() > 60


@pytest.mark.parametrize("where", ["centres", "corners"])
def test_vertex_on_a_pixel_centre_follows_the_top_left_rule(where):
    v = R.rule_triangle(where)
    r = R.render_f32(v, [[0, 1, 2]], R.pixel_camera(), 8, 8)
    j, i = np.mgrid[0:8, 0:8]
    assert np.array_equal(r["mask"][0] != 0, (i >= 1) & (j >= 1) & (i + j <= 6))
    assert r["dropped"].tolist() == [0]
    flipped = R.render_f32(v, [[0, 2, 1]], R.pixel_camera(), 8, 8)
    assert np.array_equal(flipped["mask"], r["mask"]) and np.array_equal(flipped["depth"], r["depth"])
    # the right-angle vertex sits on the centre of pixel (1, 1) (centres) and owns it: a top AND a left edge meet there
    assert r["mask"][0, 1, 1] == 1 and r["mask"][0, 1, 6] == 0 and r["mask"][0, 6, 1] == 0


def test_zero_area_triangles_cover_nothing():
    sx, sy = [300, 900, 1500, 300], [300, 900, 1500, 300]
    assert not R.coverage_counts(sx, sy, [[0, 1, 2], [0, 0, 1], [0, 3, 0], [1, 1, 1]], 8, 8).any()
    v = np.array([[1.5, 1.5, 1], [3.5, 3.5, 1], [5.5, 5.5, 2]], np.float32)
    r = R.render_f32(v, [[0, 1, 2], [2, 2, 0]], R.pixel_camera(), 8, 8)
    assert not r["mask"].any() and (r["face"] == -1).all() and r["dropped"].tolist() == [0]


def test_restatement_against_fp64_is_the_recorded_base():
    """the number the GPU tolerance is 4 x of: the restatement's worst depth deviation from fp64, relative to the depth range"""
    w = R.restatement_error()
    print(w)
    assert 0.5 * R.DEPTH_BASE_U < w["depth"] <= R.DEPTH_BASE_U
    assert w["near_tie"] <= R.DEPTH_BASE_U and w["bary"] <= 4.0


def test_contour_rule_of_the_restatement():
    mask = np.zeros((1, 6, 6), np.uint8)
    mask[0, 0:4, 2:5] = 1                                       # touches the top border
    depth = np.where(mask != 0, np.float32(1), np.float32(np.inf)).astype(np.float32)
    normal = np.zeros((1, 6, 6, 3), np.float32)
    normal[mask != 0] = (0, 0, -1)
    ink = R.contours_ref(mask, depth, normal, 0.5, 0.5)[0]
    want = np.zeros((6, 6), np.uint8)
    want[0:5, 1:6] = 1
    want[1:3, 3] = 0                                            # the interior
    want[4, 1] = want[4, 5] = 0                                 # diagonal neighbours do not count
    assert np.array_equal(ink, want), ink
    depth[0, 2, 3] = 2.0
    assert R.contours_ref(mask, depth, normal, 0.5, 0.5)[0][1:4, 3].tolist() == [1, 1, 1]
    assert R.contours_ref(mask, depth, normal, 1.5, 0.5)[0][1:3, 3].tolist() == [0, 0]


# ---- 4. images --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7), (5, 7, 3), (4, 3, 4), (1, 1)])
def test_png_round_trip(RD, tmp_path, shape):
    img = np.random.default_rng(0).integers(0, 256, shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    RD.write_png(path, img)
    assert open(path, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    assert np.array_equal(RD.read_png(path), img)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(path)), img)               # a real decoder reads the same pixels
    Image.fromarray(img).save(path)                                        # and the reader takes a real encoder's filters
    assert np.array_equal(RD.read_png(path), img)
    with pytest.raises(TypeError, match="uint8"):
        RD.write_png(path, img.astype(np.float32))
    with pytest.raises(ValueError, match="write_png takes"):
        RD.write_png(path, np.zeros((2, 2, 2), np.uint8))


def test_to_uint8(RD):
    a = np.array([[0.0, 0.5, 1.0, np.inf]])
    assert RD.to_uint8(a).tolist() == [[0, 128, 255, 255]]
    assert RD.to_uint8(a, 0.0, 2.0, background=7).tolist() == [[0, 64, 128, 7]]
    assert RD.to_uint8(torch.full((2, 2), 3.0)).tolist() == [[0, 0], [0, 0]]


def test_condition_helpers_feed_the_preprocessing(RD):
    from surfd_amd import preprocess
    r = R.render_f32(*R.box(), RD.orbit_cameras(2, 25.0, 2.6, size=48).numpy(), 48, 48)
    buffers = {k: torch.from_numpy(r[k].copy()) for k in ("mask", "shaded", "depth", "normal")}
    rgb, mask = RD.condition_image(buffers, 1)
    assert rgb.shape == (48, 48, 3) and rgb.dtype == np.uint8 and mask.dtype == np.uint8 and set(np.unique(mask)) == {0, 1}
    assert rgb[mask == 1].min() >= int(0.3 * 255) and not rgb[mask == 0].any()
    clean, comp = preprocess.masked_crops(rgb, mask)
    assert clean.size == (256, 256) and comp.size == (256, 256)
    assert preprocess.clip_image_tensor(clean).shape == (3, 224, 224)
    ink = R.contours_ref(r["mask"], r["depth"], r["normal"], 0.05, RD.cos_crease(30.0))
    sk = RD.condition_sketch(ink, 0)
    assert sk.size == (48, 48) and sk.mode == "RGB"
    a = np.asarray(sk)
    assert set(np.unique(a)) == {0, 255} and np.array_equal(a[:, :, 0] == 0, ink[0] != 0)
    assert preprocess.sketch_clip_tensor(sk).shape == (3, 224, 224)
    assert RD.depth_image(buffers, 0).shape == (48, 48) and RD.normal_image(buffers, 0).shape == (48, 48, 3)
    assert (RD.shaded_image(buffers, 1)[mask == 0] == 255).all() and RD.shaded_image(buffers, 1)[mask == 1].max() < 255


# ---- 5. the module's refusals (no GPU needed) -------------------------------------------------------------------------------------
def test_input_checks_before_any_launch(RD):
    v, f = (torch.from_numpy(a) for a in R.box())
    with pytest.raises(ValueError, match="no CPU fallback"):
        RD.render_mesh(v, f)
    with pytest.raises(TypeError, match="float32"):
        RD.render_mesh(v.double(), f)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        RD.render_mesh(v, f.reshape(-1))
    with pytest.raises(TypeError, match="tensors"):
        RD.render_mesh(v.numpy(), f)
    cams = RD.orbit_cameras(2, 20.0, 2.6)
    assert RD._check_cameras(cams, 2).shape == (2, 18) and RD._check_cameras(cams[0], 2).shape == (1, 18)
    bad = cams.clone(); bad[1, 12] = 2.0
    with pytest.raises(ValueError, match="mode"):
        RD._check_cameras(bad, 2)
    with pytest.raises(TypeError, match="float32"):
        RD._check_cameras(cams.double(), 2)
    with pytest.raises(ValueError, match="NaN"):
        RD._check_cameras(cams * float("nan"), 2)


# ---- 6. the example driver's similarity path, with the seeded towers ----------------------------------------------------------------
@pytest.mark.parametrize("cond", ["text", "image"])
def test_example_clip_similarities_with_seeded_towers(RD, tmp_path, monkeypatch, capsys, cond):
    """examples/render.py's --clip_text / --clip_image path on restated views: every view's condition image goes through
    masked_crops -> clip_image_tensor -> the image tower, and the printed cosine is the one computed here from the same blocks"""
    import types
    from examples import render as EX
    from surfd_amd import clip_towers as ct, preprocess, synth
    towers = ct.ClipTowers(synth.synth_clip_state_dict(seed=16))
    monkeypatch.setattr(ct.ClipTowers, "from_file", classmethod(lambda cls, path: towers))
    r = R.render_f32(*R.box(), RD.orbit_cameras(2, 25.0, 2.6, size=48).numpy(), 48, 48)
    views = {k: torch.from_numpy(r[k].copy()) for k in ("mask", "shaded", "depth", "normal")}
    a = types.SimpleNamespace(clip_weights=None, clip_text=None, clip_image=None,
                              bpe_path=os.path.join(ROOT, "tests", "golden", "clip_bpe_merges_48894.txt.gz"))
    if cond == "text":
        a.clip_text = "a dining chair"
        want = towers.encode_text(ct.SimpleTokenizer(a.bpe_path).tokenize([a.clip_text]))
    else:
        img = np.random.default_rng(3).integers(0, 256, (40, 52, 3), dtype=np.uint8)
        a.clip_image = str(tmp_path / "photo.png")
        RD.write_png(a.clip_image, img)
        want = towers.encode_image(preprocess.clip_image_tensor(img)[None])
    assert EX.clip_similarities(a, views) is None and "skipped" in capsys.readouterr().out          # no weights file: says so
    a.clip_weights = str(tmp_path / "clip.pt")
    open(a.clip_weights, "wb").close()
    sim = EX.clip_similarities(a, views)
    assert len(sim) == 2 and "view 1: cosine similarity" in capsys.readouterr().out
    for k in range(2):
        rgb, mask = RD.condition_image(views, k)
        emb = towers.encode_image(preprocess.clip_image_tensor(preprocess.masked_crops(rgb, mask)[0])[None])
        assert sim[k] == pytest.approx(float(torch.nn.functional.cosine_similarity(emb, want)), abs=1e-5)
