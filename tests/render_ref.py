"""Yardsticks of the mesh renderer (surfd_amd/render.py, csrc/raster.hip), numpy only.

  render_f32    the kernel's arithmetic restated: every fp32 operation in the kernel's order (numpy rounds each operation of a
                float32 array once), integer coverage in int64, the winner as the minimum of (depth bits << 32) | face.
  depth_f64     the same geometry in fp64: the SNAPPED screen triangle (so coverage is the kernel's), fp64 camera z of the fp32
                inputs, fp64 barycentrics and depth; for every pixel the fp64 depth of a given face buffer and the fp64 minimum
                over all covering faces.
  contours_ref  the contour rule.
  scenes        the meshes and cameras the tests share.

Run as a script it prints the restatement's worst deviation from fp64 on the test scenes (depth relative to the scene's depth
range, barycentrics, normals), in units of u = 2^-24: the numbers DESIGN.md section 8.4 quotes and tests/test_gpu_render.py
takes its tolerance from (DEPTH_BASE_U below is that printout, rounded up)."""
import os
import sys

import numpy as np

F32 = np.float32
U = 2.0 ** -24
SMALL_MAX = 16                  # RS_SMALL_MAX of csrc/raster.hip
SNAP_MAX = 1 << 22
# worst |depth_f32 - depth_f64| / (scene depth range) of render_f32 on fp64_scenes(), in u, as `python tests/render_ref.py`
# prints it (rounded up); the GPU test allows DEPTH_TOL_FACTOR times that (the factor of DESIGN.md section 8.2)
DEPTH_BASE_U = 8.9
DEPTH_TOL_FACTOR = 4.0


# ---- vertex stage -------------------------------------------------------------------------------------------------------------
def project_f32(vertices, cam):
    """vertices [V, 3] float32, cam [18] float32 -> sx, sy (int64), valid, d (float32), cam_xyz [V, 3] float32"""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    cam = np.asarray(cam, F32)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    row = lambda m: ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
    xc, yc, zc = row(cam[0:4]), row(cam[4:8]), row(cam[8:12])
    ortho = cam[12] != 0
    fx, fy, cx, cy, near = cam[13], cam[14], cam[15], cam[16], cam[17]
    with np.errstate(all="ignore"):
        if ortho:
            u = fx * xc + cx
            w = fy * yc + cy
            d = zc.copy()
        else:
            u = (fx * xc) / zc + cx
            w = (fy * yc) / zc + cy
            d = F32(1) - near / zc
        su, sv = np.rint(u * F32(256)), np.rint(w * F32(256))
        valid = (zc > near) & (np.abs(su) <= SNAP_MAX) & (np.abs(sv) <= SNAP_MAX)
    sx = np.where(valid, su, 0).astype(np.int64)
    sy = np.where(valid, sv, 0).astype(np.int64)
    return sx, sy, valid, np.where(valid, d, 0).astype(F32), np.stack([xc, yc, zc], 1).astype(F32)


# ---- set-up and coverage (integer, shared by the fp32 and the fp64 version) -----------------------------------------------------
def _setup(sx, sy, valid, faces, H, W):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(sx)
    in_range = ((f >= 0) & (f < V)).all(1)
    fc = np.where(in_range[:, None], f, 0)
    ok = in_range & valid[fc].all(1) if V else np.zeros(len(f), bool)
    dropped = int((~ok).sum())
    ax, ay = sx[fc[:, 0]] if V else np.zeros(len(f), np.int64), sy[fc[:, 0]] if V else np.zeros(len(f), np.int64)
    bx, by = (sx[fc[:, 1]], sy[fc[:, 1]]) if V else (ax, ay)
    cx, cy = (sx[fc[:, 2]], sy[fc[:, 2]]) if V else (ax, ay)
    a2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    swapped = a2 < 0
    bx, cx = np.where(swapped, cx, bx), np.where(swapped, bx, cx)
    by, cy = np.where(swapped, cy, by), np.where(swapped, by, cy)
    order = np.stack([fc[:, 0], np.where(swapped, fc[:, 2], fc[:, 1]), np.where(swapped, fc[:, 1], fc[:, 2])], 1)
    a2 = np.abs(a2)
    xmin, xmax = np.minimum(ax, np.minimum(bx, cx)), np.maximum(ax, np.maximum(bx, cx))
    ymin, ymax = np.minimum(ay, np.minimum(by, cy)), np.maximum(ay, np.maximum(by, cy))
    i0, i1 = np.maximum(0, (xmin - 128 + 255) >> 8), np.minimum(W - 1, (xmax - 128) >> 8)
    j0, j1 = np.maximum(0, (ymin - 128 + 255) >> 8), np.minimum(H - 1, (ymax - 128) >> 8)
    draw = ok & (a2 != 0) & (i0 <= i1) & (j0 <= j1)
    k = np.nonzero(draw)[0]
    return dict(k=k, order=order[k], swapped=swapped[k], a2=a2[k], ax=ax[k], ay=ay[k], bx=bx[k], by=by[k], cx=cx[k], cy=cy[k],
                i0=i0[k], i1=i1[k], j0=j0[k], j1=j1[k], dropped=dropped)


def _top_left(px, py, qx, qy):
    dx, dy = qx - px, qy - py
    return ((dy == 0) & (dx > 0)) | (dy < 0)


def _pairs(s):
    """every (drawable triangle, pixel of its clipped box): t (index into the set-up arrays), pi, pj, E0..E2 (int64), inside"""
    bw = s["i1"] - s["i0"] + 1
    cnt = bw * (s["j1"] - s["j0"] + 1)
    t = np.repeat(np.arange(len(cnt)), cnt)
    off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    pi, pj = s["i0"][t] + off % bw[t], s["j0"][t] + off // bw[t]
    px, py = 256 * pi + 128, 256 * pj + 128
    g = lambda n: s[n][t]
    edge = lambda p, q: (g(q + "x") - g(p + "x")) * (py - g(p + "y")) - (g(q + "y") - g(p + "y")) * (px - g(p + "x"))
    tl = lambda p, q: _top_left(g(p + "x"), g(p + "y"), g(q + "x"), g(q + "y"))
    e0, e1, e2 = edge("b", "c"), edge("c", "a"), edge("a", "b")
    inside = ((e0 > 0) | ((e0 == 0) & tl("b", "c"))) & ((e1 > 0) | ((e1 == 0) & tl("c", "a"))) & ((e2 > 0) | ((e2 == 0) & tl("a", "b")))
    return t, pi, pj, e0, e1, e2, inside


def coverage_counts(sx, sy, faces, H, W):
    """how many triangles cover each pixel (coordinates given in 1/256 pixel): the restatement's fill rule on its own"""
    s = _setup(np.asarray(sx, np.int64), np.asarray(sy, np.int64), np.ones(len(sx), bool), faces, H, W)
    t, pi, pj, _, _, _, inside = _pairs(s)
    out = np.zeros((H, W), np.int64)
    np.add.at(out, (pj[inside], pi[inside]), 1)
    return out


# ---- the fp32 restatement -----------------------------------------------------------------------------------------------------
def _normalise_turn(g, dtype):
    with np.errstate(all="ignore"):
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        n = np.where((ln > 0)[:, None], g / ln[:, None], dtype(0)).astype(dtype)
    return np.where((n[:, 2] > 0)[:, None], -n, n)


def render_view_f32(vertices, faces, cam, H, W, vertex_normals=None, light=(0.0, 0.0, -1.0), ambient=0.3):
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cam = np.asarray(cam, F32)
    sx, sy, valid, d, xyz = project_f32(v, cam)
    s = _setup(sx, sy, valid, f, H, W)
    t, pi, pj, e0, e1, e2, inside = _pairs(s)
    fa = s["a2"].astype(F32)
    key = np.full(H * W, np.uint64(0xFFFFFFFFFFFFFFFF))
    if len(t):
        b0, b1, b2 = e0.astype(F32) / fa[t], e1.astype(F32) / fa[t], e2.astype(F32) / fa[t]
        o = s["order"][t]
        dd = (b0 * d[o[:, 0]] + b1 * d[o[:, 1]]) + b2 * d[o[:, 2]]
        k64 = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | s["k"][t].astype(np.uint64)
        m = inside
        np.minimum.at(key, (pj[m] * W + pi[m]), k64[m])
    out = dict(face=np.full(H * W, -1, np.int32), depth=np.full(H * W, np.inf, F32), bary=np.zeros((H * W, 3), F32),
               normal=np.zeros((H * W, 3), F32), mask=np.zeros(H * W, np.uint8), shaded=np.zeros(H * W, F32), dropped=s["dropped"],
               key=key.reshape(H, W))
    pix = np.nonzero(key != np.uint64(0xFFFFFFFFFFFFFFFF))[0]
    if len(pix):
        face = (key[pix] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        # the winner's barycentrics again: its set-up row
        row = np.full(len(f), -1, np.int64)
        row[s["k"]] = np.arange(len(s["k"]))
        r = row[face]
        px, py = 256 * (pix % W) + 128, 256 * (pix // W) + 128
        g = lambda n: s[n][r]
        edge = lambda p, q: (g(q + "x") - g(p + "x")) * (py - g(p + "y")) - (g(q + "y") - g(p + "y")) * (px - g(p + "x"))
        fa_r = fa[r]
        b0, b1, b2 = edge("b", "c").astype(F32) / fa_r, edge("c", "a").astype(F32) / fa_r, edge("a", "b").astype(F32) / fa_r
        o = s["order"][r]
        dd = (b0 * d[o[:, 0]] + b1 * d[o[:, 1]]) + b2 * d[o[:, 2]]
        sw = s["swapped"][r]
        b1, b2 = np.where(sw, b2, b1), np.where(sw, b1, b2)                  # the caller's vertex order
        ia, ib, ic = f[face, 0], f[face, 1], f[face, 2]
        if cam[12] != 0:
            c0, c1, c2, depth = b0, b1, b2, dd
        else:
            w0, w1, w2 = b0 / xyz[ia, 2], b1 / xyz[ib, 2], b2 / xyz[ic, 2]
            sm = (w0 + w1) + w2
            c0, c1, c2, depth = w0 / sm, w1 / sm, w2 / sm, F32(1) / sm
        if vertex_normals is not None:
            vn = np.asarray(vertex_normals, F32).reshape(-1, 3)
            wv = (c0[:, None] * vn[ia] + c1[:, None] * vn[ib]) + c2[:, None] * vn[ic]
            rot = lambda m: (m[0] * wv[:, 0] + m[1] * wv[:, 1]) + m[2] * wv[:, 2]
            g3 = np.stack([rot(cam[0:3]), rot(cam[4:7]), rot(cam[8:11])], 1)
        else:
            ea, eb = xyz[ib] - xyz[ia], xyz[ic] - xyz[ia]
            g3 = np.stack([ea[:, 1] * eb[:, 2] - ea[:, 2] * eb[:, 1], ea[:, 2] * eb[:, 0] - ea[:, 0] * eb[:, 2],
                           ea[:, 0] * eb[:, 1] - ea[:, 1] * eb[:, 0]], 1)
        n = _normalise_turn(g3.astype(F32), F32)
        l = np.asarray(light, F32)
        amb = F32(ambient)
        dot = (n[:, 0] * l[0] + n[:, 1] * l[1]) + n[:, 2] * l[2]
        out["face"][pix] = face
        out["depth"][pix] = depth
        out["bary"][pix] = np.stack([c0, c1, c2], 1)
        out["normal"][pix] = n
        out["mask"][pix] = 1
        out["shaded"][pix] = amb + (F32(1) - amb) * np.abs(dot)
    for k in ("face", "depth", "mask", "shaded"):
        out[k] = out[k].reshape(H, W)
    out["bary"] = out["bary"].reshape(H, W, 3)
    out["normal"] = out["normal"].reshape(H, W, 3)
    return out


def render_f32(vertices, faces, cams, H, W, **kw):
    views = [render_view_f32(vertices, faces, c, H, W, **kw) for c in np.asarray(cams, F32).reshape(-1, 18)]
    out = {k: np.stack([v[k] for v in views]) for k in ("face", "depth", "bary", "normal", "mask", "shaded", "key")}
    out["dropped"] = np.array([v["dropped"] for v in views], np.int32)
    return out


def depth_ties(vertices, faces, cam, H, W):
    """how many (pixel, depth bits) pairs are shared by two covering triangles: 0 means no pixel's winner hangs on the face index"""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    sx, sy, valid, d, _ = project_f32(v, np.asarray(cam, F32))
    s = _setup(sx, sy, valid, faces, H, W)
    t, pi, pj, e0, e1, e2, inside = _pairs(s)
    fa = s["a2"].astype(F32)
    o = s["order"][t]
    dd = ((e0.astype(F32) / fa[t]) * d[o[:, 0]] + (e1.astype(F32) / fa[t]) * d[o[:, 1]]) + (e2.astype(F32) / fa[t]) * d[o[:, 2]]
    code = ((pj * W + pi).astype(np.uint64) << np.uint64(32)) | dd.view(np.uint32).astype(np.uint64)
    code = np.sort(code[inside])
    return int((code[1:] == code[:-1]).sum())


# ---- fp64 -----------------------------------------------------------------------------------------------------------------------
def depth_f64(vertices, faces, cam, H, W, face_buffer):
    """-> (chosen [H, W]: the fp64 depth of face_buffer's face at every covered pixel, NaN elsewhere; best [H, W]: the fp64
    minimum over all covering faces, +inf where none; bary [H, W, 3] and normal [H, W, 3] of the chosen face in fp64;
    depth range of the scene's valid vertices)"""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cam = np.asarray(cam, F32)
    sx, sy, valid, _, _ = project_f32(v, cam)
    s = _setup(sx, sy, valid, f, H, W)
    t, pi, pj, e0, e1, e2, inside = _pairs(s)
    c64, v64 = cam.astype(np.float64), v.astype(np.float64)
    xyz = v64 @ c64[:12].reshape(3, 4)[:, :3].T + c64[:12].reshape(3, 4)[:, 3]
    z = xyz[:, 2]
    a2 = s["a2"].astype(np.float64)
    b = np.stack([e0, e1, e2], 1).astype(np.float64) / a2[t][:, None]
    o = s["order"][t]
    zz = z[o]
    dep = 1.0 / (b / zz).sum(1) if cam[12] == 0 else (b * zz).sum(1)
    best = np.full(H * W, np.inf)
    p = pj * W + pi
    np.minimum.at(best, p[inside], dep[inside])
    chosen = np.full(H * W, np.nan)
    bary = np.zeros((H * W, 3))
    normal = np.zeros((H * W, 3))
    fb = np.asarray(face_buffer).reshape(-1)
    hit = inside & (s["k"][t] == fb[p])
    chosen[p[hit]] = dep[hit]
    bb = b[hit]
    sw = s["swapped"][t][hit]
    bb = np.stack([bb[:, 0], np.where(sw, bb[:, 2], bb[:, 1]), np.where(sw, bb[:, 1], bb[:, 2])], 1)
    fi = f[s["k"][t][hit]]
    if cam[12] == 0:
        w = bb / z[fi]
        bb = w / w.sum(1, keepdims=True)
    bary[p[hit]] = bb
    g3 = np.cross(xyz[fi[:, 1]] - xyz[fi[:, 0]], xyz[fi[:, 2]] - xyz[fi[:, 0]])
    normal[p[hit]] = _normalise_turn(g3, np.float64)
    zr = z[valid]
    return chosen.reshape(H, W), best.reshape(H, W), bary.reshape(H, W, 3), normal.reshape(H, W, 3), float(zr.max() - zr.min())


# ---- contours -------------------------------------------------------------------------------------------------------------------
def contours_ref(mask, depth, normal, depth_jump, cos_crease):
    """[n, H, W] uint8, [n, H, W] float32, [n, H, W, 3] float32 -> ink [n, H, W] uint8"""
    m = np.asarray(mask) != 0
    d = np.where(m, np.asarray(depth, F32), F32(0))
    nr = np.asarray(normal, F32)
    n, H, W = m.shape
    ink = np.zeros_like(m)
    mp = np.pad(m, ((0, 0), (1, 1), (1, 1)))
    dp = np.pad(d, ((0, 0), (1, 1), (1, 1)))
    npad = np.pad(nr, ((0, 0), (1, 1), (1, 1), (0, 0)))
    for dj, di in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        mn = mp[:, 1 + dj:1 + dj + H, 1 + di:1 + di + W]
        dn = dp[:, 1 + dj:1 + dj + H, 1 + di:1 + di + W]
        nn = npad[:, 1 + dj:1 + dj + H, 1 + di:1 + di + W]
        both = m & mn
        dot = (nr[..., 0] * nn[..., 0] + nr[..., 1] * nn[..., 1]) + nr[..., 2] * nn[..., 2]
        ink |= (m != mn) | (both & (np.abs(d - dn) > F32(depth_jump))) | (both & (dot < F32(cos_crease)))
    return ink.astype(np.uint8)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def wavy_sheet(n_triangles, jitter=0.0, seed=0, amplitude=0.15, extent=0.8):
    """an open wavy sheet of about n_triangles triangles in [-1, 1]^3 (alternating diagonals, so both windings occur)"""
    m = max(2, int(round((n_triangles / 2) ** 0.5)))
    g = np.linspace(-extent, extent, m + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    z = amplitude * (np.sin(4.0 * x) * np.cos(3.0 * y) + 0.5 * np.sin(7.0 * x + 2.0 * y))
    v = np.stack([x, y, z], -1).reshape(-1, 3)
    if jitter:
        v = v + np.random.default_rng(seed).uniform(-jitter, jitter, v.shape)
    idx = lambda r, c: r * (m + 1) + c
    r, c = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    r, c = r.reshape(-1), c.reshape(-1)
    even = (r + c) % 2 == 0
    t1 = np.where(even[:, None], np.stack([idx(r, c), idx(r, c + 1), idx(r + 1, c + 1)], 1), np.stack([idx(r, c), idx(r, c + 1), idx(r + 1, c)], 1))
    t2 = np.where(even[:, None], np.stack([idx(r, c), idx(r + 1, c), idx(r + 1, c + 1)], 1), np.stack([idx(r, c + 1), idx(r + 1, c + 1), idx(r + 1, c)], 1))
    return v.astype(F32), np.concatenate([t1, t2]).astype(np.int32)


def box(half=(0.6, 0.45, 0.5)):
    """a closed box of 12 triangles"""
    h = np.asarray(half)
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v.astype(F32), np.array(f, np.int32)


def folded_sheet(angle_deg=90.0, n=6):
    """two flat wings meeting along the y axis with `angle_deg` between their normals"""
    a = np.radians(angle_deg) / 2
    g = np.linspace(-0.7, 0.7, n + 1)
    s = np.linspace(0.0, 0.7, n + 1)
    verts, faces = [], []
    for sign in (-1, 1):
        base = len(verts)
        for yy in g:
            for ss in s:
                verts.append([sign * ss * np.cos(a), yy, ss * np.sin(a)])
        for r in range(n):
            for c in range(n):
                p = base + r * (n + 1) + c
                faces += [[p, p + 1, p + n + 2], [p, p + n + 2, p + n + 1]]
    return np.array(verts, F32), np.array(faces, np.int32)


def pixel_camera(near=0.0):
    """the orthographic camera under which world (x, y, z) IS pixel (x, y) at depth z"""
    return np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 1, 1, 0, 0, near]], F32)


def rule_triangle(where):
    """a right triangle with its vertices on pixel centres or on pixel corners, for the pixel camera"""
    o = 0.5 if where == "centres" else 0.0
    hi = 6.5 if where == "centres" else 7.0
    return np.array([[1 + o, 1 + o, 1], [hi, 1 + o, 1], [1 + o, hi, 1]], F32)


def _render_module():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from surfd_amd import render
    return render


def fp64_scenes():
    """[(name, vertices, faces, cameras [n, 18] float32, H, W)]: the scenes of the restatement and fp64 GPU tests"""
    R = _render_module()
    out = []
    for name, (v, f) in (("sheet", wavy_sheet(2000)), ("box", box())):
        for mode in ("perspective", "orthographic"):
            for (H, W) in ((48, 48), (61, 97)):
                cams = R.orbit_cameras(2, 25.0, 2.6, mode=mode, size=(H, W)).numpy()
                out.append((f"{name}-{mode}-{W}x{H}", v, f, cams, H, W))
    return out


def restatement_error():
    """worst deviation of render_f32 from fp64 over fp64_scenes(): depth / depth range, bary, normal (absolute), each in u"""
    worst = dict(depth=0.0, bary=0.0, normal=0.0, near_tie=0.0)
    for name, v, f, cams, H, W in fp64_scenes():
        r = render_f32(v, f, cams, H, W)
        for i, cam in enumerate(cams):
            chosen, best, bary, normal, zrange = depth_f64(v, f, cam, H, W, r["face"][i])
            m = r["mask"][i] != 0
            assert np.isfinite(chosen[m]).all() and np.isnan(chosen[~m]).all() and np.array_equal(m, np.isfinite(best))
            worst["depth"] = max(worst["depth"], float(np.abs(r["depth"][i][m].astype(np.float64) - chosen[m]).max() / zrange / U))
            worst["near_tie"] = max(worst["near_tie"], float((chosen[m] - best[m]).max() / zrange / U))
            worst["bary"] = max(worst["bary"], float(np.abs(r["bary"][i][m] - bary[m]).max() / U))
            worst["normal"] = max(worst["normal"], float(np.abs(r["normal"][i][m] - normal[m]).max() / U))
    return worst


if __name__ == "__main__":
    w = restatement_error()
    print(f"fp32 restatement vs fp64 on {len(fp64_scenes())} scenes x 2 views, in u = 2^-24:")
    print(f"  depth / depth range        {w['depth']:.3f} u   (DEPTH_BASE_U = {DEPTH_BASE_U}, GPU tolerance {DEPTH_TOL_FACTOR * DEPTH_BASE_U} u)")
    print(f"  chosen face vs fp64 minimum {w['near_tie']:.3f} u")
    print(f"  barycentrics (absolute)    {w['bary']:.3f} u")
    print(f"  normals (absolute)         {w['normal']:.3f} u")
