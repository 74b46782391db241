"""Yardsticks of the point-cloud normals (surfd_amd/cloudnormals.py, csrc/cloudnormals.hip).  Neither the code under test nor its
output: numpy restatements of the seven steps of the kernel's contract, fp32 where the contract says fp32 and fp64 elsewhere,
every elementwise numpy operation being one IEEE rounding.

  knn_keys          steps 1-2: the sorted 64-bit keys bits(d2) << 32 | j of the K nearest candidates of every point
  covariances       step 3: the fp64 moments in rank order and the covariance matrices
  jacobi_f64ops     step 4: six cyclic Jacobi sweeps, + - * / sqrt only
  normals_f64ops    steps 1-7 of one cloud / normals_batch of a batch with lengths
  normals_eigh      the same covariances through numpy.linalg.eigh (fp64): the truth the restatement is checked against
  angle_between     unsigned angle of two direction fields, without arccos near 1
  sphere_cloud, torus_cloud, random_cloud, lattice_cloud, copies_cloud     deterministic test clouds
  normal_consistency_f64   the normal consistency of two clouds with normals, in numpy, on cloud_ref's nearest neighbours
"""
import numpy as np

import cloud_ref as R

SWEEPS = 6
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))          # (p, q, r): r the third index


# ---- steps 1-2 --------------------------------------------------------------------------------------------------------------------
def knn_keys(x, K, rows=256):
    """x [n, 3] float32 -> keys [n, K] uint64, ascending: the K smallest of bits(d2) << 32 | j over ALL j < n (self included),
    d = x_j - x_i per coordinate, d2 = (dx dx + dy dy) + dz dz in fp32"""
    x = np.ascontiguousarray(x, np.float32)
    n = len(x)
    assert 1 <= K <= n
    out = np.empty((n, K), np.uint64)
    j = np.arange(n, dtype=np.uint64)[None, :]
    cx, cy, cz = x[None, :, 0], x[None, :, 1], x[None, :, 2]
    with np.errstate(all="ignore"):
        for r0 in range(0, n, rows):
            q = x[r0:r0 + rows]
            dx, dy, dz = cx - q[:, 0:1], cy - q[:, 1:2], cz - q[:, 2:3]
            dd = (dx * dx + dy * dy) + dz * dz
            assert dd.dtype == np.float32
            key = (np.ascontiguousarray(dd).view(np.uint32).astype(np.uint64) << np.uint64(32)) | j
            if K < n:
                key = np.partition(key, K - 1, axis=1)[:, :K]
            out[r0:r0 + rows] = np.sort(key, axis=1)
    return out


def key_index(keys):
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ---- step 3 -----------------------------------------------------------------------------------------------------------------------
def covariances(x, idx):
    """x [n, 3] float32, idx [n, K] -> C [n, 3, 3] float64 (symmetric, filled from the 6 unique entries)"""
    x = np.ascontiguousarray(x, np.float32)
    n, K = idx.shape
    s1 = np.zeros((n, 3), np.float64)
    s2 = np.zeros((n, 3, 3), np.float64)
    with np.errstate(all="ignore"):
        for r in range(K):
            d32 = x[idx[:, r]] - x                              # fp32, candidate minus query
            assert d32.dtype == np.float32
            d = d32.astype(np.float64)
            s1 = s1 + d
            for a in range(3):
                for b in range(a, 3):
                    s2[:, a, b] = s2[:, a, b] + d[:, a] * d[:, b]
        k = np.float64(K)
        m = s1 / k
        C = np.zeros((n, 3, 3), np.float64)
        for a in range(3):
            for b in range(a, 3):
                C[:, a, b] = s2[:, a, b] / k - m[:, a] * m[:, b]
                C[:, b, a] = C[:, a, b]
    return C


# ---- step 4 -----------------------------------------------------------------------------------------------------------------------
def jacobi_f64ops(C, sweeps=SWEEPS):
    """C [n, 3, 3] float64 symmetric -> (diag [n, 3], V [n, 3, 3] with eigenvectors in columns, off [n]: largest |off-diagonal|
    left).  Only the upper triangle is carried, as the kernel does."""
    A = np.array(C, np.float64)
    n = len(A)
    V = np.zeros((n, 3, 3), np.float64)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0

    def get(a, b):
        return A[:, min(a, b), max(a, b)]

    def put(a, b, v):
        A[:, min(a, b), max(a, b)] = v

    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q, r in PAIRS:
                app, aqq, apq, arp, arq = get(p, p).copy(), get(q, q).copy(), get(p, q).copy(), get(r, p).copy(), get(r, q).copy()
                on = apq != 0.0
                theta = (aqq - app) / (2.0 * apq)
                root = np.sqrt(theta * theta + 1.0)
                t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + root)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                tapq = t * apq
                put(p, p, np.where(on, app - tapq, app))
                put(q, q, np.where(on, aqq + tapq, aqq))
                put(p, q, np.where(on, 0.0, apq))
                put(r, p, np.where(on, c * arp - s * arq, arp))
                put(r, q, np.where(on, s * arp + c * arq, arq))
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(on[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(on[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    diag = np.stack((A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]), 1)
    off = np.max(np.abs(np.stack((A[:, 0, 1], A[:, 0, 2], A[:, 1, 2]), 1)), 1)
    return diag, V, off


# ---- steps 5-6 --------------------------------------------------------------------------------------------------------------------
def sorted_pairs(diag, V):
    """stable ascending sort of (lambda, column) -> (lam [n, 3] float64, vec [n, 3, 3] float64 with vec[:, :, k] the k-th column)"""
    order = np.argsort(diag, axis=1, kind="stable")
    lam = np.take_along_axis(diag, order, 1)
    vec = np.take_along_axis(V, order[:, None, :], 2)
    return lam, vec


def canonical_sign(nrm):
    """nrm [n, 3] float32 -> negated as a whole where the component of largest magnitude (lowest axis on a tie) is negative"""
    pick = np.argmax(np.abs(nrm), axis=1)                       # the first maximum: the lowest axis on a tie
    big = nrm[np.arange(len(nrm)), pick]
    return np.where((big < 0)[:, None], -nrm, nrm)


# ---- steps 1-7 --------------------------------------------------------------------------------------------------------------------
def normals_f64ops(x, K, keys=None, full=False):
    """x [n, 3] float32 -> (normals [n, 3] float32, eigenvalues [n, 3] float32, idx [n, K] int64).  ``keys``: the knn_keys of x
    for a K' >= K (their first K columns are the neighbourhood).  ``full``: also the fp64 (lam, vec, C, off)."""
    x = np.ascontiguousarray(x, np.float32)
    keys = knn_keys(x, K) if keys is None else keys[:, :K]
    idx = key_index(keys)
    C = covariances(x, idx)
    diag, V, off = jacobi_f64ops(C)
    lam, vec = sorted_pairs(diag, V)
    with np.errstate(all="ignore"):
        nrm = canonical_sign(vec[:, :, 0].astype(np.float32))
        ev = lam.astype(np.float32)
    if full:
        return nrm, ev, idx, (lam, vec, C, off)
    return nrm, ev, idx


def normals_batch(x, K, lengths=None):
    """x [B, N, 3] -> (normals [B, N, 3], eigenvalues [B, N, 3], idx [B, N, K]); rows at or beyond lengths[b]: 0, 0, -1"""
    x = np.ascontiguousarray(x, np.float32)
    B, N = x.shape[:2]
    nrm, ev, idx = np.zeros((B, N, 3), np.float32), np.zeros((B, N, 3), np.float32), np.full((B, N, K), -1, np.int64)
    for b in range(B):
        n = N if lengths is None else int(lengths[b])
        nrm[b, :n], ev[b, :n], idx[b, :n] = normals_f64ops(x[b, :n], K)
    return nrm, ev, idx


def normals_eigh(C):
    """C [n, 3, 3] float64 -> (lam [n, 3] ascending, normal [n, 3] float64 unit, unsigned) by numpy.linalg.eigh"""
    lam, vec = np.linalg.eigh(C)
    return lam, vec[:, :, 0]


def angle_between(a, b):
    """unsigned angle in radians between the directions a, b [n, 3] (any length, any sign): atan2(|a x b|, |a . b|), accurate
    down to angles of 1e-16 where arccos of a dot product near 1 is not"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


# ---- clouds -----------------------------------------------------------------------------------------------------------------------
def sphere_cloud(n, seed=0):
    """n seeded points on the unit sphere; the analytic normal of a point is the point"""
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def torus_cloud(n, seed=0, R0=0.7, r0=0.25):
    """n seeded points on the torus of radii R0, r0 about z -> (points float32, analytic unit normals float64)"""
    g = np.random.default_rng(seed)
    v = g.uniform(0, 2 * np.pi, n)                              # the angle about the tube first, then the one about z
    u = g.uniform(0, 2 * np.pi, n)
    p = np.stack(((R0 + r0 * np.cos(v)) * np.cos(u), (R0 + r0 * np.cos(v)) * np.sin(u), r0 * np.sin(v)), 1)
    nrm = np.stack((np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)), 1)
    return p.astype(np.float32), nrm


def random_cloud(n, seed=0):
    return np.random.default_rng(seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def lattice_cloud(n, seed=0):
    """n distinct points of the integer lattice {0 .. s-1}^3 / 8 with s = max(8, ceil(cbrt n)), in a seeded order: every fp32
    squared distance is exact and most neighbourhood boundaries are exact ties.  n = 512 is the whole 8^3 lattice."""
    s = 8
    while s ** 3 < n:
        s += 1
    g = np.arange(s, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) / np.float32(8)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(len(p))[:n]])


def copies_cloud(m, copies=5, seed=0):
    """m seeded points, each ``copies`` times, in a seeded order: every neighbourhood starts with ties at d2 = 0"""
    p = np.repeat(random_cloud(m, seed), copies, axis=0)
    return np.ascontiguousarray(p[np.random.default_rng(seed + 1).permutation(len(p))])


def make_cloud(family, n, seed=0):
    if family == "random":
        return random_cloud(n, seed)
    if family == "torus":
        return torus_cloud(n, seed)[0]
    if family == "lattice":
        return lattice_cloud(n, seed)
    if family == "sphere":
        return sphere_cloud(n, seed)
    raise ValueError(family)


def case_cloud(family, n):
    """the cloud of a (family, size) case of tests/test_gpu_cloudnormals.py"""
    return make_cloud(family, n, seed=n)


def boundary_ties(x, K):
    """share of the points whose K-th and (K+1)-th candidates have the same d2: the neighbourhood is decided by the index"""
    keys = knn_keys(x, K + 1)
    return float(((keys[:, K - 1] >> np.uint64(32)) == (keys[:, K] >> np.uint64(32))).mean())


# ---- normal consistency -----------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    l = np.sqrt((v * v).sum(1, keepdims=True))
    with np.errstate(all="ignore"):
        return np.where(l > 0, v / np.where(l > 0, l, 1.0), 0.0)


def normal_consistency_f64(a, na, b, nb, oriented=False):
    """a [Na, 3], b [Nb, 3] float32 with normals -> (nc_ab, nc_ba, nc): the fp64 means of |<n, n'>| (the signed dot when
    ``oriented``) between every point's unit normal and that of its nearest neighbour (cloud_ref.nn_f32) in the other cloud"""
    ua, ub = _unit(na), _unit(nb)
    _, iab = R.nn_f32(a, b)
    _, iba = R.nn_f32(b, a)
    dab, dba = (ua * ub[iab]).sum(1), (ub * ua[iba]).sum(1)
    if not oriented:
        dab, dba = np.abs(dab), np.abs(dba)
    ab, ba = float(dab.mean()), float(dba.mean())
    return ab, ba, (ab + ba) / 2
