"""Yardsticks of the point-cloud metrics (surfd_amd/cloudmetrics.py, csrc/cloudnn.hip).  Neither the code under test nor its
output: numpy / torch-CPU restatements.

  nn_f32            the kernels' pair arithmetic at fp32 in the stated operation order (diff = p - q per coordinate,
                    d2 = (dx dx + dy dy) + dz dz, one rounding per operation) with (d2, index) selection: lower index on ties
  nn_f64            the same mathematics in fp64 (the truth the derived bounds are about)
  mean_f32 / mean_f64, matrix_f32 / matrix_f64     the directed Chamfer means of a pair of clouds / of two sets
  mean_kernel_order, matrix_kernel_order           the same means in the fp64 summation order the kernel documents: its bits
  mmd_cov_f64, one_nna_f64                         the set metrics, written as plain loops
  row_gaps          how clearly every arg-min of a matrix is decided
  shell_cloud, torus_cloud, family, lattice_cloud, random_cloud     deterministic test clouds

`python tests/cloud_ref.py` checks the fp32 restatement against fp64 on this file's own clouds and prints the largest relative
error of a cloud-pair mean in units of u = 2^-24 (tests/test_gpu_cloudmetrics.py quotes it beside its derived bound of 7 u).
"""
import numpy as np
import torch

U = 2.0 ** -24                      # unit roundoff of fp32
MEAN_BOUND = 7 * U                  # derived in tests/test_gpu_cloudmetrics.py (item 6 of the issue), not tuned


# ---- nearest neighbours -----------------------------------------------------------------------------------------------------------
def nn_f32(a, b, rows=512):
    """a [Na, 3], b [Nb, 3] float32 -> (d2 [Na] float32, idx [Na] int64).  numpy evaluates every elementwise operation on its
    own, rounded to float32; argmin returns the first (lowest) index among equal minima."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    d2 = np.empty(len(a), np.float32)
    idx = np.empty(len(a), np.int64)
    bx, by, bz = b[None, :, 0], b[None, :, 1], b[None, :, 2]
    for r0 in range(0, len(a), rows):
        q = a[r0:r0 + rows]
        dx, dy, dz = q[:, 0:1] - bx, q[:, 1:2] - by, q[:, 2:3] - bz
        dd = (dx * dx + dy * dy) + dz * dz
        assert dd.dtype == np.float32
        i = dd.argmin(1)
        idx[r0:r0 + rows] = i
        d2[r0:r0 + rows] = dd[np.arange(len(q)), i]
    return d2, idx


def nn_f64(a, b, rows=1024):
    """a [Na, 3], b [Nb, 3] -> d2 [Na] float64: the squared distance to the nearest point, everything in fp64 (torch on the CPU)"""
    a = torch.from_numpy(np.ascontiguousarray(a)).double()
    b = torch.from_numpy(np.ascontiguousarray(b)).double()
    out = []
    for r0 in range(0, len(a), rows):
        q = a[r0:r0 + rows]
        dd = (q[:, 0:1] - b[None, :, 0]).square_()
        dd += (q[:, 1:2] - b[None, :, 1]).square_()
        dd += (q[:, 2:3] - b[None, :, 2]).square_()
        out.append(dd.min(1).values)
    return torch.cat(out).numpy()


def mean_f32(a, b, tau2=None):
    """(float32(float64 sum of the fp32 restatement's d2 / Na), the count of d2 < tau2 compared in fp32)"""
    d2, _ = nn_f32(a, b)
    mean = np.float32(d2.astype(np.float64).sum() / len(d2))
    return mean, (None if tau2 is None else int((d2 < np.float32(tau2)).sum()))


def mean_f64(a, b):
    return float(nn_f64(a, b).sum() / len(a))


def matrix_f64(A, B):
    """[M, R] float64: mean over the points of A_i of the squared distance to their nearest point of B_j"""
    return np.array([[mean_f64(a, b) for b in B] for a in A], np.float64)


def matrix_f32(A, B, tau2=None):
    """([M, R] float32 means, [M, R] int64 counts or None) of the fp32 restatement"""
    res = [[mean_f32(a, b, tau2) for b in B] for a in A]
    mean = np.array([[r[0] for r in row] for row in res], np.float32)
    return mean, (None if tau2 is None else np.array([[r[1] for r in row] for row in res], np.int64))


def mean_kernel_order(d2):
    """d2 [Na] float32 -> float32: the mean in the summation order csrc/cloudnn.hip documents.  Lane t of 256 adds d2[t::256] in
    ascending order to an fp64 accumulator that starts at 0.0 (a lane whose point lies beyond Na adds 0.0, which changes no
    accumulator: none is -0.0); each wave of 64 lanes reduces by the xor tree with offsets 32, 16, 8, 4, 2, 1, after which all
    64 lanes hold one value (asserted); the four waves are added as ((w0 + w1) + w2) + w3; the sum is divided by float(Na) and
    rounded once to fp32.  The order does not depend on P: for a fixed lane, ascending (tile, p) is ascending index, stride 256."""
    d2 = np.ascontiguousarray(d2, dtype=np.float32)
    assert d2.ndim == 1 and len(d2) >= 1
    na = len(d2)
    rows = -(-na // 256)
    padded = np.zeros(rows * 256, np.float64)
    padded[:na] = d2
    acc = np.zeros(256, np.float64)
    for row in padded.reshape(rows, 256):
        acc = acc + row
    w = acc.reshape(4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lanes ^ o]
    assert (w == w[:, :1]).all()
    total = ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]
    return np.float32(total / float(na))


def matrix_kernel_order(A, B, tau2=None):
    """([M, R] float32 means in the kernel's summation order, [M, R] int64 counts of d2 < float32(tau2) or None), on nn_f32"""
    mean = np.empty((len(A), len(B)), np.float32)
    below = None if tau2 is None else np.empty((len(A), len(B)), np.int64)
    for i, a in enumerate(A):
        for j, b in enumerate(B):
            d2, _ = nn_f32(a, b)
            mean[i, j] = mean_kernel_order(d2)
            if below is not None:
                below[i, j] = int((d2 < np.float32(tau2)).sum())
    return mean, below


def ulp_distance(x, y):
    """|x - y| in units of the last place of float32 numbers of one sign (0 = the same bits)"""
    x = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    y = np.ascontiguousarray(y, np.float32).view(np.int32).astype(np.int64)
    return np.abs(x - y)


# ---- set metrics in fp64, as loops ---------------------------------------------------------------------------------------------------
def mmd_cov_f64(D):
    D = np.asarray(D, np.float64)
    G, R = D.shape
    mmd = sum(min(D[i, j] for i in range(G)) for j in range(R)) / R
    matched = set()
    for i in range(G):
        best = 0
        for j in range(1, R):
            if D[i, j] < D[i, best]:            # strict: a tie keeps the lower index
                best = j
        matched.add(best)
    mmd_smp = sum(min(D[i, j] for j in range(R)) for i in range(G)) / G
    return {"mmd": mmd, "cov": len(matched) / R, "mmd_smp": mmd_smp}


def union_matrix(D_gg, D_rr, D_gr):
    D_gg, D_rr, D_gr = (np.asarray(x, np.float64) for x in (D_gg, D_rr, D_gr))
    return np.block([[D_gg, D_gr], [D_gr.T, D_rr]])


def one_nna_f64(D_gg, D_rr, D_gr):
    U_ = union_matrix(D_gg, D_rr, D_gr)
    G, n = len(D_gg), len(U_)
    ok = []
    for i in range(n):
        best = None
        for j in range(n):
            if j != i and (best is None or U_[i, j] < U_[i, best]):
                best = j
        ok.append((best >= G) == (i >= G))
    ok = np.array(ok)
    return {"acc": int(ok.sum()) / n, "acc_gen": int(ok[:G].sum()) / G, "acc_ref": int(ok[G:].sum()) / (n - G)}


def row_gaps(D, exclude_diagonal=False):
    """per row of D: (second-best - best) / second-best, i.e. by how much, relatively, the row's arg-min is decided"""
    D = np.array(D, np.float64)
    if exclude_diagonal:
        np.fill_diagonal(D, np.inf)
    s = np.sort(D, axis=1)
    return (s[:, 1] - s[:, 0]) / np.maximum(s[:, 1], 1e-300)


# ---- clouds -------------------------------------------------------------------------------------------------------------------------
def shell_cloud(seed, n=2048):
    """n points on an ellipsoid shell with seeded semi-axes in [0.3, 0.9]"""
    g = np.random.default_rng(1000 + seed)
    ax = g.uniform(0.3, 0.9, 3)
    v = g.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * ax).astype(np.float32)


def torus_cloud(seed, n=2048):
    """n points on a torus with seeded radii R in [0.5, 0.7], r in [0.1, 0.3], about a seeded axis"""
    g = np.random.default_rng(2000 + seed)
    R, r = g.uniform(0.5, 0.7), g.uniform(0.1, 0.3)
    u, v = g.uniform(0, 2 * np.pi, n), g.uniform(0, 2 * np.pi, n)
    p = np.stack(((R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)), 1)
    return np.roll(p, seed % 3, axis=1).astype(np.float32)


def family(kind, count, n=2048, first=0):
    make = {"shell": shell_cloud, "torus": torus_cloud}[kind]
    return np.stack([make(first + s, n) for s in range(count)])


def metric_sets(n=2048):
    """(clouds [24, n, 3]: 12 shells then 12 tori, {split name: (indices of the generated set, indices of the reference set)}):
    both sets drawn from the same two families, one family against the other, and a set against its own copy"""
    e, t = list(range(12)), list(range(12, 24))
    splits = {"same": (e[:6] + t[:6], e[6:] + t[6:]), "disjoint": (e, t), "copy": (e[:6] + t[:6], e[:6] + t[:6])}
    return np.concatenate((family("shell", 12, n), family("torus", 12, n))), splits


def split_matrices(D, gi, ri):
    """the symmetric [24, 24] matrix of all clouds -> (D_gr, D_gg, D_rr) of one split"""
    return D[np.ix_(gi, ri)], D[np.ix_(gi, gi)], D[np.ix_(ri, ri)]


def assert_decided(D_gr, D_gg, D_rr, tol=1e-5):
    """every arg-min the set metrics take on these fp64 matrices (rows of D_gr for COV, columns for MMD's matching, rows of the
    union without its diagonal for 1-NNA) is decided by more than `tol` relative: 100 % of the rows, none skipped"""
    gaps = {"gr rows": row_gaps(D_gr), "gr columns": row_gaps(D_gr.T), "union": row_gaps(union_matrix(D_gg, D_rr, D_gr), True)}
    for name, g in gaps.items():
        assert (g > tol).all(), (name, g.min())
    return {k: float(v.min()) for k, v in gaps.items()}


def lattice_cloud(B, N, seed):
    """points on the 1/8 lattice of [-2, 2]^3 (every fp32 squared distance exact; ties everywhere) plus duplicated points, built
    as tests/test_gpu_dgcnn.py builds them"""
    g = torch.Generator().manual_seed(seed)
    side = max(3, int(round((N / 4) ** (1 / 3))))
    p = torch.randint(-side, side + 1, (B, N, 3), generator=g).float() / 8
    if N >= 10:
        dup = torch.randint(0, N, (B, N // 10), generator=g)
        p[torch.arange(B)[:, None], torch.randint(0, N, (B, N // 10), generator=g)] = p[torch.arange(B)[:, None], dup]
    return p.numpy()


def random_cloud(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, N, 3, generator=g) * 2 - 1).numpy()


def wave_order_case():
    """(a [256, 3], b [1, 3], the mean in the kernel's order, the mean of the exact sum): a cloud on which the association of
    the four wave sums decides the fp32 result.  b is the origin, so d2 = x^2 exactly: 4 and 2^-22 in wave 0 (lanes 0 and 1),
    2^-52 twice in wave 2 (lanes 128, 129) and twice in wave 3 (lanes 192, 193).  w0 = 4 + 2^-22, the midpoint of two fp32
    neighbours; w2 = w3 = 2^-51, half an fp64 ulp of w0.  ((w0 + w1) + w2) + w3 absorbs each half ulp in turn (ties to even:
    w0 is an even multiple of 2^-50), the sum stays the midpoint and float32 rounds it to even: mean = 4 / 256.  Any order that
    adds w2 and w3 first, and the exact sum, lie above the midpoint and round up."""
    a = np.zeros((256, 3), np.float32)
    a[0, 0], a[1, 0] = 2.0, 2.0 ** -11
    a[[128, 129, 192, 193], 0] = 2.0 ** -26
    b = np.zeros((1, 3), np.float32)
    kernel_order = np.float32(2.0 ** -6)
    return a, b, kernel_order, np.nextafter(kernel_order, np.float32(1))


def self_check_clouds():
    """the clouds the restatement is checked on: four shells and four tori of 2 048 points, and two odd sizes"""
    c = [shell_cloud(s) for s in range(4)] + [torus_cloud(s) for s in range(4)]
    return c, [shell_cloud(9, 777), torus_cloud(9, 2049)]


def fp32_restatement_error():
    """the largest relative error |mean32 - mean64| / mean64 of a cloud-pair mean over the self-check clouds, in units of u"""
    c, odd = self_check_clouds()
    pairs = [(a, b) for i, a in enumerate(c) for j, b in enumerate(c) if i != j] + [(odd[0], odd[1]), (odd[1], odd[0])]
    worst = 0.0
    for a, b in pairs:
        m32, m64 = float(mean_f32(a, b)[0]), mean_f64(a, b)
        worst = max(worst, abs(m32 - m64) / m64)
    return worst / U, len(pairs)


if __name__ == "__main__":
    err, n = fp32_restatement_error()
    print(f"fp32 restatement vs fp64 on {n} cloud pairs: largest relative error of a mean = {err:.3f} u (bound 7 u)")
    assert err * U < MEAN_BOUND
