"""NumPy oracle of the t-SNE kernels (csrc/tsne.hip, include/l3hip.h "t-SNE"): the textbook algorithm in float64 --
calibration, symmetrisation, gradient, KL -- the update in float32 with the kernel's counted roundings, and the derived error bounds
of the two passes.

The bounds are derived from the kernels' operations, not fitted to what they give.  u = 2^-24 is the unit roundoff of float32, v =
2^-53 that of float64; (1 + u)^m - 1 <= 1.01 m u for the m used here.

Repulsive pass, one pair, inputs exact float32 coordinates:
    dx = fl(yi - yj)                       relative error u against the true difference (likewise dy)
    d2 = fmaf(dx, dx, fl(dy dy))           dx^2 carries 2u, fl(dy dy) 3u, the fma's rounding u more: both terms >= 0, so <= 4u
    w  = fl(1 + d2)                        <= 5u
    q  = rcp(w)                            v_rcp_f32 is accurate to 1 ulp = 2u: <= 7u             (the term of z)
    q2 = fl(q q)                           <= 15u
    q2 dx                                  <= 16u (dx's own u); its rounding belongs to the accumulation    (the term of R)
  A run of 256 such terms is a float32 chain (R by fmaf, z by addition): recursive summation of m terms errs by at most m u sum|terms|,
  m = 256.  The run sums enter float64 (at most runs + segments additions of relative error v each).  A reciprocal below the smallest
  normal float32 is flushed: an absolute error of at most 2^-126 in q, and after the product with dx of 2^-126 |dx| in the term of R.
  So   |z - z64| <= (1.01 (7 + 256) u + (runs + 64) v) sum_j q_ij + n 2^-126
       |R - R64| <= (1.01 (16 + 256) u + (runs + 64) v) sum_j |q_ij^2 (y_i - y_j)| + 2^-125 sum_j |y_i - y_j|   per coordinate.

Attractive pass, one entry, float64 from exact float32 inputs:
    dx exact; d2 = fma(dx, dx, fl(dy dy)): 2v; 1 + d2: 3v; 1 / .: 4v; P times: 5v; fma with dx: accumulation.  log1p: the device's is
    taken accurate to 4v (a few ulp), its product with P by fma: accumulation.
  A lane adds ceil(m / 64) terms and the butterfly 6 more levels: (ceil(m / 64) + 6) v sum|terms|.
  So   |A - A64| <= 1.01 (5 + ceil(m / 64) + 6) v sum_j |P_ij q_ij (y_i - y_j)|,  kl likewise with 4 in place of 5.
"""
import math

import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
RUN = 256
SEARCH_STEPS = 100
TINY = 2.0 ** -126


# ---- calibration ------------------------------------------------------------------------------------------------------------------------
def conditional_ref(dist, perplexity, steps=SEARCH_STEPS):
    """(p (n, k), beta (n)) float64: the bracket rule of l3hip.h, all rows at once, every sum over j ascending"""
    d32 = np.asarray(dist, np.float32)
    n, k = d32.shape
    d = d32.astype(np.float64) - d32.min(axis=1).astype(np.float64)[:, None]
    target = math.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)

    def sums(beta):
        sum_p, sum_dp = np.zeros(n), np.zeros(n)
        p = np.empty((n, k))
        with np.errstate(over='ignore', under='ignore', invalid='ignore'):
            for j in range(k):
                p[:, j] = np.exp(-d[:, j] * beta)
                sum_p = sum_p + p[:, j]
                sum_dp = sum_dp + d[:, j] * p[:, j]
        return p, sum_p, sum_dp

    for _ in range(steps):
        _, sum_p, sum_dp = sums(beta)
        H = np.log(sum_p) + beta * sum_dp / sum_p
        up = H > target
        lo, hi = np.where(up, beta, lo), np.where(up, hi, beta)
        with np.errstate(invalid='ignore', over='ignore'):
            beta = np.where(up, np.where(np.isinf(hi), beta * 2.0, (beta + hi) / 2.0), np.where(np.isinf(lo), beta / 2.0, (beta + lo) / 2.0))
    p, sum_p, _ = sums(beta)
    return p / sum_p[:, None], beta


def conditional_loop(drow, perplexity, steps=SEARCH_STEPS):
    """one row by a plain double loop of Python floats: the oracle's own check"""
    drow = [float(v) for v in np.asarray(drow, np.float32)]
    m = min(drow)
    target = math.log(perplexity)
    beta, lo, hi = 1.0, -math.inf, math.inf
    for step in range(steps + 1):
        sum_p = sum_dp = 0.0
        ps = []
        for dj in drow:
            p = math.exp(-(dj - m) * beta)
            ps.append(p)
            sum_p += p
            sum_dp += (dj - m) * p
        if step == steps:
            break
        H = math.log(sum_p) + beta * sum_dp / sum_p
        if H > target:
            lo = beta
            beta = beta * 2.0 if hi == math.inf else (beta + hi) / 2.0
        else:
            hi = beta
            beta = beta / 2.0 if lo == -math.inf else (beta + lo) / 2.0
    return np.array(ps) / sum_p, beta


def entropy(p):
    p = np.asarray(p, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return -np.where(p > 0, p * np.log(p), 0.0).sum(axis=-1)


# ---- P ----------------------------------------------------------------------------------------------------------------------------------
def dense_conditional(idx, p, n):
    C = np.zeros((n, n))
    C[np.arange(n)[:, None], np.asarray(idx)] = p
    return C


def joint_dense(idx, p):
    """(P + P^T) / 2n as a dense float64 matrix, narrowed to float32 values as the library stores them"""
    n = len(idx)
    C = dense_conditional(idx, p, n)
    return ((C + C.T) / (2.0 * n)).astype(np.float32).astype(np.float64)


def csr_of(P):
    """dense -> (indptr int64, cols int32, vals float32) of the entries that are not zero, sorted by (row, column)"""
    P = np.asarray(P)
    r, c = np.nonzero(P)
    indptr = np.zeros(P.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=P.shape[0]), out=indptr[1:])
    return indptr, c.astype(np.int32), P[r, c].astype(np.float32)


def dense_of(indptr, cols, vals, n):
    P = np.zeros((n, n))
    r = np.repeat(np.arange(n), np.diff(indptr))
    P[r, cols] = vals
    return P


# ---- the two passes, float64 -------------------------------------------------------------------------------------------------------------
def repulsive_ref(Y, rows=None, chunk=256):
    """dict of R (m, 2), z (m) and the bound's sums Rabs (m, 2), dabs (m, 2) for the rows `rows` (all) of the map Y against every
    other point: the textbook sums in float64, the term j = i left out"""
    Y = np.asarray(Y, np.float32).astype(np.float64)
    n = len(Y)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    R, z, Rabs, dabs = np.zeros((len(rows), 2)), np.zeros(len(rows)), np.zeros((len(rows), 2)), np.zeros((len(rows), 2))
    for a in range(0, len(rows), chunk):
        i = rows[a:a + chunk]
        with np.errstate(over='ignore', invalid='ignore'):
            d = Y[i, None, :] - Y[None, :, :]
            q = 1.0 / (1.0 + (d * d).sum(axis=2))
            q[np.arange(len(i)), i] = 0.0
            t = (q * q)[:, :, None] * d
        t[np.arange(len(i)), i] = 0.0
        d[np.arange(len(i)), i] = 0.0
        R[a:a + chunk], z[a:a + chunk], Rabs[a:a + chunk], dabs[a:a + chunk] = t.sum(axis=1), q.sum(axis=1), np.abs(t).sum(axis=1), np.abs(d).sum(axis=1)
    return dict(R=R, z=z, Rabs=Rabs, dabs=dabs)


def repulsive_bound(ref, n):
    """(bound of R (m, 2), bound of z (m)) from repulsive_ref's sums, as derived above"""
    runs = (n + RUN - 1) // RUN
    tail = (runs + 64) * V
    return (1.01 * (16 + RUN) * U + tail) * ref['Rabs'] + 2.0 * TINY * ref['dabs'], (1.01 * (7 + RUN) * U + tail) * ref['z'] + n * TINY


def attractive_ref(Y, P):
    """dict of A (n, 2), kl (n) = sum_j P_ij log1p(d_ij^2) and the bound's sums Aabs, of a dense P"""
    Y = np.asarray(Y, np.float32).astype(np.float64)
    d = Y[:, None, :] - Y[None, :, :]
    d2 = (d * d).sum(axis=2)
    t = (P / (1.0 + d2))[:, :, None] * d
    return dict(A=t.sum(axis=1), kl=(P * np.log1p(d2)).sum(axis=1), Aabs=np.abs(t).sum(axis=1), count=(P != 0).sum(axis=1))


def attractive_bound(ref):
    """(bound of A (n, 2), bound of kl (n)) as derived above; kl's terms are >= 0"""
    depth = np.ceil(ref['count'] / 64.0) + 6
    return 1.01 * (5 + depth)[:, None] * V * ref['Aabs'], 1.01 * (4 + depth) * V * ref['kl']


def kl_ref(Y, P):
    """KL(P || Q) of the map in float64"""
    Y = np.asarray(Y, np.float32).astype(np.float64)
    d2 = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    w = 1.0 / (1.0 + d2)
    np.fill_diagonal(w, 0.0)
    Q = w / w.sum()
    m = P > 0
    return float((P[m] * np.log(P[m] / Q[m])).sum())


def kl_of_map(Y64, P):
    """kl_ref for a float64 map (the finite-difference check moves coordinates by less than float32 resolves)"""
    d2 = ((Y64[:, None, :] - Y64[None, :, :]) ** 2).sum(axis=2)
    w = 1.0 / (1.0 + d2)
    np.fill_diagonal(w, 0.0)
    Q = w / w.sum()
    m = P > 0
    return float((P[m] * np.log(P[m] / Q[m])).sum())


def gradient_of_map(Y64, P, exaggeration=1.0):
    """4 (exaggeration A - R / Z) in float64 for a float64 map"""
    d = Y64[:, None, :] - Y64[None, :, :]
    q = 1.0 / (1.0 + (d * d).sum(axis=2))
    np.fill_diagonal(q, 0.0)
    A = ((P * q)[:, :, None] * d).sum(axis=1)
    R = ((q * q)[:, :, None] * d).sum(axis=1)
    return 4.0 * (exaggeration * A - R / q.sum())


# ---- the update, float32 with the kernel's roundings ----------------------------------------------------------------------------------
def update_ref(y, u, gains, A, R, Z, exaggeration, momentum, lr):
    """-> the new (y, u, gains), float32, by the counted roundings of l3hip.h"""
    f = np.float32
    y, u, gains = np.asarray(y, f), np.asarray(u, f), np.asarray(gains, f)
    with np.errstate(all='ignore'):
        g = (4.0 * (float(exaggeration) * np.asarray(A, np.float64) - np.asarray(R, np.float64) / float(Z))).astype(f)
        inc = (u * g) < f(0.0)
        gains = np.where(inc, gains + f(0.2), gains * f(0.8)).astype(f)
        gains = np.where(gains < f(0.01), f(0.01), gains).astype(f)
        step = (f(lr) * gains) * g
        un = (f(momentum) * u - step).astype(f)
        return (y + un).astype(f), un, gains


def run_sum(v):
    """a sum over rows in the run order: runs of 256 summed sequentially from 0.0, the run sums added sequentially"""
    total = 0.0
    for a in range(0, len(v), RUN):
        acc = 0.0
        for x in v[a:a + RUN]:
            acc += float(x)
        total += acc
    return total


def geometry_ref(n):
    """(row_block, segments, runs_per_segment): the function of l3hip.h"""
    row_block = 256 if n <= 8192 else 1024
    runs, row_blocks = -(-n // RUN), -(-n // row_block)
    rps = max(1, -(-(runs * row_blocks) // 1024))
    return row_block, -(-runs // rps), rps


# ---- a whole fit in NumPy (the restatement the quality bar was checked with) -----------------------------------------------------------
def knn_lists(X, k):
    X = np.asarray(X, np.float64)
    d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind='stable')[:, :k]
    return idx.astype(np.int32), np.take_along_axis(d, idx, axis=1).astype(np.float32)


def fit_ref(X, perplexity, seed, n_iter=1000, exaggeration_iter=250, early_exaggeration=12.0, momentum=(0.5, 0.8)):
    """-> (map (n, 2) float32, KL of the last iteration): tsne.TSNE's schedule with float64 sums and the float32 update"""
    n = len(X)
    k = min(n - 1, int(3.0 * perplexity + 1.0))
    idx, dist = knn_lists(X, k)
    p, _ = conditional_ref(dist, perplexity)
    P = joint_dense(idx, p)
    lr = max(n / early_exaggeration / 4.0, 50.0)
    y = (1e-4 * np.random.RandomState(seed).standard_normal((n, 2))).astype(np.float32)
    u, gains = np.zeros_like(y), np.ones_like(y)
    kl = None
    for it in range(n_iter):
        ex, mom = (early_exaggeration, momentum[0]) if it < exaggeration_iter else (1.0, momentum[1])
        if it == exaggeration_iter:          # each phase starts from a zero update and unit gains, as scikit-learn's do
            u, gains = np.zeros_like(y), np.ones_like(y)
        Y = y.astype(np.float64)
        d = Y[:, None, :] - Y[None, :, :]
        q = 1.0 / (1.0 + (d * d).sum(axis=2))
        np.fill_diagonal(q, 0.0)
        A = ((P * q)[:, :, None] * d).sum(axis=1)
        R = ((q * q)[:, :, None] * d).sum(axis=1)
        if it == n_iter - 1:
            kl = kl_ref(y, P)
        y, u, gains = update_ref(y, u, gains, A, R, q.sum(), ex, mom, lr)
    return y, kl


def one_nn_accuracy(Y, labels):
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float((np.asarray(labels)[d.argmin(axis=1)] == np.asarray(labels)).mean())


def blobs(dataset_seed, per=100, dim=16, centres=3):
    """the quality fixture: `centres` Gaussian blobs of `per` points in `dim` dimensions, centres 6 randn"""
    rng = np.random.RandomState(dataset_seed)
    c = 6.0 * rng.randn(centres, dim)
    X = np.concatenate([c[j] + rng.randn(per, dim) for j in range(centres)]).astype(np.float32)
    return X, np.repeat(np.arange(centres), per)
