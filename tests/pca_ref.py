"""NumPy float64 oracle of the principal-component kernels (csrc/pca.hip, include/l3hip.h "Principal components") and the
error bounds that follow from their arithmetic.  No library is used, and nothing here is measured: every bound is derived from the
count of roundings the contract names.

u = 2^-24 is the unit roundoff of float32, R = 256 the rows of a float32 chain (L3_PCA_CHAIN).
"""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
R = 256
FILL = 512          # L3_PCA_FILL
MAX_SPLITS = 256    # L3_PCA_MAX_SPLITS


def embedding_like(rng, n, D):
    """ReLU-like, non-negative rows with a large mean, as embeddings are: max(0, randn * geomspace(4, .05, D) + 1), float32"""
    return np.maximum(0.0, rng.randn(n, D) * np.geomspace(4.0, 0.05, D) + 1.0).astype(np.float32)


def mean_ref(X):
    """the column means of the float32 rows in float64"""
    return np.asarray(X, np.float64).mean(axis=0)


def mean_bound(X):
    """|m64 - mean| <= n 2^-53 sum|x| / n per column: a column's sum is n - 1 float64 additions of exactly widened float32 values
    in a fixed order, each with a relative error of 2^-53 of a partial sum that is at most sum|x| (the division adds one rounding of
    the quotient, the reference's own sum its rounding: both are inside the slack between n - 1 and n and the first-order form)"""
    X = np.asarray(X, np.float64)
    return X.shape[0] * U64 * np.abs(X).sum(axis=0) / X.shape[0]


def centred(X, m32):
    """xc = fl32(x - m32): the one float32 subtraction of the staging, exactly widened"""
    return (np.asarray(X, np.float32) - np.asarray(m32, np.float32)[None, :]).astype(np.float64)


def scatter_ref(X, m32):
    """S = sum over the rows of xc xc^T in float64 (D, D).  The rows are taken in blocks of R and the blocks' Gram matrices added in
    order, so an entry has at most min(n, R) + ceil(n / R) float64 roundings."""
    xc = centred(X, m32)
    S = np.zeros((xc.shape[1], xc.shape[1]), np.float64)
    for lo in range(0, xc.shape[0], R):
        S += xc[lo:lo + R].T @ xc[lo:lo + R]
    return S


def scatter_bound(X, m32, chain=R):
    """|S_lib - scatter_ref| <= gamma_R sum_rows |xc_i xc_j| + n 2^-53 sum_rows |xc_i xc_j|, elementwise, gamma_R = R u / (1 - R u).

    Within a chain an entry is a sequence of at most R fused multiply-adds, fl(a b + acc): one rounding each, so the chain's result
    differs from its exact sum by at most gamma_R times the sum of its |xc_i xc_j| (the standard bound of a recursive sum of R terms,
    Higham 2002, section 3.1, with the products exact inside the fma).  Summed over the chains that is the first term.  The chains'
    results, exactly widened, are then added in float64: at most 2 ceil(n / R) additions in the library (chains into a split's partial,
    partials into S), each with a relative error of 2^-53 of a partial sum bounded by (1 + gamma_R) sum |xc_i xc_j|; scatter_ref's own
    float64 roundings (above) are of the same kind.  Together they stay below n roundings for n < R (the library then adds nothing) and
    for n >= 263, which is every n the tests use; the term is eight orders of magnitude below the first."""
    xc = np.abs(centred(X, m32))
    mag = xc.T @ xc
    gamma = chain * U / (1.0 - chain * U)
    return gamma * mag + xc.shape[0] * U64 * mag


def gram_exact(rows_int, c_int):
    """the int64 Gram matrix of the integer rows centred at the integer vector c: what the scatter must equal when every product
    and sum is exact in float32"""
    xc = np.asarray(rows_int, np.int64) - np.asarray(c_int, np.int64)[None, :]
    return xc.T @ xc


def project_ref(X, m32, W, scale=None):
    """y = xc W^T in float64 with xc = fl32(x - m32), times scale per column when given -> (n, k)"""
    y = centred(X, m32) @ np.asarray(W, np.float64).T
    return y if scale is None else y * np.asarray(scale, np.float64)[None, :]


def project_bound(X, m32, W, scale=None):
    """|y_lib - project_ref| <= (D + 2) u sum_d |xc_d w_d|, elementwise; with a scale that bound times scale, plus 2 u |y|.

    An entry is one chain of D fused multiply-adds over the exactly known xc and w: D roundings, so at most D u sum|xc_d w_d| to first
    order (Jeannerod and Rump 2013 show that n u holds for a recursive sum of n terms without a higher-order factor); the 2 u on top
    covers the float64 reference's own D 2^-53 and the padding's additions of zero, which are exact.  With a scale the library rounds
    the product y scale[c] once: the error of y is scaled, and u |y scale| is added; the second u |y| covers that factor being taken
    at the reference's value instead of the library's."""
    mag = np.abs(centred(X, m32)) @ np.abs(np.asarray(W, np.float64)).T
    bound = (np.asarray(W).shape[1] + 2) * U * mag
    if scale is None:
        return bound
    s = np.asarray(scale, np.float64)[None, :]
    return bound * s + 2.0 * U * np.abs(project_ref(X, m32, W, scale))


def inverse_ref(Y, W, m32, scale=None):
    """x = (y / scale) W + m32 in float64 -> (n, D)"""
    z = np.asarray(Y, np.float64)
    if scale is not None:
        z = z / np.asarray(scale, np.float64)[None, :]
    return z @ np.asarray(W, np.float64) + np.asarray(m32, np.float64)[None, :]


def inverse_bound(Y, W, m32, scale=None):
    """|x_lib - inverse_ref| for the SAME float32 Y on both sides.  z = fl32(y / scale) differs from y / scale by u |z|, which the chain
    carries as u sum_c |z_c w_cd|; the chain over the k components has (k + 2) u sum_c |z_c w_cd| as in project_bound; the last
    addition of the mean rounds once, u |x| with |x| at most the reference's plus the chain's error, and is exact for a zero mean."""
    z = np.abs(np.asarray(Y, np.float64))
    if scale is not None:
        z = z / np.asarray(scale, np.float64)[None, :]
    k = np.asarray(W).shape[0]
    mag = z @ np.abs(np.asarray(W, np.float64))
    chain = ((k + 2) + (1 if scale is not None else 0)) * U * mag
    if not np.any(np.asarray(m32)):
        return chain
    return chain + U * (np.abs(inverse_ref(Y, W, m32, scale)) + chain)


def sign_rule(components):
    """each row with its entry of largest magnitude positive; among equal magnitudes the lowest index decides"""
    w = np.array(components, copy=True)
    for c in range(w.shape[0]):
        a = np.abs(w[c])
        first = int(np.flatnonzero(a == a.max())[0])
        if w[c, first] < 0:
            w[c] = -w[c]
    return w


def eigen_ref(C):
    """eigh of the symmetric float64 matrix C, eigenvalues descending and clipped at 0, components as rows under the sign rule"""
    lam, vec = np.linalg.eigh(np.asarray(C, np.float64))
    order = np.argsort(-lam, kind='stable')
    return np.maximum(lam[order], 0.0), sign_rule(vec[:, order].T)


def fit_ref(X):
    """the full-float64 fit of the rows -> dict of mean, covariance (np.cov of the float64 rows), variance (D, descending),
    components (D, D) as rows, ratio"""
    X = np.asarray(X, np.float64)
    C = np.atleast_2d(np.cov(X, rowvar=False))
    variance, components = eigen_ref(C)
    total = variance.sum()
    return dict(mean=X.mean(axis=0), covariance=C, variance=variance, components=components,
                ratio=variance / total if total > 0 else np.zeros_like(variance))


def count_for_ref(ratio, share):
    """the fewest leading components whose ratios sum to at least `share` (a plain loop)"""
    total = 0.0
    for c, r in enumerate(ratio):
        total += r
        if total >= share:
            return c + 1
    return len(ratio)


def splits_ref(n, D):
    """the count that splits = 0 stands for, as include/l3hip.h states it: max(1, min(C, L3_PCA_MAX_SPLITS, floor(L3_PCA_FILL / U))), C = ceil(n
    / 256), T = ceil(D / 128), U = T (T + 1) / 2"""
    C, T = -(-n // R), -(-D // 128)
    tiles = T * (T + 1) // 2
    return max(1, min(C, MAX_SPLITS, FILL // tiles))


def split_ranges(n, splits):
    """the row ranges of the splits, as include/l3hip.h states them: split s is the chains [floor(s C / S), floor((s + 1) C / S)) with
    S = min(splits, C), chain c the rows [256 c, min(n, 256 (c + 1)))"""
    C = -(-n // R)
    S = min(splits, C)
    return [(R * (s * C // S), min(n, R * ((s + 1) * C // S))) for s in range(S)]
