"""NumPy float64 oracle of the top-k eigensolver's device operations (csrc/eig.hip, include/l3hip.h "Symmetric top-k problems"; DESIGN.md
8v) and the error bounds that follow from their contract.  No library is used and nothing here is measured.

The contract: an entry of apply, gram or mix is one float64 accumulator that takes the K products of its reduction in groups of 4,
ascending; the order inside a group is the hardware's.  Whatever that order, the entry is a sum of K products, each rounded at most
once, added by at most K additions, so with u = 2^-53 and gamma_n = n u / (1 - n u)

    |c - exact| <= gamma_(K + 1) sum |a b|          (Higham 2002, eq. 3.5: any order of summation; one more u for a product that is
                                                     rounded before it is added rather than fused)

The reference itself (`@`, a BLAS) obeys the same bound against the exact value, so |c - ref| <= 2 gamma_(K + 1) sum |a b| is what
a test may assert.
"""
import numpy as np

import pca_ref as R

U64 = 2.0 ** -53


def gamma(n):
    return n * U64 / (1.0 - n * U64)


class NumpyOps(object):
    """the `ops` of eigen.top_eigh by `@`: a symmetric S (D, D) and the blocks 'V' and 'W' (m, D)"""

    def __init__(self, S, m):
        S = np.asarray(S, np.float64)
        if S.ndim != 2 or S.shape[0] != S.shape[1] or not np.array_equal(S, S.T):
            raise ValueError('a symmetric square matrix is needed')
        self.S, self.D, self.m = S, S.shape[0], int(m)
        self.blocks = {'V': np.zeros((self.m, self.D)), 'W': np.zeros((self.m, self.D))}

    def trace(self):
        t = 0.0
        for d in range(self.D):
            t += self.S[d, d]
        return t

    def set_block(self, which, B):
        B = np.asarray(B, np.float64)
        assert B.shape == (self.m, self.D)
        self.blocks[which] = B.copy()

    def get_block(self, which):
        return self.blocks[which].copy()

    def apply(self):
        self.blocks['W'] = self.blocks['V'] @ self.S

    def gram(self, a, b):
        return self.blocks[a] @ self.blocks[b].T

    def mix(self, src, M, dst):
        self.blocks[dst] = np.asarray(M, np.float64) @ self.blocks[src]

    def residual(self, theta):
        return np.linalg.norm(self.blocks['W'] - np.asarray(theta)[:, None] * self.blocks['V'], axis=1)


def apply_bound(S, V):
    """|W_lib - V @ S| elementwise: the library's and the reference's gamma_(D + 1) sum_e |v_e s_de|"""
    return 2.0 * gamma(S.shape[0] + 1) * (np.abs(V) @ np.abs(S))


def gram_bound(A, B):
    """|G_lib - A @ B^T| elementwise, reduction length D"""
    return 2.0 * gamma(A.shape[1] + 1) * (np.abs(A) @ np.abs(B).T)


def mix_bound(M, B):
    """|dst_lib - M @ B| elementwise, reduction length m"""
    return 2.0 * gamma(M.shape[1] + 1) * (np.abs(M) @ np.abs(B))


def residual_bound(V, W, theta):
    """|res_lib - ||W - theta V||| per row.  An entry e = fl(w - fl(theta v)) differs from the exact one by at most u |theta v| + u |e|
    <= 2 u (|w| + |theta v|) =: 2 u a, and so does the reference's; the vector of the library's entries is within 2 u ||a|| of the exact
    vector in norm, and the norm of a D-vector computed in floating point in any order is within (D / 2 + 2) u (1 + small) of its exact
    value relatively (D + 1 roundings on the squares' sum, halved by the root, and the root's own).  Both sides: twice the sum."""
    D = V.shape[1]
    a = np.linalg.norm(np.abs(W) + np.abs(np.asarray(theta)[:, None] * V), axis=1)
    exact = np.linalg.norm(W - np.asarray(theta)[:, None] * V, axis=1)
    return 2.0 * (2.0 * U64 * a + (D / 2.0 + 2.0) * U64 * 1.001 * (exact + 2.0 * U64 * a))


def kahan_bound(k, tol, lam_max, D):
    """|theta_j - lambda_j| for the k converged Ritz values.  The residual matrix R = S V^T - V^T diag(theta) of k orthonormal Ritz
    vectors has ||R||_F <= sqrt(k) max_j ||r_j|| <= sqrt(k) tol lam_max, and k eigenvalues of S lie within ||R||_2 of the k Ritz values
    (Kahan 1967; Parlett, The Symmetric Eigenvalue Problem, theorem 11.5.1); D 2^-52 lam_max covers the reference eigh's own error."""
    return np.sqrt(k) * tol * lam_max + D * 2.0 ** -52 * lam_max


# ---- the row sets of the solver's tests ------------------------------------------------------------------------------------------------
FULL_RANK = [(300, 96, 8), (700, 130, 20), (2051, 515, 50), (600, 1024, 64)]


def rows_of(case):
    """the six row sets of the solver's tests: four of full rank, two whose scatter has a lower rank than the block is wide"""
    if case == 'rank20':
        rng = np.random.RandomState(20)
        return (rng.randn(263, 20) @ rng.randn(20, 96) + 1.0).astype(np.float32), 32
    if case == 'rank39':
        return R.embedding_like(np.random.RandomState(39), 40, 257), 30
    n, D, k = case
    return R.embedding_like(np.random.RandomState(n + D), n, D), k


def scatter_of(X):
    xc = X.astype(np.float64) - X.astype(np.float64).mean(axis=0)
    S = xc.T @ xc
    return 0.5 * (S + S.T)
