"""The k largest eigenpairs of a symmetric positive semi-definite matrix by block subspace iteration ("The subspace
solver").

`top_eigh` is the control flow and the m x m linear algebra (NumPy / LAPACK, float64, on the host); whatever is D long goes through
`ops`: `_lib.Eig` on the GPU (csrc/eig.hip), or any object with the same seven methods, such as the NumPy stand-in of
tests/eig_ref.py.  `ops` holds a symmetric matrix S (D, D) and two blocks 'V' and 'W' of m = k + oversample vectors, the rows of
(m, D) float64 matrices:

    apply()                W_j = S V_j
    gram(a, b)             (m, m): <a_i, b_j>
    mix(src, M, dst)       dst_j = sum_i M[j][i] src_i; dst may be src
    residual(theta)        (m): ||W_j - theta_j V_j||
    get_block(which) / set_block(which, B)
    trace()                (not used here: pca.PCA takes the total variance from it)

and the attributes D and m.  The result is a function of S, k, the other arguments and `random_state`: there is no fallback, and an
iteration that has not converged after `max_iter` products raises NotConverged.
"""
import time

import numpy as np


class NotConverged(RuntimeError):
    """block subspace iteration did not reach `tol` within `max_iter` products.  residual: the largest ||S v_j - theta_j v_j|| over the
    k wanted pairs at the last check, relative to theta_0; products: the products S V done; tol: what was asked for."""

    def __init__(self, residual, products, tol):
        RuntimeError.__init__(self, 'subspace iteration has not converged after %d products: the largest residual is %.3g of the largest '
                                    'eigenvalue, the tolerance %.3g (raise max_iter or oversample, or use the full solver)' % (products, residual, tol))
        self.residual, self.products, self.tol = residual, products, tol


def default_oversample(k):
    return max(32, k // 4)


def block_width(k, oversample, D):
    """m = k + oversample, refused when it exceeds D"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError('k must be an integer >= 1, not %r' % (k,))
    if oversample is None:
        oversample = default_oversample(int(k))
    if isinstance(oversample, bool) or not isinstance(oversample, (int, np.integer)) or oversample < 0:
        raise ValueError('oversample must be None or an integer >= 0, not %r' % (oversample,))
    m = int(k) + int(oversample)
    if m > D:
        raise ValueError('k + oversample = %d + %d exceeds the %d features: a block that wide is the whole space (use the full solver, or a '
                         'smaller oversample)' % (k, oversample, D))
    return m


class _Clock(object):
    """ops with its calls counted and their wall time added up"""

    def __init__(self, ops):
        self.ops, self.seconds, self.calls = ops, 0.0, {}

    def __getattr__(self, name):
        fn = getattr(self.ops, name)

        def timed(*args):
            t0 = time.perf_counter()
            self.calls[name] = self.calls.get(name, 0) + 1
            try:
                return fn(*args)
            finally:
                self.seconds += time.perf_counter() - t0
        return timed


def _refill(ops, which, G, tau, rng, info):
    """the deflate-and-refill path of one orthonormalisation round: the directions of the block whose Gram eigenvalue is above tau
    lambda_max are kept, at unit length; the other rows become fresh random directions orthogonal to them and to each other"""
    lam, U = np.linalg.eigh(G)
    order = np.argsort(-lam, kind='stable')
    lam, U = lam[order], U[:, order]
    keep = int(np.count_nonzero(lam > tau * lam[0])) if lam[0] > 0.0 else 0
    M = np.zeros_like(G)
    M[:keep] = U[:, :keep].T / np.sqrt(lam[:keep])[:, None]
    ops.mix(which, M, which)
    B = ops.get_block(which)
    kept = B[:keep]
    fresh = rng.randn(B.shape[0] - keep, B.shape[1])
    for _ in range(2):
        fresh -= (fresh @ kept.T) @ kept
        fresh = np.linalg.qr(fresh.T)[0].T
    B[keep:] = fresh
    ops.set_block(which, B)
    info['refills'] += 1


def _orthonormalise(ops, src, dst, tau, rng, info):
    """CholeskyQR2: block `dst` = the rows of block `src` orthonormalised.  Two rounds of G = gram, G = L L^T on the host, and a mix by
    L^-1; a round whose factorisation fails or loses a row (below) deflates and refills instead."""
    m = ops.m
    for last in (False, True):
        G = ops.gram(src, src)
        G = 0.5 * (G + G.T)
        target = dst if last else src
        try:
            L = np.linalg.cholesky(G)
            # Two ways for a row to be lost.  Pivot j squared over G[j][j] is the share of row j that is not in the span of the rows
            # before it: below tau the factor's inverse would amplify rounding past what the second round repairs.  And a pivot below
            # tau times the largest row norm is a direction that is null beside the others as far as float64 can tell (the rows past
            # the rank of S).  Rows that are merely short -- W_j = theta_j V_j of a small theta_j after a Rayleigh-Ritz step -- are
            # neither: a graded Gram matrix factors accurately, and such pairs must be left to converge.
            piv2, diag = np.diag(L) ** 2, np.diag(G)
            ok = bool(np.all(piv2 >= tau * diag)) and bool(np.min(piv2) >= tau * tau * np.max(diag))
        except np.linalg.LinAlgError:
            ok = False
        if ok:
            ops.mix(src, np.ascontiguousarray(np.linalg.solve(L, np.eye(m))), target)
        else:
            _refill(ops, src, G, tau, rng, info)
            if target != src:
                ops.mix(src, np.eye(m), target)


def top_eigh(ops, k, oversample=None, tol=1e-9, max_iter=500, check_every=5, random_state=0):
    """-> (theta (k) descending, vectors (k, D) float64 with orthonormal rows, info) of the matrix that `ops` holds.

    info: products (the products S V done), checks (Rayleigh-Ritz steps), refills (orthonormalisation rounds that deflated),
    residual (max over j < k of ||S v_j - theta_j v_j|| / theta_0 at the last check), converged_at (the product at which it was
    met), calls (how often each method of `ops` was called), ops_seconds and host_seconds (wall time inside `ops` and outside it)."""
    D, m = int(ops.D), int(ops.m)
    if block_width(k, oversample, D) != m:
        raise ValueError('ops holds blocks of %d vectors, but k + oversample = %d' % (m, block_width(k, oversample, D)))
    if not tol > 0.0:
        raise ValueError('tol must be positive, not %r' % (tol,))
    if max_iter < 1 or check_every < 1:
        raise ValueError('max_iter and check_every must be at least 1')
    started = time.perf_counter()
    ops = _Clock(ops)
    ops.D, ops.m = D, m
    rng = np.random.RandomState(random_state)
    tau = 1e3 * m * D * 2.0 ** -52
    info = dict(products=0, checks=0, refills=0, residual=None, converged_at=None)

    ops.set_block('V', rng.randn(m, D))
    _orthonormalise(ops, 'V', 'V', tau, rng, info)
    for t in range(1, max_iter + 1):
        ops.apply()
        info['products'] = t
        if t == 1 or t % check_every == 0 or t == max_iter:
            H = ops.gram('V', 'W')
            lam, Q = np.linalg.eigh(0.5 * (H + H.T))
            order = np.argsort(-lam, kind='stable')
            theta, M = lam[order], np.ascontiguousarray(Q[:, order].T)
            ops.mix('V', M, 'V')
            ops.mix('W', M, 'W')
            res = ops.residual(np.ascontiguousarray(theta))
            info['checks'] += 1
            scale = abs(float(theta[0]))
            worst = float(np.max(res[:k]))
            info['residual'] = worst / scale if scale > 0.0 else (0.0 if worst == 0.0 else np.inf)
            if worst <= tol * scale:
                info['converged_at'] = t
                vectors = ops.get_block('V')[:k].copy()
                info['ops_seconds'], info['calls'] = ops.seconds, dict(ops.calls)
                info['host_seconds'] = time.perf_counter() - started - ops.seconds
                return theta[:k].copy(), vectors, info
        if t < max_iter:
            _orthonormalise(ops, 'W', 'V', tau, rng, info)
    raise NotConverged(info['residual'], info['products'], tol)
