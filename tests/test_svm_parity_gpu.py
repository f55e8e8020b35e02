"""csrc/svm.hip kernel by kernel against the float64 restatement in tests/svm_ref.py, at the class counts, ragged support-vector
counts and feature widths the sklearn fixtures of test_svm_gpu.py do not reach:

  A  the fused decision launch (svm_decision_kernel + svm_pairs_kernel) with synthetic coefficients against ref.ovo_decision, up to
     64 classes, D with 4 | D, 4 | D but not 8 | D, and neither, in all four input forms (bit-equal with each other); exact
     arithmetic on small integers; one-hot coefficients
  B  test rows that span two row blocks of l3_svm_decision, host-matrix and resident-index form
  C  kernel rows (svm_rows_kernel) at the scalar tails of the MFMA loop
  D  the batched solver on problems of 2 ... 1000 rows in one call: optimality certificate, independence of the batch, rho
  E  SVC at 50 classes: decision values, libsvm's coefficient layout through the certificate of every pair, the vote

Every accuracy bound is the kernel-row bound of test_svm_gpu.py (ref.kernel_rows_bound) carried through the float64 sums, or
float64 round-off; to_kern rounds gamma and coef0 to fp32, so the reference takes the rounded values.  Nothing here needs
sklearn."""
import logging

import numpy as np
import pytest

import svm_ref as ref
from l3embedding_amd import _lib
from l3embedding_amd.svm import SVC

pytestmark = pytest.mark.gpu
LOG = logging.getLogger(__name__)

SV_COUNTS = (33, 0, 100, 1, 32, 31)      # support vectors per class, cycled: every case of 6 or more classes holds all of them


def _say(msg):
    LOG.info(msg)
    print(msg)


def _f32r(v):
    return float(np.float32(v))


def _counts(n_class, shift):
    return [SV_COUNTS[(c + shift) % len(SV_COUNTS)] for c in range(n_class)]


def _rows_blk(D, n_class):
    """the row block of l3_svm_decision (csrc/svm.hip)"""
    blk = min(65536, (64 << 20) // D, (32 << 20) // (n_class * (n_class - 1)))
    return max(32, blk & ~31)


def _forms(Z, x_idx, sv_idx):
    return (('X, SV', dict(X=Z[x_idx], SV=Z[sv_idx])), ('x_idx, sv_idx', dict(x_idx=x_idx, sv_idx=sv_idx)),
            ('X, sv_idx', dict(X=Z[x_idx], sv_idx=sv_idx)), ('x_idx, SV', dict(x_idx=x_idx, SV=Z[sv_idx])))


def _synthetic(seed, n_class, D, n, counts, n_pool=400):
    """a pool of rows drawn as test_kernel_rows_match_float64 draws them, test rows and support vectors picked out of it (with
    repeats, so some test rows are support vectors), randn coefficients with exact zeros, randn rho"""
    r = np.random.RandomState(seed)
    Z = (r.randn(n_pool, D) / np.sqrt(D) * 3).astype(np.float32)
    n_sv = int(sum(counts))
    x_idx = r.randint(0, n_pool, n).astype(np.int32)
    sv_idx = r.randint(0, n_pool, n_sv).astype(np.int32)
    coef = r.randn(n_class - 1, n_sv) * (r.rand(n_class - 1, n_sv) > 0.2)
    rho = r.randn(n_class * (n_class - 1) // 2)
    return Z, x_idx, sv_idx, coef, rho


# ---- A. decision values with synthetic coefficients ----------------------------------------------------------------------------
# kind, degree, n_class, D, n: every kind and poly degree, every class count, every D and every n of the lists meet; the
# support-vector counts per class are SV_COUNTS cycled from the case's number
DECISION_CASES = [
    ('linear', 3, 2, 64, 1), ('linear', 3, 3, 1, 31), ('linear', 3, 10, 7, 32), ('linear', 3, 50, 30, 33),
    ('linear', 3, 64, 515, 1000), ('linear', 3, 50, 6144, 33), ('linear', 3, 64, 36, 32),
    ('poly', 0, 3, 3, 33), ('poly', 1, 10, 36, 31), ('poly', 2, 50, 100, 32), ('poly', 3, 64, 512, 33), ('poly', 5, 2, 515, 1000),
    ('poly', 3, 10, 6144, 1), ('poly', 2, 64, 7, 31), ('poly', 5, 50, 30, 1),
    ('rbf', 3, 2, 1, 33), ('rbf', 3, 3, 30, 1000), ('rbf', 3, 10, 64, 32), ('rbf', 3, 50, 512, 1000), ('rbf', 3, 64, 36, 31),
    ('rbf', 3, 64, 6144, 32), ('rbf', 3, 50, 7, 1), ('rbf', 3, 10, 100, 33), ('rbf', 3, 64, 3, 1000), ('rbf', 3, 2, 515, 32),
    ('sigmoid', 3, 2, 3, 32), ('sigmoid', 3, 3, 515, 31), ('sigmoid', 3, 10, 30, 1), ('sigmoid', 3, 50, 36, 1000),
    ('sigmoid', 3, 64, 100, 33), ('sigmoid', 3, 3, 6144, 32), ('sigmoid', 3, 64, 1, 1000), ('sigmoid', 3, 50, 64, 31),
]


@pytest.mark.parametrize('case', range(len(DECISION_CASES)), ids=['%s%d-c%d-D%d-n%d' % c for c in DECISION_CASES])
def test_decision_matches_float64(gpu_required, case):
    kind, degree, n_class, D, n = DECISION_CASES[case]
    counts = _counts(n_class, case)
    Z, x_idx, sv_idx, coef, rho = _synthetic(1000 + case, n_class, D, n, counts)
    gamma, coef0 = 4.0 / D, 0.5
    kp = _lib.svm_kernel(kind, gamma, coef0, degree)
    cs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    h = _lib.SVM()
    h.set_data(Z)
    got = [(name, h.decision(kp, cs, coef, rho, **kw)) for name, kw in _forms(Z, x_idx, sv_idx)]
    h.close()
    exact, bound = ref.ovo_decision_bound(Z[x_idx], Z[sv_idx], counts, coef, rho, kind, _f32r(gamma), _f32r(coef0), degree)
    if D <= 515:
        assert np.array_equal(exact, ref.ovo_decision(Z[x_idx], Z[sv_idx], counts, coef, rho, kind, _f32r(gamma), _f32r(coef0),
                                                      degree))
    err = np.abs(got[0][1] - exact)
    _say('A %s degree %d, %d classes, D=%d, n=%d, n_sv=%d: max err %.3g, max err / bound %.3g' % (
        kind, degree, n_class, D, n, cs[-1], err.max(), (err / bound).max()))
    assert got[0][1].shape == exact.shape
    assert np.all(err <= bound), float((err / bound).max())
    for name, dec in got[1:]:
        assert np.array_equal(dec, got[0][1]), name


@pytest.mark.parametrize('kind,n_class,D', [('rbf', 3, 30), ('linear', 50, 64), ('poly', 64, 7), ('sigmoid', 2, 512)])
def test_decision_without_support_vectors_is_minus_rho(gpu_required, kind, n_class, D):
    counts = [0] * n_class
    Z, x_idx, sv_idx, coef, rho = _synthetic(7 + D, n_class, D, 33, counts)
    kp = _lib.svm_kernel(kind, 4.0 / D, 0.5, 3)
    h = _lib.SVM()
    h.set_data(Z)
    for name, kw in _forms(Z, x_idx, sv_idx):
        dec = h.decision(kp, np.zeros(n_class + 1, np.int64), coef, rho, **kw)
        assert np.array_equal(dec, np.broadcast_to(-rho, dec.shape)), name
    h.close()


@pytest.mark.parametrize('kind,n_class,D,n', [('linear', 50, 512, 33), ('linear', 64, 30, 1000), ('poly', 64, 512, 31),
                                              ('poly', 50, 7, 32)])
def test_decision_exact_arithmetic(gpu_required, kind, n_class, D, n):
    """x and SV small integers, coefficients and rho multiples of 2^-6: every product and sum is exact in fp32 and in float64
    (|dot| <= 16 D <= 2^13; poly degree 1 with gamma = 2^-3 and coef0 = 0.5 keeps 17 bits), so the GPU equals the reference"""
    r = np.random.RandomState(n_class + D)
    counts = _counts(n_class, D)
    n_sv = int(sum(counts))
    Z = r.randint(-4, 5, (300, D)).astype(np.float32)
    x_idx = r.randint(0, 300, n).astype(np.int32)
    sv_idx = r.randint(0, 300, n_sv).astype(np.int32)
    coef = r.randint(-128, 129, (n_class - 1, n_sv)) / 64.0 * (r.rand(n_class - 1, n_sv) > 0.2)
    rho = r.randint(-128, 129, n_class * (n_class - 1) // 2) / 64.0
    gamma, coef0, degree = 0.125, 0.5, 1
    kp = _lib.svm_kernel(kind, gamma, coef0, degree)
    cs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    exact = ref.ovo_decision(Z[x_idx], Z[sv_idx], counts, coef, rho, kind, gamma, coef0, degree)
    h = _lib.SVM()
    h.set_data(Z)
    for name, kw in _forms(Z, x_idx, sv_idx):
        dec = h.decision(kp, cs, coef, rho, **kw)
        wrong = np.argwhere(dec != exact)
        assert wrong.size == 0, (name, len(wrong), wrong[:5].tolist())
    h.close()


@pytest.mark.parametrize('n_class', [50, 64])
def test_decision_one_hot_coefficients(gpu_required, n_class):
    """one non-zero coefficient coef[r, s] = 1, s a support vector of class c: libsvm reads it for the pair (c, r + 1) when
    r >= c and for the pair (r, c) when r < c, and for no other; rbf, so the value that moves is K(x, sv_s) > 0"""
    D, n = 30, 33
    counts = _counts(n_class, n_class)
    Z, x_idx, sv_idx, _, _ = _synthetic(n_class, n_class, D, n, counts)
    n_sv, R, P = int(sum(counts)), n_class - 1, n_class * (n_class - 1) // 2
    cs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    gamma = 1.0 / D
    kp = _lib.svm_kernel('rbf', gamma)
    K, bK = ref.kernel_rows_bound(Z[x_idx], Z[sv_idx], 'rbf', _f32r(gamma))
    r = np.random.RandomState(5)
    sample = [(0, 0), (R - 1, 0), (0, n_sv - 1), (R - 1, n_sv - 1), (31, int(cs[33])), (32, int(cs[32])), (32, int(cs[34]) - 1)]
    sample += [(int(r.randint(R)), int(r.randint(n_sv))) for _ in range(40)]
    h = _lib.SVM()
    h.set_data(Z)
    worst = 0.0
    for rr, s in sample:
        c = int(np.searchsorted(cs, s, side='right') - 1)
        col = ref.pair_index(c, rr + 1, n_class) if rr >= c else ref.pair_index(rr, c, n_class)
        coef = np.zeros((R, n_sv))
        coef[rr, s] = 1.0
        dec = h.decision(kp, cs, coef, np.zeros(P), x_idx=x_idx, sv_idx=sv_idx)
        moved = np.flatnonzero(np.any(dec != 0, axis=0))
        assert moved.tolist() == [col], (rr, s, c, col, moved.tolist())
        err = np.abs(dec[:, col] - K[:, s])
        assert np.all(err <= bK[:, s] + 1e-12 * K[:, s]), (rr, s)
        worst = max(worst, float((err / bK[:, s]).max()))
    h.close()
    _say('A one-hot, %d classes: %d coefficients, max err / bound %.3g' % (n_class, len(sample), worst))


# ---- B. row blocks ---------------------------------------------------------------------------------------------------------------
def _fill_rows(r, Z, chunk=2048):
    for r0 in range(0, Z.shape[0], chunk):
        Z[r0:r0 + chunk] = r.randn(min(chunk, Z.shape[0] - r0), Z.shape[1]) / np.sqrt(Z.shape[1]) * 3


def _check_chunks(dec, Xrows, SV, counts, coef, rho, kind, gamma, coef0=0.0, degree=3, chunk=2048):
    """|dec - float64| <= bound, the reference evaluated in row chunks -> max err / bound"""
    worst = 0.0
    for r0 in range(0, dec.shape[0], chunk):
        exact, bound = ref.ovo_decision_bound(Xrows(r0, r0 + chunk), SV, counts, coef, rho, kind, gamma, coef0, degree)
        err = np.abs(dec[r0:r0 + chunk] - exact)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (r0, float((err / bound).max()))
    return worst


@pytest.mark.parametrize('n_class,D,per_class', [(64, 8, 2), (2, 6144, 20)], ids=['class-term', 'D-term'])
def test_decision_row_blocks(gpu_required, n_class, D, per_class):
    """n = rows_blk + 33 test rows: the second block's 33 rows (one full tile and a tile of one row) through the offsets of the
    resident-index form and through the re-used staging buffer of the host form"""
    blk = _rows_blk(D, n_class)
    assert blk == ((32 << 20) // (n_class * (n_class - 1)) if n_class == 64 else (64 << 20) // D) & ~31      # the term the case names
    n = blk + 33
    counts = [per_class] * n_class
    n_sv = per_class * n_class
    r = np.random.RandomState(D)
    Z = np.empty((n + n_sv, D), np.float32)       # resident: the test rows, then the support vectors
    _fill_rows(r, Z)
    sv_idx = np.arange(n, n + n_sv, dtype=np.int32)
    x_idx = r.permutation(n).astype(np.int32)
    coef = r.randn(n_class - 1, n_sv)
    rho = r.randn(n_class * (n_class - 1) // 2)
    kind, gamma = 'rbf', 1.0 / D
    kp = _lib.svm_kernel(kind, gamma)
    cs = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    SV = Z[n:]
    h = _lib.SVM()
    h.set_data(Z)
    # resident indices, a permutation: the second block reads x_idx[blk:]
    dec = h.decision(kp, cs, coef, rho, x_idx=x_idx, sv_idx=sv_idx)
    w_idx = _check_chunks(dec, lambda a, b: Z[x_idx[a:b]], SV, counts, coef, rho, kind, _f32r(gamma))
    for a, b in ((0, blk), (blk, n)):
        assert np.array_equal(dec[a:b], h.decision(kp, cs, coef, rho, x_idx=x_idx[a:b], sv_idx=sv_idx)), (a, b)
    del dec
    # host rows: the first n rows of Z as they lie
    dec = h.decision(kp, cs, coef, rho, X=Z[:n], SV=SV)
    w_host = _check_chunks(dec, lambda a, b: Z[a:min(b, n)], SV, counts, coef, rho, kind, _f32r(gamma))
    for a, b in ((0, blk), (blk, n)):
        assert np.array_equal(dec[a:b], h.decision(kp, cs, coef, rho, X=Z[a:b], SV=SV)), (a, b)
    # and both forms on the same rows
    assert np.array_equal(dec[-33:], h.decision(kp, cs, coef, rho, x_idx=np.arange(blk, n, dtype=np.int32), sv_idx=sv_idx))
    h.close()
    _say('B %d classes, D=%d, rows_blk=%d, n=%d: max err / bound %.3g (resident indices), %.3g (host rows)' % (
        n_class, D, blk, n, w_idx, w_host))


# ---- C. kernel rows at the tails -----------------------------------------------------------------------------------------------
TAIL_D = (1, 2, 3, 5, 7, 12, 30, 100, 515, 6145)
TAIL_NA = (1, 32, 128, 129, 300)
TAIL_NB = (1, 31, 33)


@pytest.mark.parametrize('kind', ref.KINDS)
@pytest.mark.parametrize('k', range(len(TAIL_D)), ids=['D%d' % d for d in TAIL_D])
def test_kernel_rows_tails_match_float64(gpu_required, kind, k):
    """test_kernel_rows_match_float64's check and bound where D % 8 != 0: the scalar loads of the last k step (and of every step
    when 4 does not divide D)"""
    D = TAIL_D[k]
    shift = ref.KINDS.index(kind)
    na, nb = TAIL_NA[(k + shift) % len(TAIL_NA)], TAIL_NB[(k + shift) % len(TAIL_NB)]
    r = np.random.RandomState(D + len(kind))
    n_x = 300
    x = (r.randn(n_x, D) / np.sqrt(D) * 3).astype(np.float32)
    a_idx = r.randint(0, n_x, na).astype(np.int32)
    b_idx = r.randint(0, n_x, nb).astype(np.int32)
    gamma, coef0, degree = 1.0 / D * 4, 0.5, 3
    got = _lib.op_svm_kernel_rows(x, a_idx, b_idx, kind, gamma=gamma, coef0=coef0, degree=degree)
    exact, bound = ref.kernel_rows_bound(x[a_idx], x[b_idx], kind, _f32r(gamma), _f32r(coef0), degree)
    err = np.abs(got - exact)
    _say('C %s D=%d, %d x %d: max err %.3g, max err / bound %.3g' % (kind, D, na, nb, err.max(), (err / bound).max()))
    assert got.shape == (na, nb)
    assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize('D', [1, 7, 30, 512, 6145])
def test_rbf_of_a_row_with_itself(gpu_required, D):
    """the distance |u|^2 + |u|^2 - 2 u.u is clamped at 0: K(u, u) <= 1, and within the bound of 1"""
    r = np.random.RandomState(D)
    x = (r.randn(129, D) / np.sqrt(D) * 3).astype(np.float32)
    idx = np.arange(129, dtype=np.int32)
    gamma = 4.0 / D
    got = _lib.op_svm_kernel_rows(x, idx, idx, 'rbf', gamma=gamma)
    exact, bound = ref.kernel_rows_bound(x, x, 'rbf', _f32r(gamma))
    d = np.diag(got).astype(np.float64)
    assert np.all(got <= 1.0)
    assert np.all(np.abs(d - 1.0) <= np.diag(bound)), float((np.abs(d - 1.0) / np.diag(bound)).max())
    _say('C rbf K(u, u) D=%d: min %.9g, max |K - 1| / bound %.3g' % (D, d.min(), (np.abs(d - 1.0) / np.diag(bound)).max()))


@pytest.mark.parametrize('D', [1, 30, 515])
def test_poly_degree_0_is_one(gpu_required, D):
    r = np.random.RandomState(D)
    x = (r.randn(64, D) * 100).astype(np.float32)
    idx = np.arange(64, dtype=np.int32)
    got = _lib.op_svm_kernel_rows(x, idx, idx[:33], 'poly', gamma=4.0 / D, coef0=0.5, degree=0)
    assert np.array_equal(got, np.ones((64, 33), np.float32))


# ---- D. the batched solver on a ragged problem set ---------------------------------------------------------------------------------
SOLVER_SIZES = (2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000)
SOLVER_D = 30
SOLVER_GAMMA = 1.0 / SOLVER_D
_solver_cache = {}


def _solver_set():
    """two overlapping classes in D = 30; balanced problems of SOLVER_SIZES rows on rows of their own, one row against 200, and 40
    rows + the first of them again under the opposite sign (rbf: K_ii + K_jj - 2 K_ij = 0 for that pair)"""
    if 'set' in _solver_cache:
        return _solver_cache['set']
    r = np.random.RandomState(11)
    n_x = 3200
    y = np.arange(n_x) % 2
    centres = r.randn(2, SOLVER_D) * 0.25
    X = (centres[y] + r.randn(n_x, SOLVER_D) / np.sqrt(SOLVER_D) * 2.5).astype(np.float32)
    pos, neg = np.flatnonzero(y == 0).astype(np.int32), np.flatnonzero(y == 1).astype(np.int32)
    problems, o = [], 0

    def take(npos, nneg):
        nonlocal o
        rows = np.concatenate((pos[o:o + npos], neg[o:o + nneg]))
        o += max(npos, nneg)
        return rows, np.concatenate((np.ones(npos, np.int8), -np.ones(nneg, np.int8)))

    for s in SOLVER_SIZES:
        problems.append(take((s + 1) // 2, s // 2))
    problems.append(take(1, 200))
    rows, signs = take(20, 20)
    problems.append((np.concatenate((rows, rows[:1])), np.concatenate((signs, -signs[:1]))))
    assert o <= pos.size
    _solver_cache['set'] = (X, problems)
    return X, problems


def _solver_k32(X, problems, p):
    """the fp32 kernel matrix of problem p as the GPU computes it, in float64"""
    key = ('K', p)
    if key not in _solver_cache:
        rows = problems[p][0]
        _solver_cache[key] = _lib.op_svm_kernel_rows(X, rows, rows, 'rbf', gamma=SOLVER_GAMMA).astype(np.float64)
    return _solver_cache[key]


# q, tol, C: every q meets every tol, every tol every C, every q every C it runs at (q = 2: one pair and one host wait per outer
# iteration, so only the problems of at most 257 rows and C <= 1)
SOLVER_CONFIGS = [(2, 1e-3, 1.0), (2, 1e-5, 1e-3), (16, 1e-3, 100.0), (16, 1e-5, 1.0), (16, 1e-3, 1e-3), (64, 1e-3, 1e-3),
                  (64, 1e-5, 100.0), (64, 1e-3, 1.0), (128, 1e-5, 1e-3), (128, 1e-3, 100.0), (128, 1e-5, 1.0)]


@pytest.mark.parametrize('q,tol,C', SOLVER_CONFIGS)
def test_ragged_batch_certificate_independence_and_rho(gpu_required, q, tol, C):
    X, problems = _solver_set()
    keep = [p for p in range(len(problems)) if q > 2 or problems[p][0].size <= 257]
    probs = [problems[p] for p in keep]
    kp = _lib.svm_kernel('rbf', SOLVER_GAMMA)
    h = _lib.SVM()
    h.set_data(X)
    alphas, rho, upd, outer, gaps = h.fit(kp, probs, cost=C, tol=tol, q=q)
    r_alphas, r_rho, r_upd, r_outer, _ = h.fit(kp, probs[::-1], cost=C, tol=tol, q=q)
    n_free, n_nofree, worst_gap, worst_rho = 0, 0, -np.inf, 0.0
    for k, p in enumerate(keep):
        rows, s = probs[k]
        n, a = rows.size, alphas[k]
        tag = 'q=%d tol=%g C=%g problem %d (%d rows)' % (q, tol, C, p, n)
        # batching independence: alone, and in the reversed set
        a1, rho1, upd1, outer1, _ = h.fit(kp, [probs[k]], cost=C, tol=tol, q=q)
        kr = len(keep) - 1 - k
        assert np.array_equal(a, a1[0]) and np.array_equal(a, r_alphas[kr]), tag
        assert rho[k] == rho1[0] == r_rho[kr], tag
        assert upd[k] == upd1[0] == r_upd[kr] and outer[k] == outer1[0] == r_outer[kr], tag
        # the optimality certificate of test_optimality_certificate_at_scale on the fp32 kernel matrix
        K = _solver_k32(X, problems, p)
        gap, lo, hi, eq = ref.optimality(K, s, a, C)
        assert gap <= tol and lo >= 0 and hi <= 0 and eq <= 1e-9 * max(C * a.sum(), 1e-300), (tag, gap, lo, hi, eq)
        assert gaps[k] < tol, (tag, gaps[k])
        worst_gap = max(worst_gap, gap)
        # rho: calculate_rho on the gradient recomputed from alpha; the solver's own gradient differs by float64 round-off
        y = s.astype(np.float64)
        G = y * (K @ (y * a)) - 1.0
        dist = abs(rho[k] - ref.calculate_rho(a, G, y, C)) / max(1.0, C * n)
        assert dist <= 1e-9, (tag, dist)
        worst_rho = max(worst_rho, dist)
        free = int(((a > 0) & (a < C)).sum())
        n_free += free > 0
        n_nofree += free == 0
    h.close()
    _say('D q=%d tol=%g C=%g: %d problems, worst gap %.3g, rho distance / max(1, C n) %.3g, %d end with free variables, %d with '
         'none; outer %d..%d, updates %d..%d' % (q, tol, C, len(keep), worst_gap, worst_rho, n_free, n_nofree, outer.min(),
                                                 outer.max(), upd.min(), upd.max()))
    # float64 reasoning, checked with ref.solve: at C = 1e-3 every alpha of a balanced problem ends at C (calculate_rho's
    # (ub + lb) / 2 branch); at C = 1 and 100 the larger problems keep free variables (its mean branch)
    if C == 1e-3:
        assert n_nofree > 0
    else:
        assert n_free > 0


# ---- E. the multiclass shell at 50 classes ---------------------------------------------------------------------------------------
def _clusters50(D=512, nc=50, seed=3):
    r = np.random.RandomState(seed)
    per = r.randint(8, 41, nc)
    per[:2] = 8, 40
    y = np.repeat(np.arange(nc), per)
    r.shuffle(y)
    centres = r.randn(nc, D) * 0.25
    X = (centres[y] + r.randn(y.size, D) / np.sqrt(D) * 2.5).astype(np.float32)
    yt = r.randint(0, nc, 300)
    Xt = (centres[yt] + r.randn(300, D) / np.sqrt(D) * 2.5).astype(np.float32)
    return X, y.astype(np.int32), Xt


@pytest.mark.parametrize('kind', ['rbf', 'linear'])
def test_svc_50_classes(gpu_required, kind):
    nc, D, tol, C = 50, 512, 1e-5, 1.0
    X, y, Xt = _clusters50(D, nc)
    m = SVC(kernel=kind, tol=tol, C=C, gamma='auto', decision_function_shape='ovo').fit(X, y)
    gamma = 1.0 / D                                     # a power of two: the same in fp32
    start = np.concatenate(([0], np.cumsum(m.n_support_)))
    assert m.dual_coef_.shape == (nc - 1, m.support_.size) and start[-1] == m.support_.size
    assert np.array_equal(y[m.support_], np.repeat(np.arange(nc), m.n_support_))       # grouped by class
    # decision values from the fitted arrays
    Xall = np.concatenate((Xt, X))
    exact, bound = ref.ovo_decision_bound(Xall, X[m.support_], m.n_support_, m.dual_coef_, -m.intercept_, kind, gamma)
    dec = m.decision_function(Xall)
    err = np.abs(dec - exact)
    assert np.all(err <= bound), float((err / bound).max())
    # libsvm's layout read back: for pair (i, j) class i's alpha is dual_coef_[j - 1] over its support vectors, class j's is
    # -dual_coef_[i]; rows that are no support vectors have alpha 0
    idx = np.arange(y.size, dtype=np.int32)
    K32 = _lib.op_svm_kernel_rows(X, idx, idx, kind, gamma=gamma).astype(np.float64)
    K64 = ref.kernel_matrix(X, X, kind, gamma)
    groups = [np.flatnonzero(y == c) for c in range(nc)]
    worst, worst64, p = -np.inf, -np.inf, 0
    for i in range(nc):
        for j in range(i + 1, nc):
            alpha = np.zeros(y.size)
            alpha[m.support_[start[i]:start[i + 1]]] = m.dual_coef_[j - 1, start[i]:start[i + 1]]
            alpha[m.support_[start[j]:start[j + 1]]] = -m.dual_coef_[i, start[j]:start[j + 1]]
            rows = np.concatenate((groups[i], groups[j]))
            s = np.concatenate((np.ones(groups[i].size), -np.ones(groups[j].size)))
            a = alpha[rows]
            gap, lo, hi, eq = ref.optimality(K32[np.ix_(rows, rows)], s, a, C)
            assert gap <= tol and lo >= 0 and hi <= 0 and eq <= 1e-9 * max(C * a.sum(), 1e-300), (i, j, gap, lo, hi, eq)
            # the intercept belongs to the same pair: rho lies between the bounds the optimal alpha leaves it
            G = s * (K32[np.ix_(rows, rows)] @ (s * a)) - 1.0
            assert abs(-m.intercept_[p] - ref.calculate_rho(a, G, s, C)) <= 1e-9 * max(1.0, C * rows.size), (i, j)
            worst = max(worst, gap)
            worst64 = max(worst64, ref.optimality(K64[np.ix_(rows, rows)], s, a, C)[0])
            p += 1
    # the vote, wherever no pair of the row can change sign within the bound
    sure = np.all(np.abs(exact) > bound, axis=1)
    pred = m.predict(Xall)
    assert np.array_equal(pred[sure], m.classes_[ref.ovo_vote(exact, nc)][sure])
    _say('E %s: %d rows, %d support vectors, decision max err / bound %.3g; worst gap %.3g on the fp32 kernel, %.3g on the exact '
         'one; vote compared on %d of %d rows' % (kind, y.size, m.support_.size, (err / bound).max(), worst, worst64, sure.sum(),
                                                  sure.size))
    assert sure.any()
