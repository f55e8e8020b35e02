"""The top-k eigensolver on the GPU (csrc/eig.hip, eigen.py, pca.PCA(solver='subspace'); DESIGN.md 8v "The subspace solver") against
tests/eig_ref.py and tests/pca_ref.py: every device operation within the bound its contract gives, exact on small integers, the same
bits twice; whole fits against the full solver and the float64 oracle; and the layers above down to the command line.

Largest observed error / bound over OP_SHAPES and apply at (6144, 320) (profiles/r39_pca_subspace.txt has the run): apply 0.0064, gram
0.0152, mix 0.02, residual 0.0186; 0 at several shapes, where the result equals the BLAS's in every bit.  Whole fits: eigenvalues
against the full solver 3e-14 ... 5e-11 of a bound of 2e-8 ... 1e-6, the span outside the full solver's 1e-7 ... 2e-7 of a bound of 1e-6
... 1e-5."""
import numpy as np
import pytest

import eig_ref as E
import pca_ref as R
from l3embedding_amd import _lib, cli_pca, eigen, pca

pytestmark = pytest.mark.gpu

FULL_RANK, rows_of = E.FULL_RANK, E.rows_of
OP_SHAPES = [(96, 40), (130, 52), (515, 82), (1024, 96), (2048, 320)]
EXACT_SHAPES = [(130, 52), (515, 82)]
FIT_CASES = FULL_RANK + ['rank20', 'rank39']
U32 = R.U
TOL = 1e-9


def case_id(c):
    return c if isinstance(c, str) else '%d-%d-%d' % c


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def symmetric(rng, D):
    A = rng.standard_normal((D, D))
    return A + A.T          # (a + b == b + a: equal to its transpose bit for bit)


def share(err, bound):
    return float(np.max(err / np.maximum(bound, 1e-300)))


# ---- 1. every operation against NumpyOps within its bound ------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=OP_SHAPES, ids=lambda s: '%d-%d' % s)
def ops_case(request, gpu_required):
    D, m = request.param
    rng = np.random.default_rng(D + m)
    S, V, W, M, theta = symmetric(rng, D), rng.standard_normal((m, D)), rng.standard_normal((m, D)), rng.standard_normal((m, m)), rng.standard_normal(m)
    h = _lib.Eig(D, m)
    h.set_matrix(S)
    yield dict(D=D, m=m, S=S, V=V, W=W, M=M, theta=theta, h=h)
    h.close()


def test_apply_within_the_bound(ops_case):
    c, h = ops_case, ops_case['h']
    h.set_block('V', c['V'])
    h.apply()
    got = h.get_block('W')
    err, bound = np.abs(got - c['V'] @ c['S']), E.apply_bound(c['S'], c['V'])
    print('apply %s: largest error / bound %.3g' % ((c['D'], c['m']), share(err, bound)))
    assert np.all(err <= bound)
    assert same_bits(h.get_block('V'), c['V'])
    h.apply()
    assert same_bits(h.get_block('W'), got)


def test_gram_within_the_bound_and_symmetric(ops_case):
    c, h = ops_case, ops_case['h']
    h.set_block('V', c['V'])
    h.set_block('W', c['W'])
    for a, b in (('V', 'W'), ('W', 'V'), ('V', 'V'), ('W', 'W')):
        G = h.gram(a, b)
        err, bound = np.abs(G - c[a] @ c[b].T), E.gram_bound(c[a], c[b])
        print('gram(%s, %s) %s: largest error / bound %.3g' % (a, b, (c['D'], c['m']), share(err, bound)))
        assert np.all(err <= bound)
        assert same_bits(h.gram(a, b), G)
        if a == b:
            assert same_bits(G, np.ascontiguousarray(G.T))


def test_mix_within_the_bound_in_place_and_not(ops_case):
    c, h = ops_case, ops_case['h']
    h.set_block('V', c['V'])
    h.set_block('W', c['W'])
    h.mix('V', c['M'], 'W')
    other = h.get_block('W')
    err, bound = np.abs(other - c['M'] @ c['V']), E.mix_bound(c['M'], c['V'])
    print('mix %s: largest error / bound %.3g' % ((c['D'], c['m']), share(err, bound)))
    assert np.all(err <= bound)
    assert same_bits(h.get_block('V'), c['V'])          # the source is left as it is
    h.mix('V', c['M'], 'V')
    assert same_bits(h.get_block('V'), other) and same_bits(h.get_block('W'), other)


def test_residual_within_the_bound(ops_case):
    c, h = ops_case, ops_case['h']
    h.set_block('V', c['V'])
    h.set_block('W', c['W'])
    res = h.residual(c['theta'])
    ref = np.linalg.norm(c['W'] - c['theta'][:, None] * c['V'], axis=1)
    err, bound = np.abs(res - ref), E.residual_bound(c['V'], c['W'], c['theta'])
    print('residual %s: largest error / bound %.3g' % ((c['D'], c['m']), share(err, bound)))
    assert res.shape == (c['m'],) and np.all(err <= bound)
    assert same_bits(h.residual(c['theta']), res)


def test_trace_is_the_ascending_sum(ops_case):
    assert ops_case['h'].trace() == E.NumpyOps(ops_case['S'], 1).trace()


def test_apply_at_the_real_width(gpu_required):
    """(6144, 320): 5 x 96 tiles, the geometry of a fit of framewise embeddings"""
    D, m = 6144, 320
    rng = np.random.default_rng(1)
    S, V = symmetric(rng, D), rng.standard_normal((m, D))
    h = _lib.Eig(D, m)
    h.set_matrix(S)
    h.set_block('V', V)
    h.apply()
    got = h.get_block('W')
    h.close()
    err, bound = np.abs(got - V @ S), E.apply_bound(S, V)
    print('apply (6144, 320): largest error / bound %.3g' % share(err, bound))
    assert np.all(err <= bound)


# ---- 2. exact on small integers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda s: '%d-%d' % s)
def test_small_integers_are_exact(shape, gpu_required):
    """S, V, M and theta of integers in [-8, 8]: every product and every sum is an integer below 2^53, so every operation must equal
    the int64 result whatever the order inside an instruction.  V and M are not symmetric in anything, so a wrong lane map, a swap of
    rows and columns or a tail that reads past D or m shows as a wrong integer."""
    D, m = shape
    rng = np.random.RandomState(D * m)
    A = rng.randint(-8, 9, size=(D, D))
    S = np.triu(A) + np.triu(A, 1).T
    V, M, theta = rng.randint(-8, 9, size=(m, D)), rng.randint(-8, 9, size=(m, m)), rng.randint(-8, 9, size=m)
    h = _lib.Eig(D, m)
    h.set_matrix(S.astype(np.float64))
    h.set_block('V', V.astype(np.float64))
    h.apply()
    W = V @ S
    assert np.array_equal(h.get_block('W'), W.astype(np.float64))
    assert np.array_equal(h.gram('V', 'W'), (V @ W.T).astype(np.float64))
    assert np.array_equal(h.gram('W', 'V'), (W @ V.T).astype(np.float64))
    assert np.array_equal(h.gram('V', 'V'), (V @ V.T).astype(np.float64))
    r = W - theta[:, None] * V
    assert np.array_equal(h.residual(theta.astype(np.float64)), np.sqrt((r * r).sum(axis=1).astype(np.float64)))
    assert h.trace() == float(np.trace(S))
    h.mix('V', M.astype(np.float64), 'W')
    assert np.array_equal(h.get_block('W'), (M @ V).astype(np.float64))
    h.mix('W', M.astype(np.float64), 'W')
    assert np.array_equal(h.get_block('W'), (M @ M @ V).astype(np.float64))
    h.close()


# ---- 3. the matrix: from an l3_pca on the device, and the refusals ----------------------------------------------------------------------------
def test_set_matrix_pca_equals_set_matrix_of_the_download(gpu_required):
    D, m = 130, 20
    X = R.embedding_like(np.random.RandomState(9), 700, D)
    V = np.random.RandomState(10).randn(m, D)
    p = _lib.PCA(D)
    p.set_rows(X)
    a, b = _lib.Eig(D, m), _lib.Eig(D, m)
    with pytest.raises(_lib.L3Error, match='holds no scatter matrix'):
        a.set_matrix_pca(p)
    p.mean()
    S = p.scatter()
    a.set_matrix_pca(p)
    b.set_matrix(S)
    got = []
    for h in (a, b):
        h.set_block('V', V)
        h.apply()
        got.append((h.get_block('W'), h.trace()))
    assert same_bits(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    assert p.scatter(download=False) is None          # S may stay on the device
    a.set_matrix_pca(p)
    a.apply()
    assert same_bits(a.get_block('W'), got[1][0])
    p.mean()          # a new mean voids the scatter matrix
    with pytest.raises(_lib.L3Error, match='holds no scatter matrix'):
        a.set_matrix_pca(p)
    with pytest.raises(ValueError, match='matrix comes first'):
        a.apply()
    for h in (a, b, p):
        h.close()


def test_a_matrix_that_is_not_symmetric_or_not_finite_is_refused_with_the_entry_named(gpu_required):
    D = 70
    S = symmetric(np.random.default_rng(2), D)
    h = _lib.Eig(D, 4)
    bad = S.copy()
    bad[66, 3] = np.nextafter(bad[66, 3], 1e9)
    bad[40, 69] = 0.5
    with pytest.raises(_lib.L3Error, match=r'entry \(3, 66\) differs from entry \(66, 3\)'):
        h.set_matrix(bad)
    bad = S.copy()
    bad[65, 20] = bad[20, 65] = np.inf
    bad[68, 67] = np.nan
    with pytest.raises(_lib.L3Error, match=r'entry \(20, 65\) is not finite'):
        h.set_matrix(bad)
    bad = S.copy()
    bad[5, 5] = np.nan
    with pytest.raises(_lib.L3Error, match=r'entry \(5, 5\) is not finite'):
        h.set_matrix(bad)
    with pytest.raises(ValueError, match='matrix comes first'):
        h.apply()
    h.set_matrix(S)
    h.apply()
    h.close()


# ---- 4. whole fits ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=FIT_CASES, ids=case_id)
def fits(request, gpu_required):
    X, k = rows_of(request.param)
    sub = pca.PCA(k, solver='subspace', keep_covariance=True).fit(X)
    full = pca.PCA(solver='full', keep_covariance=True).fit(X)
    yield dict(case=request.param, X=X, k=k, n=X.shape[0], D=X.shape[1], sub=sub, full=full, ref=R.fit_ref(X))
    sub.close()
    full.close()


def test_subspace_fit_against_the_full_solver_and_the_oracle(fits):
    f, sub, full, ref = fits, fits['sub'], fits['full'], fits['ref']
    n, D, k = f['n'], f['D'], f['k']
    m = eigen.block_width(k, None, D)
    lam, C, info = sub.explained_variance_, sub.covariance_, sub.solver_info_
    assert sub.components_.dtype == np.float32 and sub.components_.shape == (k, D) and lam.dtype == np.float64 and lam.shape == (k,)
    assert sub.n_components_ == k and sub.n_samples_ == n and sub.mean_.dtype == np.float32
    assert np.array_equal(bits(C), bits(full.covariance_))          # one scatter matrix under both solvers
    assert info['converged_at'] == info['products'] and info['residual'] <= TOL
    # (the scatter matrix of the float32 chains is of full rank: its eigenvalues past the rank of the rows are round-off near 1e-7 of
    # the largest, of either sign, which the iteration has to resolve like any others; whether a round refills is not asserted there)
    assert info['refills'] == 0 or isinstance(f['case'], str)
    lam_max = ref['variance'][0]
    kahan = E.kahan_bound(k, TOL, (n - 1) * lam_max, D) / (n - 1)
    # against the full solver: the same matrix, so the Ritz values' bound and LAPACK's own error (inside kahan_bound)
    d_full = np.max(np.abs(lam - full.explained_variance_[:k]))
    # against the float64 oracle: Weyl's term for the covariance, as test_pca_gpu.py has it
    weyl = np.linalg.norm(C - ref['covariance'], 'fro') + D * 2.0 ** -52 * lam_max
    d_ref = np.max(np.abs(lam - ref['variance'][:k]))
    print('fit %s (m = %d): %d products, %d checks, %d refills; |dlam| vs full %.3g (bound %.3g), vs oracle %.3g (bound %.3g)' % (
        case_id(f['case']), m, info['products'], info['checks'], info['refills'], d_full, kahan, d_ref, kahan + weyl))
    assert d_full <= kahan and d_ref <= kahan + weyl
    assert np.all(lam >= 0) and np.all(np.diff(lam) <= 0)
    V = sub.components_.astype(np.float64)
    assert np.max(np.abs(V @ V.T - np.eye(k))) <= 3 * U32
    residual = np.linalg.norm(C @ V.T - V.T * lam[None, :], axis=0)
    print('    largest |V V^T - I| / u %.3g, largest residual / ((2 u + tol) lam_max) %.3g' % (
        np.max(np.abs(V @ V.T - np.eye(k))) / U32, residual.max() / ((2 * U32 + TOL) * lam_max)))
    assert np.all(residual <= (2 * U32 + TOL) * lam_max)
    assert np.array_equal(sub.components_, R.sign_rule(sub.components_))
    # the ratios are the variances over trace / (n - 1).  diag(C) is the diagonal of S over n - 1, rounded, and its sum one more
    # float64 sum of D terms: (D + 3) 2^-53, relatively
    total = float(np.sum(np.diag(C)))
    assert np.all(np.abs(sub.explained_variance_ratio_ - lam / total) <= (D + 3) * 2.0 ** -53 * (lam / total))
    assert np.array_equal(sub.mean_, full.mean_)


def test_subspace_agrees_with_the_full_solvers_within_davis_kahan(fits):
    f, sub, full = fits, fits['sub'], fits['full']
    if isinstance(f['case'], str):
        return          # (a rank-deficient set: the k-th and the (k + 1)-th eigenvalue are both zero, and there is no gap to divide by)
    k = f['k']
    lam_max = full.explained_variance_[0]
    gap = sub.explained_variance_[k - 1] - full.explained_variance_[k]
    assert gap > 0
    Vs, Vf = sub.components_.astype(np.float64), full.components_[:k].astype(np.float64)
    outside = np.linalg.norm(Vs.T - Vf.T @ (Vf @ Vs.T), 'fro')
    bound = np.sqrt(k) * TOL * lam_max / gap + 8 * U32 * np.sqrt(k)
    print('subspace %s: ||(I - P_full) V^T||_F %.3g, bound %.3g' % (case_id(f['case']), outside, bound))
    assert outside <= bound


def test_two_fits_with_one_seed_give_the_same_bits(fits):
    f, sub = fits, fits['sub']
    if f['case'] not in ((700, 130, 20), 'rank39'):
        return          # (one full-rank set and one that refills: the others add nothing)
    again = pca.PCA(f['k'], solver='subspace', random_state=0).fit(f['X'])
    other = pca.PCA(f['k'], solver='subspace', random_state=7).fit(f['X'])
    assert np.array_equal(again.components_.view(np.uint32), sub.components_.view(np.uint32))
    assert np.array_equal(bits(again.explained_variance_), bits(sub.explained_variance_))
    assert again.solver_info_['products'] == sub.solver_info_['products']
    kahan = E.kahan_bound(f['k'], TOL, (f['n'] - 1) * fits['ref']['variance'][0], f['D']) / (f['n'] - 1)
    assert np.all(np.abs(other.explained_variance_ - sub.explained_variance_) <= 2 * kahan)
    again.close()
    other.close()


def test_projection_is_that_of_the_arrays(fits):
    f, sub = fits, fits['sub']
    if f['case'] != (700, 130, 20):
        return
    plain = pca.PCA.from_arrays(sub.mean_, sub.components_, explained_variance=sub.explained_variance_)
    Y = sub.transform(f['X'])
    assert Y.dtype == np.float32 and Y.shape == (f['n'], f['k'])
    assert np.array_equal(Y.view(np.uint32), plain.transform(f['X']).view(np.uint32))
    plain.close()
    white = pca.PCA(f['k'], whiten=True, solver='subspace').fit(f['X'])
    assert np.array_equal(white.scale_, (1.0 / np.sqrt(white.explained_variance_)).astype(np.float32))
    assert np.allclose(white.transform(f['X']).astype(np.float64).var(axis=0, ddof=1), 1.0, rtol=1e-3)
    white.close()


def test_auto_takes_the_solver_its_rule_names(gpu_required):
    X, k = rows_of((600, 1024, 64))
    model = pca.PCA(k, solver='auto').fit(X)
    assert (model.solver_info_ is not None) == (model.solver_for(1024) == 'subspace')
    model.close()
    small = pca.PCA(8, solver='auto').fit(rows_of((300, 96, 8))[0])
    assert small.solver_info_ is None          # D = 96 is below every candidate of AUTO_MIN_D
    small.close()


def test_not_converged_leaves_no_model(gpu_required):
    X, k = rows_of((2051, 515, 50))
    model = pca.PCA(k, solver='subspace', max_iter=2)
    with pytest.raises(eigen.NotConverged, match='after 2 products'):
        model.fit(X)
    assert model.components_ is None and model._h is None
    with pytest.raises(ValueError, match='fit comes first'):
        model.transform(X)


def test_cli_fit_with_the_subspace_solver_then_transform(tmp_path, gpu_required):
    X, k = rows_of((300, 96, 8))
    src = tmp_path / 'F'
    src.mkdir()
    for c in range(3):
        np.savez(src / ('clip%d.npz' % c), X=X[100 * c:100 * (c + 1)], y=np.array(c))
    path = cli_pca.main(['fit', '--features', str(src), '--n-components', str(k), '--out', str(tmp_path / 'm.npz'), '--solver', 'subspace',
                         '--oversample', '24', '--tol', '1e-10', '--max-iter', '200', '--seed', '5'])
    ref = pca.PCA(k, solver='subspace', oversample=24, tol=1e-10, max_iter=200, random_state=5).fit(X)
    loaded = cli_pca.load_model(path)
    assert np.array_equal(loaded.components_.view(np.uint32), ref.components_.view(np.uint32))
    assert np.array_equal(bits(loaded.explained_variance_), bits(ref.explained_variance_))
    out = cli_pca.main(['transform', '--model', path, '--features', str(src), '--out', str(tmp_path / 'G')])
    assert len(out) == 3
    for c in range(3):
        with np.load(tmp_path / 'G' / ('clip%d.npz' % c)) as npz:
            assert np.array_equal(npz['X'].view(np.uint32), ref.transform(X[100 * c:100 * (c + 1)]).view(np.uint32)) and int(npz['y']) == c
    ref.close()
    loaded.close()
