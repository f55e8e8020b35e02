"""CPU tests of the top-k eigensolver (eigen.py, DESIGN.md 8v "The subspace solver"): block subspace iteration over the NumPy stand-in of
the device operations (tests/eig_ref.py) against numpy.linalg.eigh, the deflate-and-refill path on rank-deficient rows, the refusal
to return an iteration that has not converged, the refusals of pca.PCA that come before the device, the rule of solver='auto', pickles
from before there was a choice of solver, and the binding table."""
import os
import pickle
import re

import numpy as np
import pytest

import eig_ref as E
import pca_ref as R
from l3embedding_amd import _lib, cli_pca, eigen, pca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_RANK, rows_of, scatter_of = E.FULL_RANK, E.rows_of, E.scatter_of


def solve(X, k, **kw):
    S = scatter_of(X)
    m = eigen.block_width(k, kw.get('oversample'), S.shape[0])
    theta, V, info = eigen.top_eigh(E.NumpyOps(S, m), k, **kw)
    lam = np.sort(np.linalg.eigvalsh(S))[::-1]
    return S, m, theta, V, info, lam


@pytest.mark.parametrize('case', FULL_RANK, ids=lambda c: '%d-%d-%d' % c)
def test_top_eigh_agrees_with_eigh(case):
    X, k = rows_of(case)
    S, m, theta, V, info, lam = solve(X, k)
    D = S.shape[0]
    assert theta.shape == (k,) and V.shape == (k, D) and V.dtype == np.float64
    assert np.all(np.diff(theta) <= 0)
    bound = E.kahan_bound(k, 1e-9, lam[0], D)
    print('%s: %d products, %d checks, residual %.3g, largest |theta - lambda| / bound %.3g' % (
        case, info['products'], info['checks'], info['residual'], np.max(np.abs(theta - lam[:k])) / bound))
    assert np.all(np.abs(theta - lam[:k]) <= bound)
    assert np.max(np.abs(V @ V.T - np.eye(k))) <= 64 * 2.0 ** -53 * m
    assert info['refills'] == 0
    assert info['converged_at'] == info['products'] and info['residual'] <= 1e-9
    assert info['checks'] == 1 + info['products'] // 5          # the first product, then every fifth
    # the pairs are eigenpairs of S: the residual the solver reported is the residual there is
    res = np.linalg.norm(V @ S - theta[:, None] * V, axis=1)
    assert np.all(res <= 1e-9 * lam[0] * (1 + 1e-6) + D * 2.0 ** -52 * lam[0])


@pytest.mark.parametrize('case', ['rank20', 'rank39'])
def test_rank_deficient_rows_take_the_refill_path(case):
    X, k = rows_of(case)
    S, m, theta, V, info, lam = solve(X, k)
    D = S.shape[0]
    rank = 20 if case == 'rank20' else 39
    bound = E.kahan_bound(k, 1e-9, lam[0], D)
    print('%s: %d products, %d refills, residual %.3g' % (case, info['products'], info['refills'], info['residual']))
    assert info['refills'] >= 1
    lead = min(rank, k)
    assert np.all(np.abs(theta[:lead] - lam[:lead]) <= bound)
    assert np.all(lam[:lead] > bound)                      # (the leading ones are not inside the bound of zero: the line above says something)
    assert np.all(np.abs(theta[lead:]) <= bound)           # the others are zero as far as the bound can tell
    assert np.max(np.abs(V @ V.T - np.eye(k))) <= 64 * 2.0 ** -53 * m


def test_an_iteration_that_has_not_converged_is_an_error():
    X, k = rows_of((2051, 515, 50))
    S = scatter_of(X)
    ops = E.NumpyOps(S, eigen.block_width(k, None, 515))
    with pytest.raises(eigen.NotConverged, match='has not converged after 2 products') as caught:
        eigen.top_eigh(ops, k, max_iter=2)
    err = caught.value
    assert isinstance(err, RuntimeError) and err.products == 2 and err.tol == 1e-9 and err.residual > 1e-9


def test_the_solver_is_a_function_of_the_matrix_and_the_seed():
    X, k = rows_of((700, 130, 20))
    a = solve(X, k, random_state=3)
    b = solve(X, k, random_state=3)
    c = solve(X, k, random_state=4)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4]['products'] == b[4]['products']
    assert not np.array_equal(a[3], c[3])
    assert np.all(np.abs(a[2] - c[2]) <= 2 * E.kahan_bound(k, 1e-9, a[5][0], 130))


def test_block_width_and_refusals_of_top_eigh():
    assert eigen.default_oversample(50) == 32 and eigen.default_oversample(256) == 64
    assert eigen.block_width(50, None, 515) == 82 and eigen.block_width(64, 0, 64) == 64
    with pytest.raises(ValueError, match=r'k \+ oversample = 50 \+ 32 exceeds the 60 features.*full solver'):
        eigen.block_width(50, None, 60)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match='k must be'):
            eigen.block_width(bad, None, 100)
    with pytest.raises(ValueError, match='oversample must be'):
        eigen.block_width(5, -1, 100)
    ops = E.NumpyOps(np.eye(40), 12)
    with pytest.raises(ValueError, match='blocks of 12 vectors'):
        eigen.top_eigh(ops, 5, oversample=8)
    with pytest.raises(ValueError, match='tol must be positive'):
        eigen.top_eigh(ops, 5, oversample=7, tol=0.0)


def test_refusals_of_the_subspace_solver_come_before_the_device():
    for bad in (None, 0.9):
        with pytest.raises(ValueError, match="solver='subspace' needs an integer n_components"):
            pca.PCA(bad, solver='subspace')
    with pytest.raises(ValueError, match='solver must be one of'):
        pca.PCA(3, solver='lanczos')
    with pytest.raises(ValueError, match='oversample must be'):
        pca.PCA(3, solver='subspace', oversample=-2)
    with pytest.raises(ValueError, match='tol must be positive'):
        pca.PCA(3, solver='subspace', tol=0.0)
    X = np.zeros((10, 40), np.float32)
    model = pca.PCA(9, solver='subspace')
    with pytest.raises(ValueError, match=r'k \+ oversample = 9 \+ 32 exceeds the 40 features.*full solver'):
        model.fit(X)
    assert model._h is None and model.components_ is None
    with pytest.raises(ValueError, match='exceeds the 1024 vectors of a block'):
        pca.PCA(1000, solver='subspace').fit(np.zeros((10, 8192), np.float32))
    assert pca.PCA(1000, solver='auto').solver_for(16384) == 'full' and pca.PCA(800, solver='auto').solver_for(16384) == 'subspace'
    for D, m in ((0, 1), (8, 9), (8, 0), (2048, 1025), (8, True)):
        with pytest.raises(ValueError, match='must be an integer'):
            _lib.Eig(D, m)
    h = _lib.Eig(8, 3)
    with pytest.raises(ValueError, match='matrix must be float64'):
        h.set_matrix(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError, match='matrix comes first'):
        h.apply()
    with pytest.raises(ValueError, match='matrix comes first'):
        h.trace()
    with pytest.raises(ValueError, match="'V' or 'W'"):
        h.get_block('X')
    with pytest.raises(ValueError, match='a block is float64'):
        h.set_block('V', np.zeros((3, 7)))
    with pytest.raises(ValueError, match='M must be float64'):
        h.mix('V', np.zeros((3, 4)), 'W')
    with pytest.raises(ValueError, match='theta must be'):
        h.residual(np.zeros(4))
    with pytest.raises(ValueError, match='_lib.PCA is needed'):
        h.set_matrix_pca(object())
    with pytest.raises(ValueError, match='holds no scatter matrix'):
        h.set_matrix_pca(_lib.PCA(8))
    assert h.h is None          # no handle was ever created


def test_the_auto_rule():
    lo, hi = pca.AUTO_MIN_D - 1, max(pca.AUTO_MIN_D, 4 * 96)
    assert pca.PCA(64, solver='auto').solver_for(hi) == 'subspace'          # 64 + 32 <= hi // 4
    assert pca.PCA(64, solver='auto').solver_for(lo) == 'full'
    D = max(pca.AUTO_MIN_D, 512)
    assert pca.PCA(D // 4 - 32, solver='auto', oversample=32).solver_for(D) == 'subspace'
    assert pca.PCA(D // 4 - 32, solver='auto', oversample=33).solver_for(D) == 'full'          # one vector too wide
    assert pca.PCA(256, solver='auto').solver_for(4 * 320) == ('subspace' if pca.AUTO_MIN_D <= 1280 else 'full')          # and of 256 is 64
    assert pca.PCA(256, solver='auto').solver_for(4 * 320 - 1) == 'full'
    assert pca.PCA(None, solver='auto').solver_for(16384) == 'full' and pca.PCA(0.9, solver='auto').solver_for(16384) == 'full'
    assert pca.PCA(64).solver_for(16384) == 'full' and pca.PCA(64).solver == 'full'          # the default is today's path
    assert pca.PCA(64, solver='subspace').solver_for(100) == 'subspace'
    assert pca.AUTO_MIN_D in (512, 1024, 2048, 4096, 6144)


def test_old_pickles_load_and_behave_as_full():
    rng = np.random.RandomState(3)
    X = R.embedding_like(rng, 100, 8)
    m64 = R.mean_ref(X)
    model = pca.PCA(3)
    model._finish(100, m64.astype(np.float32), R.scatter_ref(X, m64.astype(np.float32)))
    state = model.__getstate__()
    for name in ('solver', 'oversample', 'tol', 'max_iter', 'random_state', 'solver_info_'):
        del state[name]          # what a pickle written before the solver argument holds
    old = pca.PCA.__new__(pca.PCA)
    old.__setstate__(state)
    assert old.solver == 'full' and old.solver_for(16384) == 'full' and old.oversample is None and old.solver_info_ is None
    assert old.tol == 1e-9 and old.max_iter == 500 and old.random_state == 0
    assert np.array_equal(old.components_, model.components_)
    new = pickle.loads(pickle.dumps(pca.PCA(5, solver='subspace', oversample=9, tol=1e-7, max_iter=40, random_state=2)))
    assert (new.solver, new.oversample, new.tol, new.max_iter, new.random_state) == ('subspace', 9, 1e-7, 40, 2)


def test_cli_flags_of_the_solver():
    command, args = cli_pca.parse_arguments(['fit', '--features', 'a.npz', '--n-components', '50', '--out', 'm.npz', '--solver', 'subspace',
                                             '--oversample', '16', '--tol', '1e-8', '--max-iter', '90', '--seed', '4'])
    assert command == 'fit' and args == dict(features=['a.npz'], n_components=50, whiten=False, device=0, out='m.npz', solver='subspace',
                                             oversample=16, tol=1e-8, max_iter=90, seed=4)
    assert 'solver' not in cli_pca.parse_arguments(['fit', '--features', 'a.npz', '--n-components', '50', '--out', 'm.npz'])[1]
    with pytest.raises(SystemExit):
        cli_pca.parse_arguments(['fit', '--features', 'a.npz', '--n-components', '50', '--out', 'm.npz', '--solver', 'lanczos'])


def test_every_symbol_is_in_the_binding_and_the_header():
    header = open(os.path.join(ROOT, 'include', 'l3hip.h')).read()
    declared = set(re.findall(r'\b(l3_eig_[a-z_0-9]+)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert declared == {'l3_eig_create', 'l3_eig_destroy', 'l3_eig_set_matrix', 'l3_eig_set_matrix_pca', 'l3_eig_trace', 'l3_eig_set_block',
                        'l3_eig_get_block', 'l3_eig_apply', 'l3_eig_gram', 'l3_eig_mix', 'l3_eig_residual', 'l3_eig_time'}
    for s in declared:
        assert s in _lib.SIGNATURES
    assert '#define L3_EIG_MAX_M 1024' in header and _lib.EIG_MAX_M == 1024
    assert '#define L3_EIG_V 0' in header and '#define L3_EIG_W 1' in header and _lib.EIG_BLOCKS == {'V': 0, 'W': 1}
