"""CPU tests of the t-SNE read-out (tsne.py, csrc/tsne.hip's contract): the NumPy oracle against plain loops and a
finite difference of its own KL, the entropy the calibration reaches, the symmetrisation against the dense (P + P^T) / 2n, the
geometry function, the recorded scikit-learn bars (tests/golden/tsne_golden.npz, written by tests/golden/make_tsne_golden.py), the
binding table, the refusals that come before the device, pickling and the command line's parser."""
import math
import os
import pickle
import re

import numpy as np
import pytest

import tsne_ref as R
from l3embedding_amd import _lib, cli_tsne, tsne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'tsne_golden.npz')
SYMBOLS = ['l3_op_tsne_conditional', 'l3_tsne_geometry', 'l3_tsne_create', 'l3_tsne_destroy', 'l3_tsne_set_affinities', 'l3_tsne_set_embedding',
           'l3_tsne_get_embedding', 'l3_tsne_run', 'l3_tsne_time', 'l3_op_tsne_repulsive', 'l3_op_tsne_attractive', 'l3_op_tsne_update']


def lists(n, k, seed):
    rng = np.random.RandomState(seed)
    X = rng.randn(n, 5)
    return R.knn_lists(X, k)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def test_calibration_equals_the_double_loop():
    rng = np.random.RandomState(0)
    dist = np.sort(rng.gamma(2.0, 3.0, size=(6, 17)).astype(np.float32), axis=1)
    dist[1] = 4.0                                   # equal distances
    dist[2, :5] = 0.0                               # zeros
    dist[3, 1:] = dist[3, 1:] + 1e4                 # one near, many far
    dist[4] = dist[4] * np.float32(1e30)            # the subtraction of the minimum matters
    p, beta = R.conditional_ref(dist, 5.0)
    for i in range(len(dist)):
        pl, bl = R.conditional_loop(dist[i], 5.0)          # math.exp and np.exp may differ in the last place
        assert abs(bl - beta[i]) <= 1e-12 * beta[i] and np.max(np.abs(pl - p[i])) <= 1e-12
    assert np.array_equal(p[1], np.full(17, 1.0 / 17)) and beta[1] == 2.0 ** 100
    assert np.allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize('perplexity', [2.0, 5.0, 20.0])
def test_entropy_is_the_log_of_the_perplexity_after_100_steps(perplexity):
    _, dist = lists(80, 61, 3)
    p, beta = R.conditional_ref(dist, perplexity)
    assert np.all(beta > 0) and np.all(np.isfinite(beta))
    assert np.max(np.abs(R.entropy(p) - math.log(perplexity))) < 1e-12


def test_symmetrisation_equals_the_dense_matrix():
    n, k = 40, 7
    idx, dist = lists(n, k, 5)
    p, _ = R.conditional_ref(dist, 3.0)
    indptr, cols, vals = tsne.joint_affinities(idx, p)
    assert indptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float32
    P = R.joint_dense(idx, p)
    want = R.csr_of(P)
    assert np.array_equal(indptr, want[0]) and np.array_equal(cols, want[1]) and np.array_equal(vals, want[2])
    D = R.dense_of(indptr, cols, vals, n)
    assert np.array_equal(D, D.T) and abs(D.sum() - 1.0) < 1e-6 and np.all(np.diag(D) == 0)
    _lib.tsne_check_csr(n, indptr, cols, vals)          # sorted, in range, no diagonal
    idx2 = idx.copy()
    idx2[0, 1] = idx2[0, 0]
    with pytest.raises(ValueError, match='twice'):
        tsne.joint_affinities(idx2, p)
    with pytest.raises(ValueError, match='itself'):
        tsne.joint_affinities(np.zeros((3, 1), np.int32), np.ones((3, 1)))


def test_gradient_is_the_derivative_of_the_kl():
    n = 12
    rng = np.random.RandomState(1)
    idx, dist = lists(n, n - 1, 2)
    p, _ = R.conditional_ref(dist, 4.0)
    P = R.joint_dense(idx, p)
    Y = rng.randn(n, 2)
    g = R.gradient_of_map(Y, P)
    h = 1e-6
    for i in range(n):
        for c in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, c] += h
            Ym[i, c] -= h
            fd = (R.kl_of_map(Yp, P) - R.kl_of_map(Ym, P)) / (2 * h)
            assert abs(fd - g[i, c]) < 1e-7 * max(1.0, abs(g[i, c]))


def test_passes_of_the_oracle_agree_with_its_gradient_and_kl():
    n = 30
    idx, dist = lists(n, 10, 4)
    p, _ = R.conditional_ref(dist, 3.0)
    P = R.joint_dense(idx, p)
    Y = np.random.RandomState(2).randn(n, 2).astype(np.float32)
    rep, att = R.repulsive_ref(Y), R.attractive_ref(Y, P)
    Z = rep['z'].sum()
    assert np.allclose(4.0 * (att['A'] - rep['R'] / Z), R.gradient_of_map(Y.astype(np.float64), P), rtol=1e-12, atol=1e-15)
    plogp = float((P[P > 0] * np.log(P[P > 0])).sum())
    # the identity behind the records: exact with the weight sum P on log Z; the float32 entries sum to 1 within their rounding
    assert abs(plogp + att['kl'].sum() + P.sum() * math.log(Z) - R.kl_ref(Y, P)) < 1e-12
    assert abs(P.sum() - 1.0) < 1e-6 and abs(plogp + att['kl'].sum() + math.log(Z) - R.kl_ref(Y, P)) < 1e-6 * math.log(Z)
    sub = R.repulsive_ref(Y, rows=[3, 29])
    assert np.array_equal(sub['R'], rep['R'][[3, 29]]) and np.array_equal(sub['z'], rep['z'][[3, 29]])
    bR, bz = R.repulsive_bound(rep, n)
    assert np.all(bR > 0) and np.all(bz > 0) and np.all(bz < 1e-4 * rep['z'])


def test_update_rules():
    f = np.float32
    y, u, gains = np.zeros((4, 2), f), np.array([[1, -1], [0, 1], [1, 1], [-1, 0]], f), np.array([[1, 1], [1, 1], [0.011, 0.011], [1, 1]], f)
    A = np.array([[1, 1], [1, 0], [1, 1], [1, 1]], np.float64)
    y2, u2, g2 = R.update_ref(y, u, gains, A, np.zeros((4, 2)), 1.0, 1.0, 0.5, 1.0)
    # g = 4 A: u g < 0 only for (0, 1); a zero product (zero update or zero gradient) is not an increase; the floor holds
    assert g2[0, 1] == f(1.2) and g2[0, 0] == f(0.8) and g2[1, 0] == f(0.8) and g2[1, 1] == f(0.8) and g2[3, 1] == f(0.8)
    assert g2[2, 0] == f(0.01) and y2.dtype == u2.dtype == g2.dtype == f
    assert np.array_equal(u2, (f(0.5) * u - (f(1.0) * g2) * (4.0 * A).astype(f)).astype(f)) and np.array_equal(y2, u2)


def test_run_sum_and_geometry():
    v = np.random.RandomState(0).rand(600)
    assert R.run_sum(v) == (math.fsum([]) + sum([sum(v[:256].tolist(), 0.0), sum(v[256:512].tolist(), 0.0), sum(v[512:].tolist(), 0.0)], 0.0))
    assert R.geometry_ref(1) == (256, 1, 1) and R.geometry_ref(257) == (256, 2, 1) and R.geometry_ref(8192) == (256, 32, 1)
    assert R.geometry_ref(8193) == (1024, 33, 1) and R.geometry_ref(16384) == (1024, 64, 1) and R.geometry_ref(16385) == (1024, 33, 2)
    assert R.geometry_ref(240000) == (1024, 5, 216)
    for n in (1, 256, 257, 8192, 8193, 16384, 16385, 240000):
        assert _lib.tsne_geometry(n) == R.geometry_ref(n)[:2]


def test_golden_bars_are_recorded():
    with np.load(GOLDEN) as npz:
        g = {k: npz[k] for k in npz.files}
    assert g['kl_barnes_hut'].shape == (3, 8) and list(g['datasets']) == [1, 2, 3] and float(g['perplexity']) == 20.0
    assert np.all(g['acc_barnes_hut'] == 1.0) and np.all(g['acc_exact'] == 1.0)
    for a, ds in enumerate(g['datasets']):
        X, labels = R.blobs(int(ds))
        assert X.shape == (300, 16) and X.dtype == np.float32 and float(X.astype(np.float64).sum()) == g['x_sum'][a]
    bar = g['kl_barnes_hut'].mean(axis=1) + 3 * g['kl_barnes_hut'].std(axis=1)
    assert np.all(bar > 0.5) and np.all(bar < 1.5)


# ---- the binding, refusals, pickling, the command line -----------------------------------------------------------------------------------
def test_every_symbol_is_in_the_binding_and_the_header():
    header = open(os.path.join(ROOT, 'include', 'l3hip.h')).read()
    declared = set(re.findall(r'\b(l3_(?:op_)?tsne[a-z_]*)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert declared == set(SYMBOLS)
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
    assert '#define L3_TSNE_RUN 256' in header and _lib.TSNE_RUN == R.RUN == 256
    assert '#define L3_TSNE_SEARCH_STEPS 100' in header and _lib.TSNE_SEARCH_STEPS == R.SEARCH_STEPS == 100


def test_refusals_come_before_the_device():
    """every one of these is a ValueError on a machine without a GPU: nothing reaches the device"""
    d = np.ones((10, 5), np.float32)
    for perplexity in (1.0, 0.5, 5.0, 7.0, float('nan'), True):          # outside (1, k = 5)
        with pytest.raises(ValueError, match='perplexity'):
            _lib.op_tsne_conditional(d, perplexity)
    with pytest.raises(ValueError, match='2 to 64'):
        _lib.op_tsne_conditional(np.ones((10, 65), np.float32), 5.0)
    with pytest.raises(ValueError, match='2 to 64'):
        _lib.op_tsne_conditional(np.ones((10, 1), np.float32), 1.5)
    with pytest.raises(ValueError, match='float32'):
        _lib.op_tsne_conditional(d.astype(np.float64), 2.0)
    with pytest.raises(ValueError, match='at most 64'):
        tsne.TSNE(perplexity=21.5, random_state=0)
    with pytest.raises(ValueError, match='at most 64'):
        tsne.n_neighbors_for(30.0, 1000)
    assert tsne.n_neighbors_for(21.0, 1000) == 64 and tsne.n_neighbors_for(20.0, 1000) == 61 and tsne.n_neighbors_for(19.0, 60) == 58
    assert tsne.n_neighbors_for(21.0, 65) == 64 and tsne.n_neighbors_for(5.0, 10) == 9
    with pytest.raises(ValueError, match='more than'):
        tsne.n_neighbors_for(20.0, 15)
    with pytest.raises(ValueError, match='random_state'):
        tsne.TSNE(init='random')
    with pytest.raises(ValueError, match='init'):
        tsne.TSNE(init='pca', random_state=0)
    with pytest.raises(ValueError, match=r'\(n, 2\)'):
        tsne.TSNE(init=np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match='learning_rate'):
        tsne.TSNE(learning_rate=0.0, random_state=0)
    with pytest.raises(ValueError, match='momentum'):
        tsne.TSNE(momentum=(0.5, 1.0), random_state=0)
    with pytest.raises(ValueError, match='exaggeration_iter'):
        tsne.TSNE(n_iter=10, exaggeration_iter=11, random_state=0)
    with pytest.raises(ValueError, match='float32'):
        tsne.TSNE(perplexity=2.0, random_state=0).fit(np.zeros((10, 4)))
    with pytest.raises(ValueError, match='float32'):
        tsne.TSNE(perplexity=2.0, random_state=0).fit_neighbors(np.zeros((10, 5), np.int32), np.zeros((10, 5)))
    with pytest.raises(ValueError, match='perplexity'):
        tsne.TSNE(perplexity=6.0, random_state=0).fit_neighbors(np.zeros((10, 5), np.int32), d)
    with pytest.raises(ValueError, match='holds 4 points'):
        tsne.TSNE(perplexity=2.0, init=np.zeros((4, 2), np.float32)).fit_neighbors(np.zeros((10, 5), np.int32), d)
    # the CSR
    h = _lib.TSNE(4)
    ok = (np.array([0, 2, 3, 4, 4]), np.array([1, 2, 0, 0]), np.full(4, 0.25, np.float32))          # (row 3 is empty)
    _lib.tsne_check_csr(4, *ok)
    with pytest.raises(ValueError, match='unsorted'):
        h.set_affinities(ok[0], np.array([2, 1, 0, 0]), ok[2])
    with pytest.raises(ValueError, match='unsorted'):
        h.set_affinities(ok[0], np.array([1, 1, 0, 0]), ok[2])
    with pytest.raises(ValueError, match='diagonal'):
        h.set_affinities(ok[0], np.array([0, 2, 0, 0]), ok[2])
    with pytest.raises(ValueError, match='outside'):
        h.set_affinities(ok[0], np.array([1, 4, 0, 0]), ok[2])
    with pytest.raises(ValueError, match='outside'):
        h.set_affinities(ok[0], np.array([1, 2, -1, 0]), ok[2])
    with pytest.raises(ValueError, match='indptr'):
        h.set_affinities(np.array([0, 2, 1, 4, 4]), ok[1], ok[2])
    with pytest.raises(ValueError, match='float32'):
        h.set_affinities(ok[0], ok[1], ok[2].astype(np.float64))
    with pytest.raises(ValueError, match='finite'):
        h.set_affinities(ok[0], ok[1], np.array([0.25, np.nan, 0.25, 0.25], np.float32))
    with pytest.raises(ValueError, match='2-D only'):
        h.set_embedding(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match='come first'):
        h.run(10, 1.0, 0.5, 10.0)
    with pytest.raises(ValueError, match='2-D only'):
        _lib.op_tsne_repulsive(np.zeros((4, 2)))
    with pytest.raises(ValueError, match='momentum'):
        _lib.op_tsne_update(np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32), np.ones((4, 2), np.float32), np.zeros((4, 2)), np.zeros((4, 2)),
                            1.0, 1.0, 1.0, 10.0)
    with pytest.raises(ValueError, match='points'):
        _lib.TSNE(0)
    assert h.h is None          # no handle was ever created


def test_auto_learning_rate_and_the_seeded_init():
    m = tsne.TSNE(random_state=5)
    assert m.learning_rate_for(300) == 50.0 and m.learning_rate_for(240000) == 240000 / 12.0 / 4.0
    assert tsne.TSNE(learning_rate=7, random_state=5).learning_rate_for(300) == 7.0
    y = m.initial_map(9)
    assert y.dtype == np.float32 and np.array_equal(y, (1e-4 * np.random.RandomState(5).standard_normal((9, 2))).astype(np.float32))
    given = np.arange(18, dtype=np.float32).reshape(9, 2)
    assert tsne.TSNE(init=given).initial_map(9) is not None and np.array_equal(tsne.TSNE(init=given).initial_map(9), given)


def test_pickling_keeps_the_map_and_no_handle():
    m = tsne.TSNE(perplexity=5.0, random_state=7)
    m.embedding_ = np.arange(8, dtype=np.float32).reshape(4, 2)
    m._h = object()          # stands for a device handle
    back = pickle.loads(pickle.dumps(m))
    assert back._h is None and np.array_equal(back.embedding_, m.embedding_) and back.random_state == 7 and back.perplexity == 5.0
    m._h = None


def test_cli_parser_and_file_means():
    command, args = cli_tsne.parse_arguments(['fit', '--features', 'a.npz', 'dir', '--perplexity', '15', '--seed', '3', '--out', 'm.npz'])
    assert command == 'fit' and args == dict(features=['a.npz', 'dir'], perplexity=15.0, seed=3, n_iter=1000, exaggeration_iter=250,
                                             early_exaggeration=12.0, metric='sqeuclidean', per_file=False, plot=None, device=0, out='m.npz')
    command, args = cli_tsne.parse_arguments(['fit', '--features', 'a.npz', '--seed', '3', '--out', 'm.npz', '--per-file', '--plot', 'p.png'])
    assert args['per_file'] is True and args['plot'] == 'p.png' and args['perplexity'] == 20.0
    for bad in (['fit', '--features', 'a.npz', '--out', 'm.npz'],                                          # no seed
                ['fit', '--features', 'a.npz', '--seed', '1', '--perplexity', '22', '--out', 'm.npz'],
                ['fit', '--features', 'a.npz', '--seed', '1', '--perplexity', '1', '--out', 'm.npz'],
                ['fit', '--features', 'a.npz', '--seed', '1', '--n-iter', '10', '--exaggeration-iter', '11', '--out', 'm.npz'],
                ['fit', '--seed', '1', '--out', 'm.npz']):
        with pytest.raises(SystemExit):
            cli_tsne.parse_arguments(bad)
    X = np.arange(10, dtype=np.float32).reshape(5, 2)
    means, starts = cli_tsne.file_means(X, np.array([0, 0, 1, 2, 2]))
    assert np.array_equal(starts, [0, 2, 3]) and np.array_equal(means, np.array([[1, 2], [4, 5], [7, 8]], np.float32))
