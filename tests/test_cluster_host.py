"""CPU tests of the clustering read-out (cluster.py, csrc/kmeans.hip's contract): the NumPy oracle against plain loops, the
tie, NaN and run-order rules, the k-means++ edge rules, the scores against scikit-learn's recorded values
(tests/golden/cluster_golden.npz, written by tests/golden/make_cluster_golden.py), the quality bar of the plain seeding with restarts,
the binding table, the refusals that come before the device, pickling and the command line's parser."""
import os
import pickle
import re

import numpy as np
import pytest

import cluster_ref as R
from l3embedding_amd import _lib, cli_cluster, cluster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'cluster_golden.npz')
MEMBER_COUNTS = (0, 1, 255, 256, 257, 600)
SYMBOLS = ['l3_kmeans_create', 'l3_kmeans_destroy', 'l3_kmeans_set_rows', 'l3_kmeans_set_rows_dev', 'l3_kmeans_set_centroids',
           'l3_kmeans_seed_rows', 'l3_kmeans_seed_pp', 'l3_kmeans_assign', 'l3_kmeans_update', 'l3_kmeans_fit', 'l3_kmeans_get_labels',
           'l3_kmeans_get_centroids', 'l3_kmeans_predict', 'l3_kmeans_predict_dev', 'l3_kmeans_contingency', 'l3_kmeans_file_hist',
           'l3_kmeans_time', 'l3_op_kmeans_step']


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as npz:
        return {k: npz[k] for k in npz.files}


# ---- the oracle against plain loops ----------------------------------------------------------------------------------------------------
def test_assign_ref_equals_the_double_loop():
    rng = np.random.RandomState(0)
    M = rng.randint(0, 4, (200, 7)).astype(np.float32)          # small integers: ties in almost every row
    M[rng.rand(200, 7) < 0.15] = np.nan
    M[5] = np.nan
    M[6] = [np.nan, np.inf, np.inf, np.nan, np.inf, np.inf, np.inf]          # +inf beside NaNs: the first that is no NaN
    labels, dist = R.assign_ref(M)
    wl, wd = R.assign_bruteforce(M)
    assert np.array_equal(labels, wl) and np.array_equal(dist.astype(np.float64), wd, equal_nan=True)
    assert labels[5] == -1 and np.isnan(dist[5]) and labels[6] == 1 and dist[6] == np.inf


def test_tie_and_nan_rules():
    M = np.array([[2.0, 1.0, 1.0, 3.0],          # equal distances: the smaller index
                  [np.nan, 5.0, np.nan, 5.0],    # a NaN never wins, even at a smaller index
                  [0.0, -0.0, 1.0, 1.0],         # +0 == -0: the smaller index
                  [np.nan] * 4], np.float32)     # NaNs alone: no label
    labels, dist = R.assign_ref(M)
    assert labels.tolist() == [1, 1, 0, -1]
    assert dist[:3].tolist() == [1.0, 5.0, 0.0] and np.isnan(dist[3])
    # the unlabelled row is left out of the counts, the sums and the inertia
    X = np.array([[1.0], [2.0], [4.0], [100.0]], np.float32)
    new, counts = R.update_ref(X, labels, np.zeros((4, 1), np.float32))
    assert counts.tolist() == [1, 2, 0, 0] and new[:, 0].tolist() == [4.0, 1.5, 0.0, 0.0]
    assert R.inertia_ref(dist, labels) == 6.0


@pytest.mark.parametrize('m', MEMBER_COUNTS)
def test_run_order_sums(m):
    """run_sum_fast (np.cumsum) makes the additions of the explicit loops; from 257 members on the order differs from one sequential
    chain, which is the point of writing it down"""
    rng = np.random.RandomState(m)
    terms = (rng.randn(m, 3) * 10.0 ** rng.randint(-6, 7, (m, 3))).astype(np.float32)
    loops, fast = R.run_sum(terms), R.run_sum_fast(terms)
    assert loops.shape == (3,) and np.array_equal(loops.view(np.uint64), fast.view(np.uint64))
    want = np.zeros(3)
    for r in range(0, m, R.RUN):          # the contract once more, without helpers
        s = np.zeros(3)
        for v in terms[r:r + R.RUN].astype(np.float64):
            s = s + v
        want = want + s
    assert np.array_equal(loops, want)
    if m == 0:
        assert np.array_equal(loops, np.zeros(3)) and not np.signbit(loops).any()


def test_run_order_is_not_one_chain():
    terms = np.float32(1.0) + np.arange(600, dtype=np.float32) * np.float32(1e-7)
    terms[::2] *= np.float32(1e8)
    chain = 0.0
    for v in terms.astype(np.float64):
        chain += v
    assert float(R.run_sum(terms)) != chain          # three runs, added afterwards: other roundings than one chain


def test_update_and_inertia_follow_the_run_order():
    rng = np.random.RandomState(3)
    X = rng.randn(700, 5).astype(np.float32)
    labels = rng.randint(0, 2, 700)
    labels[::50] = -1
    prev = rng.randn(3, 5).astype(np.float32)
    new, counts = R.update_ref(X, labels, prev)
    for c in range(2):
        members = np.flatnonzero(labels == c)
        assert counts[c] == len(members)
        assert np.array_equal(new[c], (R.run_sum(X[members]) / np.float64(len(members))).astype(np.float32))
    assert counts[2] == 0 and np.array_equal(new[2].view(np.uint32), prev[2].view(np.uint32))          # empty: bit for bit
    dist = rng.rand(700).astype(np.float32)
    assert R.inertia_ref(dist, labels) == float(R.run_sum(dist[labels >= 0]))


# ---- k-means++ -------------------------------------------------------------------------------------------------------------------------
def duplicate_rows():
    """50 rows holding 3 distinct values; K = 5 exceeds them, so the potential reaches 0 and the uniform pick must take over"""
    values = np.array([[0.0, 0.0], [3.0, 4.0], [-6.0, 8.0]], np.float32)
    which = np.random.RandomState(1).randint(0, 3, 50)
    return values[which], which


def test_pp_edge_rules_on_duplicate_rows():
    X, which = duplicate_rows()
    u = np.array([0.5, 0.3, 0.9, 0.2, 0.999])
    chosen = R.pp_ref(X, u, R.distances_f64)
    assert chosen[0] == 25 and len(set(which[chosen[:3]])) == 3          # three picks by the search: three distinct values
    assert chosen[3] == 10 and chosen[4] == 49                           # the total is 0: floor(u n)
    # nobody qualifies: a threshold equal to the total (u cannot reach 1, so the rule is exercised on cumulative_ref directly)
    mind = np.array([0.0, 2.0, 0.0, 1.0, 0.0])
    cum, total = R.cumulative_ref(mind)
    assert total == 3.0 and len(np.flatnonzero(cum > total)) == 0 and np.flatnonzero(mind > 0)[-1] == 3
    # a NaN counts as 0 and is never the first to exceed a threshold
    cum, total = R.cumulative_ref(np.where(np.isnan([np.nan, 1.0, np.nan, 2.0]), 0.0, [0.0, 1.0, 0.0, 2.0]))
    assert cum.tolist() == [0.0, 1.0, 1.0, 3.0] and [int(np.flatnonzero(cum > t)[0]) for t in (0.0, 0.5, 1.0, 2.9)] == [1, 1, 3, 3]


def test_pp_nan_rows_are_never_picked_by_the_search():
    rng = np.random.RandomState(2)
    X = rng.randn(600, 4).astype(np.float32)
    X[::7, 1] = np.nan
    u = np.r_[0.2, rng.random_sample(11)]          # (row 120 = floor(0.2 * 600) has no NaN)
    chosen = R.pp_ref(X, u, R.distances_f64)
    assert not np.isnan(X[chosen]).any()


def test_cumulative_ref_is_the_two_level_order():
    v = np.random.RandomState(4).rand(600) * 1e3
    cum, total = R.cumulative_ref(v)
    off, k = 0.0, 0
    for r in range(0, 600, R.RUN):
        pre = 0.0
        for x in v[r:r + R.RUN]:
            pre += x
            assert cum[k] == off + pre
            k += 1
        off += pre
    assert total == off == cum[-1] and np.all(np.diff(cum) >= 0)


# ---- scores against scikit-learn's recorded values ---------------------------------------------------------------------------------------
def test_scores_equal_sklearn(golden):
    assert str(golden['sklearn_version']) == '1.7.2' and golden['pairs_a'].shape == (10, 300)
    for a, b, nmi, ari in zip(golden['pairs_a'], golden['pairs_b'], golden['nmi'], golden['ari']):
        table = R.contingency_ref(a, b, int(a.max()) + 1, int(b.max()) + 1)
        assert table.sum() == 300
        for f_nmi, f_ari in ((R.nmi_ref, R.adjusted_rand_ref), (cluster.nmi, cluster.adjusted_rand)):
            assert abs(f_nmi(table) - nmi) <= 1e-12 and abs(f_ari(table) - ari) <= 1e-12
            assert abs(f_nmi(table.T) - nmi) <= 1e-12 and abs(f_ari(table.T) - ari) <= 1e-12          # both are symmetric


def test_purity():
    table = np.array([[5, 1, 0], [2, 2, 6], [0, 0, 0]])
    assert cluster.purity(table) == R.purity_ref(table) == 11.0 / 16.0
    assert cluster.purity(np.eye(4, dtype=np.int64) * 3) == 1.0
    with pytest.raises(ValueError):
        cluster.purity(np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError):
        cluster.nmi(np.ones((2, 2)))          # counts are integers


@pytest.mark.parametrize('fixture', range(3))
def test_quality_bar_against_sklearn_inertias(golden, fixture):
    """plain k-means++ with the best of 8 restarts against scikit-learn's greedy seeding in single runs: at or below the mean + 3 std
    of its eight recorded inertias (float64 distances on the CPU; the GPU's fit is held to the same oracle bit for bit)"""
    K, D, per, spread = golden['blob_params'][fixture]
    X, _ = R.blobs(int(K), int(D), int(per), float(spread))
    recorded = golden['blob_inertia'][fixture]
    bar = recorded.mean() + 3.0 * recorded.std()
    best = R.best_of_ref(X, int(K), 0, 8, 300, R.distances_f64)
    print('fixture %d: best of 8 = %.1f, bar = %.1f, sklearn min = %.1f' % (fixture, best['inertia'], bar, recorded.min()))
    assert best['inertia'] <= bar
    assert best['history'][-1, 1] == 0 and best['n_iter'] < 300          # it settled


def test_fit_ref_ends_with_labels_that_belong_to_the_centroids():
    X, _ = R.blobs(6, 16, 100, 2.0)
    got = R.fit_ref(X, X[:6], 2, R.distances_f64)
    assert got['n_iter'] == 2 and got['history'][0, 1] == 600 and got['history'][1, 1] > 0
    labels, dist = R.assign_ref(R.distances_f64(X, got['centroids']))
    assert np.array_equal(labels, got['labels']) and got['inertia'] == R.inertia_ref(dist, labels)


# ---- the binding, refusals, pickling, the command line -----------------------------------------------------------------------------------
def test_every_symbol_is_in_the_binding_and_the_header():
    header = open(os.path.join(ROOT, 'include', 'l3hip.h')).read()
    declared = set(re.findall(r'\b(l3_(?:op_)?kmeans[a-z_]*)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert declared == set(SYMBOLS)
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
    assert '#define L3_KMEANS_RUN 256' in header and _lib.KMEANS_RUN == R.RUN == 256
    assert _lib.KMEANS_MAX_CLUSTERS == 65536 and _lib.KMEANS_MAX_CLASSES == 256


def test_refusals_come_before_the_device():
    """every one of these is a ValueError on a machine without a GPU: nothing reaches the library"""
    X = np.zeros((10, 4), np.float32)
    for K in (0, -1, 65537, 2.0, True):
        with pytest.raises(ValueError, match='n_clusters'):
            cluster.KMeans(K, random_state=0)
    with pytest.raises(ValueError, match='at least as many rows'):
        cluster.KMeans(11, random_state=0).fit(X)
    with pytest.raises(ValueError, match='at least as many rows'):
        _lib.op_kmeans_step(X, np.zeros((11, 4), np.float32))
    with pytest.raises(ValueError, match='squared Euclidean'):
        _lib.KMeans(4, 3, metric='cosine')
    with pytest.raises(ValueError, match='float32'):
        cluster.KMeans(3, random_state=0).fit(X.astype(np.float64))
    with pytest.raises(ValueError, match='float32'):
        _lib.op_kmeans_step(X.astype(np.float64), X[:3])
    for init in ('k-means++', 'random'):
        with pytest.raises(ValueError, match='random_state'):
            cluster.KMeans(3, init=init)
    with pytest.raises(ValueError, match='init'):
        cluster.KMeans(3, init='greedy', random_state=0)
    with pytest.raises(ValueError, match='init centroids'):
        cluster.KMeans(3, init=np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match='max_iter'):
        cluster.KMeans(3, random_state=0, max_iter=0)
    km = cluster.KMeans.from_centroids(X[:3])
    with pytest.raises(ValueError, match='at most 256 classes'):
        km.contingency(np.arange(10) * 40)          # C = 361
    with pytest.raises(ValueError, match='>= 0'):
        km.contingency(np.array([-1, 0]))
    with pytest.raises(ValueError, match='fit comes first'):
        cluster.KMeans(3, random_state=0).predict(X)
    h = _lib.KMeans(4, 3)
    with pytest.raises(ValueError, match='set_rows comes first'):
        h.seed_pp(np.zeros(3))
    with pytest.raises(ValueError, match='come first'):
        h.predict(X)
    assert h.h is None and km._h is None          # no handle was ever created


def test_pickling_keeps_the_centroids_and_no_handle():
    km = cluster.KMeans(3, init='random', n_init=2, random_state=7)
    km.cluster_centers_ = np.arange(12, dtype=np.float32).reshape(3, 4)
    km._h, km._rows_resident = object(), True          # stands for a device handle
    back = pickle.loads(pickle.dumps(km))
    assert back._h is None and back._rows_resident is False
    assert np.array_equal(back.cluster_centers_, km.cluster_centers_) and back.random_state == 7 and back.init == 'random'
    km._h = None


def test_seeds_of_the_restarts():
    km = cluster.KMeans(3, n_init=4, random_state=123)
    assert km._seeds() == R.seeds_ref(123, 4).tolist()
    assert cluster.KMeans(2, init=np.zeros((2, 3), np.float32), n_init=4)._seeds() == [None]


def test_cli_parser():
    command, args = cli_cluster.parse_arguments(['fit', '--features', 'a.npz', 'dir', '--clusters', '64', '--seed', '3', '--out', 'm.npz'])
    assert command == 'fit' and args == dict(features=['a.npz', 'dir'], clusters=64, seed=3, n_init=8, max_iter=300, init='k-means++',
                                             device=0, out='m.npz')
    command, args = cli_cluster.parse_arguments(['histograms', '--model', 'm.npz', '--features', 'b.npz', '--out', 'h.npz', '--normalize'])
    assert command == 'histograms' and args == dict(model='m.npz', features=['b.npz'], out='h.npz', normalize=True, device=0)
    for bad in (['fit', '--features', 'a.npz', '--clusters', '64', '--out', 'm.npz'],                       # no seed
                ['fit', '--features', 'a.npz', '--clusters', '0', '--seed', '1', '--out', 'm.npz'],
                ['fit', '--features', 'a.npz', '--clusters', '4', '--seed', '1', '--n-init', '0', '--out', 'm.npz'],
                ['histograms', '--features', 'b.npz', '--out', 'h.npz']):
        with pytest.raises(SystemExit):
            cli_cluster.parse_arguments(bad)
