"""K-means on the GPU (csrc/kmeans.hip) against tests/cluster_ref.py: one step bit-equal to the library's own distance
matrix and within the derived bound of float64, exact integer rows, the update's run order, whole fit trajectories, the seeding, NaN
rows, the label statistics and the Python layers.

"Library distances" are l3_knn_matrix's (the rows as queries, the centroids as database): the contract says the k-means kernels have
those bits, and tests/test_knn_gpu.py holds that matrix to float64.

Largest observed |d - d64| / bound over the cases of test_step_distances_within_the_float64_bound (profiles/r36_kmeans.txt has the
run): 0.0808 (333, 3, 19), 0.0152 (1000, 130, 512), 0.078 (300, 257, 40), 0.00326 (129, 1, 6144), 3.35e-10 (700, 700, 8: every row is
a centroid, so the distances are 0 or within a rounding of it)."""
import ctypes
import pickle

import numpy as np
import pytest

import cluster_ref as R
import knn_ref
from l3embedding_amd import _lib, cli_cluster, cluster, usc

pytestmark = pytest.mark.gpu

STEP_SHAPES = [(333, 3, 19), (1000, 130, 512), (300, 257, 40), (129, 1, 6144), (700, 700, 8)]
MEMBER_COUNTS = (0, 1, 255, 256, 257, 600)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


class LibraryDistances(object):
    """distances(rows, centroids) -> l3_knn_matrix of them, float32 (n, K)"""

    def __init__(self, D):
        self.h = _lib.KNN(D, 'sqeuclidean')
        self.rows = None

    def __call__(self, rows, centroids):
        if rows is not self.rows:
            self.h.set_queries(np.ascontiguousarray(rows, np.float32))
            self.rows = rows
        self.h.set_database(np.ascontiguousarray(centroids, np.float32))
        return self.h.matrix()

    def close(self):
        self.h.close()


# ---- 1. one step --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=STEP_SHAPES, ids=lambda s: '%d-%d-%d' % s)
def step(request, gpu_required):
    n, K, D = request.param
    rng = np.random.RandomState(n + K + D)
    X = rng.randn(n, D).astype(np.float32)
    cen = X[rng.permutation(n)[:K]].copy() if K == n else (0.5 * rng.randn(K, D)).astype(np.float32)
    lib = LibraryDistances(D)
    M = lib(X, cen)
    lib.close()
    return dict(n=n, K=K, D=D, X=X, cen=cen, M=M, got=_lib.op_kmeans_step(X, cen))


def test_step_equals_the_list_oracle_on_the_library_matrix(step):
    got, M = step['got'], step['M']
    idx, dist = knn_ref.topk_ref(M, 1)
    assert got['labels'].dtype == np.int32 and got['dist'].dtype == np.float32
    assert np.array_equal(got['labels'], idx[:, 0]) and np.array_equal(bits(got['dist']), bits(dist[:, 0]))
    labels, dist = R.assign_ref(M)
    assert np.array_equal(got['labels'], labels) and np.array_equal(bits(got['dist']), bits(dist))
    if step['K'] == step['n']:
        assert np.all(got['dist'] == 0.0)          # every row is a centroid


def test_step_distances_within_the_float64_bound(step):
    """the bound is derived (knn_ref.distance_bound), not measured; d(i, label) is also at most the float64 minimum + its bound,
    since d32(i, label) <= d32(i, j*) <= d64(i, j*) + bound(i, j*) for the float64 argmin j*; no row is left out"""
    X, cen, got = step['X'], step['cen'], step['got']
    ref, bound = knn_ref.distances_ref(X, cen, 'sqeuclidean'), knn_ref.distance_bound(X, cen, 'sqeuclidean')
    rows = np.arange(step['n'])
    err = np.abs(got['dist'].astype(np.float64) - ref[rows, got['labels']])
    with np.errstate(invalid='ignore', divide='ignore'):
        print('kmeans bound ratio (%d, %d, %d): %.3g' % (step['n'], step['K'], step['D'], float(np.nanmax(err / bound[rows, got['labels']]))))
    assert np.all(err <= bound[rows, got['labels']])
    best = np.argmin(ref, axis=1)
    assert np.all(got['dist'].astype(np.float64) <= ref[rows, best] + bound[rows, best])


def test_step_update_equals_the_oracle(step):
    got = step['got']
    new, counts = R.update_ref(step['X'], got['labels'], step['cen'])
    assert got['counts'].dtype == np.int64 and np.array_equal(got['counts'], counts) and counts.sum() == step['n']
    assert np.array_equal(bits(got['centroids']), bits(new))
    assert bits(np.float64(got['inertia'])) == bits(np.float64(R.inertia_ref(got['dist'], got['labels'])))


# ---- 2. exact rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', (19, 512))
def test_exact_rows_equal_the_int64_oracle(gpu_required, D):
    """integers in [-4, 4]: every partial sum is below 2^24, float32 is exact; centroid 3 is a copy of centroid 1, so whoever is
    nearest to it ties, and the index decides"""
    rng = np.random.RandomState(D)
    X = rng.randint(-4, 5, (400, D))
    cen = X[rng.permutation(400)[:140]].copy()
    cen[3] = cen[1]
    want = R.distances_f64(X, cen)
    assert want.dtype == np.int64
    labels, dist = R.assign_ref(want)
    tied = (np.sort(want, axis=1)[:, 0] == np.sort(want, axis=1)[:, 1])
    assert tied.any() and np.any(labels == 1) and not np.any(labels == 3)          # a tie the index broke, on the oracle
    for i in np.flatnonzero(tied):
        assert labels[i] == np.flatnonzero(want[i] == want[i].min())[0]
    got = _lib.op_kmeans_step(X.astype(np.float32), cen.astype(np.float32))
    assert np.array_equal(got['labels'], labels) and np.array_equal(got['dist'].astype(np.float64), dist)
    assert got['inertia'] == float(dist.sum())          # integers below 2^53: exact in any order
    assert got['counts'][3] == 0 and np.array_equal(got['centroids'][3], cen[3].astype(np.float32))


# ---- 3. the update's run order ------------------------------------------------------------------------------------------------------------------
def test_update_at_the_run_boundaries(gpu_required):
    D = 24
    rng = np.random.RandomState(8)
    centres = (20.0 * rng.randn(len(MEMBER_COUNTS), D)).astype(np.float32)
    y = np.repeat(np.arange(len(MEMBER_COUNTS)), MEMBER_COUNTS)
    order = rng.permutation(len(y))          # the members of a cluster lie scattered among the rows
    y = y[order]
    X = (centres[y] + rng.randn(len(y), D) * 10.0 ** rng.randint(-3, 1, (len(y), 1))).astype(np.float32)
    got = _lib.op_kmeans_step(X, centres)
    assert np.array_equal(got['labels'], y) and got['counts'].tolist() == list(MEMBER_COUNTS)
    new, counts = R.update_ref(X, got['labels'], centres)
    assert np.array_equal(bits(got['centroids']), bits(new)) and np.array_equal(got['counts'], counts)
    assert np.array_equal(bits(got['centroids'][0]), bits(centres[0]))          # the empty cluster: untouched bits
    assert bits(np.float64(got['inertia'])) == bits(np.float64(R.inertia_ref(got['dist'], got['labels'])))
    for c in (2, 4, 5):          # (and the oracle's fast sums are its loops)
        members = np.flatnonzero(y == c)
        assert np.array_equal(new[c], (R.run_sum(X[members]) / np.float64(len(members))).astype(np.float32))


# ---- 4. fit ---------------------------------------------------------------------------------------------------------------------------------
def _fit_fixture(n, K, D):
    rng = np.random.RandomState(n + K)
    if K <= 16:
        X = ((3.0 * rng.randn(K, D))[rng.randint(0, K, n)] + 2.0 * rng.randn(n, D)).astype(np.float32)
    else:
        X = rng.randn(n, D).astype(np.float32)
    return X, rng.permutation(n)[:K].astype(np.int64)


@pytest.mark.parametrize('shape', [(1000, 10, 40), (600, 130, 512)], ids=lambda s: '%d-%d-%d' % s)
def test_fit_trajectory_equals_the_oracle_on_library_distances(gpu_required, shape):
    n, K, D = shape
    X, chosen = _fit_fixture(n, K, D)
    lib = LibraryDistances(D)
    want = R.fit_ref(X, X[chosen], 100, lib)
    lib.close()
    h = _lib.KMeans(D, K)
    h.set_rows(X)
    h.seed_rows(chosen)
    history = h.fit(100)
    got = h.labels()
    assert want['n_iter'] < 100 and len(history) == want['n_iter'] and history[0, 1] == n and history[-1, 1] == 0
    assert np.array_equal(bits(history), bits(want['history']))
    assert np.array_equal(got['labels'], want['labels']) and np.array_equal(bits(got['dist']), bits(want['dist']))
    assert bits(np.float64(got['inertia'])) == bits(np.float64(want['inertia'])) == bits(history[-1, :1])[0]
    assert np.array_equal(bits(h.centroids()), bits(want['centroids']))
    h.close()


def test_max_iter_ends_with_one_more_assignment(gpu_required):
    X, chosen = _fit_fixture(1000, 10, 40)
    lib = LibraryDistances(40)
    want = R.fit_ref(X, X[chosen], 2, lib)
    h = _lib.KMeans(40, 10)
    h.set_rows(X)
    h.seed_rows(chosen)
    history = h.fit(2)
    got, cen = h.labels(), h.centroids()
    h.close()
    assert len(history) == 2 and history[1, 1] > 0 and np.array_equal(bits(history), bits(want['history']))
    labels, dist = R.assign_ref(lib(X, cen))          # the labels belong to the centroids that are returned
    lib.close()
    assert np.array_equal(bits(cen), bits(want['centroids']))
    assert np.array_equal(got['labels'], labels) and np.array_equal(bits(got['dist']), bits(dist))
    assert got['inertia'] == R.inertia_ref(dist, labels) == want['inertia'] and got['inertia'] < history[1, 0]


def test_two_fits_give_identical_bits_and_restarts_choose_the_lowest_inertia(gpu_required):
    X, _ = R.blobs(10, 32, 60, 3.0)
    runs = [cluster.KMeans(10, n_init=3, random_state=4).fit(X) for _ in range(2)]
    a, b = runs
    assert np.array_equal(bits(a.cluster_centers_), bits(b.cluster_centers_)) and np.array_equal(a.labels_, b.labels_)
    assert a.inertia_ == b.inertia_ and np.array_equal(a.history_, b.history_) and np.array_equal(a.chosen_, b.chosen_)
    assert a.history_.dtype.names == ('inertia', 'changed', 'empty') and a.n_iter_ == len(a.history_) and a.history_['changed'][-1] == 0
    lib = LibraryDistances(32)
    want = R.best_of_ref(X, 10, 4, 3, 300, lib)
    singles = []
    for seed in R.seeds_ref(4, 3):
        one = cluster.KMeans(10, init=X[R.pp_ref(X, np.random.RandomState(seed).random_sample(10), lib)], max_iter=300).fit(X)
        singles.append(one.inertia_)
        one.close()
    lib.close()
    assert a.inertia_ == min(singles) == want['inertia'] and a.best_run_ == int(np.argmin(singles))
    assert np.array_equal(a.chosen_, want['chosen']) and np.array_equal(a.labels_, want['labels'])
    assert np.array_equal(bits(a.cluster_centers_), bits(want['centroids']))
    for m in runs:
        m.close()


def test_separated_blobs_from_one_row_each_are_recovered(gpu_required):
    rng = np.random.RandomState(9)
    y = np.repeat(np.arange(7), 50)[rng.permutation(350)]
    X = (100.0 * np.eye(7, 12)[y] + rng.randn(350, 12)).astype(np.float32)
    first = np.array([np.flatnonzero(y == c)[0] for c in range(7)])
    km = cluster.KMeans(7, init=X[first]).fit(X)
    got = km.scores(y)
    assert got['adjusted_rand'] == 1.0 and got['purity'] == 1.0 and abs(got['nmi'] - 1.0) < 1e-12
    assert np.array_equal(km.labels_, y) and km.chosen_ is None and km.history_['empty'].sum() == 0
    km.close()


# ---- 5. seeding -----------------------------------------------------------------------------------------------------------------------------
def test_seeding_equals_the_oracle_on_library_distances(gpu_required):
    X, _ = R.blobs(20, 40, 50, 2.5)
    assert X.shape == (1000, 40)
    u = np.random.RandomState(6).random_sample(20)
    lib = LibraryDistances(40)
    want = R.pp_ref(X, u, lib)
    lib.close()
    h = _lib.KMeans(40, 20)
    h.set_rows(X)
    chosen = h.seed_pp(u)
    assert chosen.dtype == np.int64 and np.array_equal(chosen, want) and len(set(chosen.tolist())) == 20
    assert np.array_equal(bits(h.centroids()), bits(X[chosen]))
    h.close()
    km = cluster.KMeans(20, n_init=1, random_state=6).fit(X)          # the Python layer draws its u from the restart's seed
    lib = LibraryDistances(40)
    assert np.array_equal(km.chosen_, R.pp_ref(X, np.random.RandomState(R.seeds_ref(6, 1)[0]).random_sample(20), lib))
    lib.close()
    km.close()


def test_seeding_on_duplicate_rows_follows_the_edge_rules(gpu_required):
    values = np.array([[0.0, 0.0], [3.0, 4.0], [-6.0, 8.0]], np.float32)
    X = values[np.random.RandomState(1).randint(0, 3, 50)]
    u = np.array([0.5, 0.3, 0.9, 0.2, 0.999])
    lib = LibraryDistances(2)
    want = R.pp_ref(X, u, lib)
    lib.close()
    assert want.tolist() == R.pp_ref(X, u, R.distances_f64).tolist() and want[3] == 10 and want[4] == 49
    h = _lib.KMeans(2, 5)
    h.set_rows(X)
    assert np.array_equal(h.seed_pp(u), want)
    history = h.fit(10)
    assert history[-1, 2] == 2 and history[-1, 0] == 0.0          # three distinct values: two of five clusters stay empty
    h.close()


# ---- 6. NaN rows, other rows, statistics, layers ------------------------------------------------------------------------------------------------
def test_a_nan_row_has_no_label_and_leaves_every_sum_alone(gpu_required):
    rng = np.random.RandomState(12)
    X = rng.randn(700, 20).astype(np.float32)
    cen = X[:4].copy()
    bad = X.copy()
    bad = np.insert(bad, 300, np.float32(np.nan), axis=0)
    bad[300, 1:] = 1.0          # one NaN feature is enough
    got, clean = _lib.op_kmeans_step(bad, cen), _lib.op_kmeans_step(X, cen)
    assert got['labels'][300] == -1 and np.isnan(got['dist'][300])
    keep = np.arange(701) != 300
    assert np.array_equal(got['labels'][keep], clean['labels']) and np.array_equal(bits(got['dist'][keep]), bits(clean['dist']))
    assert np.array_equal(got['counts'], clean['counts']) and got['counts'].sum() == 700
    assert np.array_equal(bits(got['centroids']), bits(clean['centroids']))
    assert bits(np.float64(got['inertia'])) == bits(np.float64(clean['inertia']))
    h = _lib.KMeans(20, 4)
    h.set_rows(bad)
    h.set_centroids(cen)
    history = h.fit(50)
    assert history[0, 1] == 701 and history[-1, 1] == 0 and h.labels()['labels'][300] == -1
    table = h.contingency(np.zeros(701, np.int64), 1)
    assert table.sum() == 700          # the row without a label is not counted
    h.close()


def test_device_features_predict_and_statistics(gpu_required, tmp_path):
    X, y = R.blobs(6, 16, 100, 2.0)
    Q, yq = R.blobs(6, 16, 30, 2.0, seed=5)
    Q = Q + np.float32(0.25)
    on_host = cluster.KMeans(6, n_init=2, random_state=1).fit(X)
    fx = usc.DeviceFeatures(X)
    on_dev = cluster.KMeans(6, n_init=2, random_state=1).fit(fx)
    fx.close()          # the model owns its rows
    assert np.array_equal(on_host.labels_, on_dev.labels_) and np.array_equal(bits(on_host.cluster_centers_), bits(on_dev.cluster_centers_))
    assert on_host.inertia_ == on_dev.inertia_ and np.array_equal(on_host.chosen_, on_dev.chosen_)
    assert np.array_equal(on_host.fit_predict(X), on_host.labels_)
    # predict and transform on other rows
    lib = LibraryDistances(16)
    M = lib(Q, on_host.cluster_centers_)
    lib.close()
    labels, _ = R.assign_ref(M)
    fq = usc.DeviceFeatures(Q)
    assert np.array_equal(on_host.predict(Q), labels) and np.array_equal(on_dev.predict(fq), labels)
    assert np.array_equal(bits(on_host.transform(Q)), bits(M)) and np.array_equal(bits(on_dev.transform(fq)), bits(M))
    assert np.array_equal(on_host.predict(X), on_host.labels_)
    # contingency and scores
    table = on_host.contingency(y)
    assert table.dtype == np.int64 and np.array_equal(table, R.contingency_ref(on_host.labels_, y, 6, 6))
    assert np.array_equal(on_dev.contingency(yq, X=fq, num_classes=9), R.contingency_ref(labels, yq, 6, 9))
    got = on_host.scores(y)
    assert got['nmi'] == R.nmi_ref(table) and got['adjusted_rand'] == R.adjusted_rand_ref(table) and got['purity'] == R.purity_ref(table)
    # file histograms
    files = [(0, 100), (100, 101), (101, 600), (50, 300)]
    hist = on_host.file_histograms(files)
    assert hist.dtype == np.int32 and hist.shape == (4, 6)
    assert np.array_equal(hist, [np.bincount(on_host.labels_[s:e], minlength=6) for s, e in files])
    qfiles = [(0, 30), (30, 180)]
    hq = on_dev.file_histograms(qfiles, X=fq, normalize=True)
    assert np.array_equal(hq, [np.bincount(labels[s:e], minlength=6) / float(e - s) for s, e in qfiles])
    fq.close()
    # a pickled model has its centroids and rebuilds its handle; the fitted rows are gone with the handle
    back = pickle.loads(pickle.dumps(on_dev))
    assert back._h is None and np.array_equal(back.predict(Q), labels)
    with pytest.raises(ValueError, match='pass X'):
        back.contingency(y)
    assert np.array_equal(back.contingency(yq, X=Q), R.contingency_ref(labels, yq, 6, 6))
    for m in (on_host, on_dev, back):
        m.close()


def test_the_librarys_refusals(gpu_required):
    lib = _lib.load()
    h = ctypes.c_void_p()
    for args, text in (((0, 4, 3, 1), b'squared Euclidean'), ((0, 4, 0, 0), b'clusters'), ((0, 4, 65537, 0), b'clusters'), ((0, 0, 3, 0), b'features')):
        assert lib.l3_kmeans_create(*args, ctypes.byref(h)) == -1 and text in lib.l3_last_error(None) and not h.value
    assert lib.l3_kmeans_create(0, 4, 3, 0, ctypes.byref(h)) == 0
    X = np.zeros((2, 4), np.float32)
    assert lib.l3_kmeans_set_rows(h, _lib._ptr(X), 2) == -1 and b'at least as many rows' in lib.l3_last_error(None)
    assert lib.l3_kmeans_assign(h, None, None, None, None) == -1 and b'rows come first' in lib.l3_last_error(None)
    X = np.arange(40, dtype=np.float32).reshape(10, 4)
    assert lib.l3_kmeans_set_rows(h, _lib._ptr(X), 10) == 0
    assert lib.l3_kmeans_fit(h, 5, None, None) == -1 and b'centroids come first' in lib.l3_last_error(None)
    assert lib.l3_kmeans_update(h, None) == -1 and b'assignment comes first' in lib.l3_last_error(None)
    u = np.array([0.1, 1.0, 0.2])
    assert lib.l3_kmeans_seed_pp(h, _lib._ptr(u), None) == -1 and b'outside [0, 1)' in lib.l3_last_error(None)
    rows = np.array([0, 10, 2], np.int64)
    assert lib.l3_kmeans_seed_rows(h, _lib._ptr(rows)) == -1 and b'outside the 10 rows' in lib.l3_last_error(None)
    rows[1] = 9
    assert lib.l3_kmeans_seed_rows(h, _lib._ptr(rows)) == 0
    assert lib.l3_kmeans_fit(h, 0, None, None) == -1 and b'max_iter' in lib.l3_last_error(None)
    assert lib.l3_kmeans_assign(h, None, None, None, None) == 0          # nothing downloaded
    classes, table = np.zeros(10, np.int32), np.zeros((3, 300), np.int64)
    assert lib.l3_kmeans_contingency(h, 0, _lib._ptr(classes), 257, _lib._ptr(table)) == -1 and b'n_classes' in lib.l3_last_error(None)
    classes[4] = 2
    assert lib.l3_kmeans_contingency(h, 0, _lib._ptr(classes), 2, _lib._ptr(table)) == -1 and b'classes[4]' in lib.l3_last_error(None)
    assert lib.l3_kmeans_contingency(h, 1, _lib._ptr(classes), 3, _lib._ptr(table)) == -1 and b'predict comes first' in lib.l3_last_error(None)
    files, hist = np.array([[0, 11]], np.int64), np.zeros((1, 3), np.int32)
    assert lib.l3_kmeans_file_hist(h, 0, _lib._ptr(files), 1, _lib._ptr(hist)) == -1 and b'outside the 10 rows' in lib.l3_last_error(None)
    lib.l3_kmeans_destroy(h)
    feat = _lib.Features(np.zeros((5, 3), np.float32))
    km = _lib.KMeans(4, 2)
    with pytest.raises(ValueError, match='columns'):
        km.set_rows(feat)
    km.close()
    feat.close()


def test_timed_rounds_leave_a_usable_handle(gpu_required):
    X, _ = R.blobs(6, 16, 100, 2.0)
    h = _lib.KMeans(16, 6)
    h.set_rows(X)
    for what in ('seed',) + tuple(w for w in _lib.KMEANS_TIMED if w != 'seed'):
        assert h.time(what, reps=1) > 0.0
    history = h.fit(50)          # the labels were voided: the first iteration changes every row again
    assert history[0, 1] == 600 and history[-1, 1] == 0
    h.close()


def test_cli_fit_then_histograms_round_trip_two_files(gpu_required, tmp_path):
    rng = np.random.RandomState(5)
    A = np.r_[rng.randn(40, 12) + 8.0, rng.randn(30, 12) - 8.0].astype(np.float32)
    B = (rng.randn(25, 12) + 8.0).astype(np.float32)
    np.savez(str(tmp_path / 'A.npz'), X=A, y=np.r_[np.zeros(40, np.int64), np.ones(30, np.int64)])
    np.savez(str(tmp_path / 'B.npz'), X=B, y=np.array(0))
    model, out = str(tmp_path / 'model.npz'), str(tmp_path / 'hist.npz')
    cli_cluster.main(['fit', '--features', str(tmp_path / 'A.npz'), str(tmp_path / 'B.npz'), '--clusters', '2', '--seed', '3', '--n-init', '2',
                      '--out', model])
    with np.load(model) as got:
        assert got['centroids'].shape == (2, 12) and got['labels'].shape == (95,) and got['entry'].tolist() == [0] * 70 + [1] * 25
        assert got['frame'][70:].tolist() == list(range(25)) and got['names'].tolist() == ['A', 'B']
        assert got['adjusted_rand'] == 1.0 and got['purity'] == 1.0 and got['contingency'].sum() == 95
        assert got['history_changed'][-1] == 0 and got['n_iter'] == len(got['history_inertia']) and len(got['chosen']) == 2
        labels = got['labels']
    cli_cluster.main(['histograms', '--model', model, '--features', str(tmp_path / 'A.npz'), str(tmp_path / 'B.npz'), '--out', out])
    with np.load(out) as got:
        assert got['names'].tolist() == ['A', 'B'] and got['hist'].shape == (2, 2) and got['hist'].dtype == np.int32
        assert np.array_equal(got['hist'][0], np.bincount(labels[:70], minlength=2))
        assert np.array_equal(got['hist'][1], np.bincount(labels[70:], minlength=2)) and got['hist'][1].max() == 25
        assert got['label'].tolist() == [0, 0] and got['file_idxs'].tolist() == [[0, 70], [70, 95]]
