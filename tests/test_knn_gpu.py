"""Nearest neighbours on the GPU (csrc/knn.hip) against tests/knn_ref.py: exact integer rows, bit-equal distances across
the matrix, listed pairs and lists, the float64 bound, segments, groups, NaN and zero rows, votes, and the Python layers.

Largest observed |d - d64| / bound over the cases of test_matrix_within_the_float64_bound (profiles/r35_knn.txt has the run):
sqeuclidean 0.114 (D = 20), 0.0143 (D = 512), 0.00507 (D = 6144); cosine 0.0912, 0.00258, 0.000216."""
import os
import pickle

import numpy as np
import pytest

import knn_ref as R
from l3embedding_amd import _lib, classifier, cli_knn, knn, usc

pytestmark = pytest.mark.gpu

DIMS = (20, 512, 6144)          # a multiple of neither 8 nor 32; the embedding size; the largest
NQ, NC = 130, 200               # two 128-tiles with a ragged 2 x two with a ragged 72
KS = (1, 5, 64)
SEARCH_KS = (1, 3, 5, 10, 20, 50)
METRICS = ('sqeuclidean', 'cosine')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _index_broke_a_tie(idx, dist):
    """some list holds two equal distances next to each other, the smaller index first"""
    same = (dist[:, 1:] == dist[:, :-1]) & (idx[:, 1:] >= 0)
    assert np.all(idx[:, 1:][same] > idx[:, :-1][same])
    return bool(same.any())


# ---- 1. exact integer rows -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=DIMS)
def exact(request, gpu_required):
    """integer rows in [-4, 4]: every partial sum is below 16 * 6144 < 2^24, so float32 is exact in any order"""
    D = request.param
    rng = np.random.RandomState(D)
    Q, X = rng.randint(-4, 5, (NQ, D)), rng.randint(-4, 5, (NC, D))
    h = _lib.KNN(D, 'sqeuclidean')
    h.set_database(X.astype(np.float32), labels=rng.randint(0, 10, NC))
    h.set_queries(Q.astype(np.float32))
    yield dict(h=h, D=D, Q=Q, X=X, want=R.distances_ref(Q, X, 'sqeuclidean'), M=h.matrix())
    h.close()


def test_exact_matrix_equals_the_int64_oracle(exact):
    assert exact['want'].dtype == np.int64 and exact['M'].dtype == np.float32 and exact['M'].shape == (NQ, NC)
    assert np.array_equal(exact['M'].astype(np.int64), exact['want']) and np.all(exact['M'] == np.floor(exact['M']))
    h = exact['h']          # a block that starts inside a tile and ends ragged
    assert np.array_equal(bits(h.matrix(3, 130, 60, 199)), bits(exact['M'][3:130, 60:199]))


@pytest.mark.parametrize('k', KS)
def test_exact_lists_equal_the_oracle(exact, k):
    idx, dist = exact['h'].topk(k)
    widx, wdist = R.topk_ref(exact['want'], k)
    assert idx.dtype == np.int32 and dist.dtype == np.float32
    assert np.array_equal(idx, widx) and np.array_equal(dist.astype(np.float64), wdist)


def test_the_index_breaks_ties_in_some_exact_list(exact):
    """without this the cases above would show nothing about the order: integer rows tie constantly"""
    for k in (5, 64):
        assert _index_broke_a_tie(*exact['h'].topk(k))


# ---- 2. real-valued rows: the same bits everywhere ------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=[(D, m) for D in DIMS for m in METRICS], ids=lambda p: '%d-%s' % p)
def real(request, gpu_required):
    """randn rows; the second half of the candidates are bit copies of the first half, so every distance has a twin"""
    D, metric = request.param
    rng = np.random.RandomState(D + len(metric))
    Q, X = rng.randn(NQ, D).astype(np.float32), rng.randn(NC, D).astype(np.float32)
    X[NC // 2:] = X[:NC // 2]
    h = _lib.KNN(D, metric)
    h.set_database(X)
    h.set_queries(Q)
    yield dict(h=h, D=D, metric=metric, Q=Q, X=X, M=h.matrix(), rng=rng)
    h.close()


@pytest.mark.parametrize('k', KS)
def test_real_lists_equal_the_oracle_on_the_matrix(real, k):
    M = real['M']
    assert np.array_equal(bits(M[:, NC // 2:]), bits(M[:, :NC // 2]))          # the twins tie bit for bit
    idx, dist = real['h'].topk(k)
    widx, wdist = R.topk_ref(M, k)
    assert np.array_equal(idx, widx) and np.array_equal(bits(dist), bits(wdist))
    if k > 1:
        assert _index_broke_a_tie(idx, dist)


def test_real_listed_pairs_have_the_matrix_bits(real):
    iq, ic = real['rng'].randint(0, NQ, 500), real['rng'].randint(0, NC, 500)
    assert np.array_equal(bits(real['h'].list(iq, ic)), bits(real['M'][iq, ic]))


# ---- 3. the matrix against float64 -----------------------------------------------------------------------------------------------------
def test_matrix_within_the_float64_bound(real):
    """the bound is derived (knn_ref.distance_bound), not measured; the observed ratio is printed for profiles/r35_knn.txt"""
    ref, bound = R.distances_ref(real['Q'], real['X'], real['metric']), R.distance_bound(real['Q'], real['X'], real['metric'])
    err = np.abs(real['M'].astype(np.float64) - ref)
    print('knn bound ratio D=%d %s: %.3g' % (real['D'], real['metric'], float((err / bound).max())))
    assert np.all(err <= bound)


# ---- 4. segments -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('k', (5, 64))
def test_segment_counts_give_identical_lists(gpu_required, k, metric):
    rng = np.random.RandomState(700 + k)
    Q, X = rng.randint(-4, 5, (NQ, 20)).astype(np.float32), rng.randint(-4, 5, (700, 20)).astype(np.float32)
    first = _lib.op_knn_topk(Q, X, k, metric=metric, segments=1)
    if metric == 'sqeuclidean':
        widx, wdist = R.topk_ref(R.distances_ref(Q.astype(np.int64), X.astype(np.int64), metric), k)
        assert np.array_equal(first[0], widx) and np.array_equal(first[1].astype(np.float64), wdist)
        assert _index_broke_a_tie(*first)
    for segments in (2, 5, 0):
        idx, dist = _lib.op_knn_topk(Q, X, k, metric=metric, segments=segments)
        assert np.array_equal(idx, first[0]) and np.array_equal(bits(dist), bits(first[1]))


def test_lists_end_empty_when_the_candidates_run_out(gpu_required):
    rng = np.random.RandomState(40)
    Q, X = rng.randint(-4, 5, (NQ, 20)).astype(np.float32), rng.randint(-4, 5, (40, 20)).astype(np.float32)
    idx, dist = _lib.op_knn_topk(Q, X, 64)
    widx, wdist = R.topk_ref(R.distances_ref(Q.astype(np.int64), X.astype(np.int64), 'sqeuclidean'), 64)
    assert np.array_equal(idx, widx) and np.array_equal(dist.astype(np.float64), wdist)
    assert np.all(idx[:, 40:] == -1) and np.all(np.isposinf(dist[:, 40:])) and np.all(idx[:, :40] >= 0)


# ---- 5. groups -------------------------------------------------------------------------------------------------------------------------
def _groups130():
    groups, g = [], 0
    while len(groups) < NQ:          # sizes 1 .. 7, the pattern of test_pairs_gpu's scorer130
        groups += [g] * (g % 7 + 1)
        g += 1
    return np.array(groups[:NQ], np.int32)


@pytest.fixture(scope='module')
def selfq(gpu_required):
    """130 rows that query themselves; the second half are bit copies of the first: every row has a twin at distance 0"""
    rng = np.random.RandomState(131)
    X = rng.randint(-4, 5, (NQ, 20)).astype(np.float32)
    X[65:] = X[:65]
    labels = rng.randint(0, 10, NQ)
    nn = knn.KNeighborsClassifier(n_neighbors=5, num_classes=10).fit(X, labels, groups=_groups130())
    yield dict(nn=nn, X=X, labels=labels, groups=_groups130(), M=R.distances_ref(X.astype(np.int64), X.astype(np.int64), 'sqeuclidean'))
    nn.close()


@pytest.mark.parametrize('k', KS)
def test_no_listed_index_shares_the_querys_group(selfq, k):
    g = selfq['groups']
    dist, idx = selfq['nn'].kneighbors(None, n_neighbors=k, groups_fit=g)
    widx, wdist = R.topk_ref(selfq['M'], k, g, g)
    assert np.array_equal(idx, widx) and np.array_equal(dist.astype(np.float64), wdist)
    listed = idx >= 0
    assert listed.any() and np.all(g[idx[listed]] != np.repeat(g[:, None], k, axis=1)[listed])


def test_a_query_whose_group_holds_every_candidate_has_no_neighbours(selfq):
    one = np.zeros(NQ, np.int32)
    dist, idx = selfq['nn'].kneighbors(None, n_neighbors=5, groups_fit=one)
    assert np.all(idx == -1) and np.all(np.isposinf(dist))
    h = selfq['nn']._handle()
    got = h.vote(5, (1, 5), 10, one, one, outputs=('pred', 'counts'))
    assert np.all(got['pred'] == -1) and not got['counts'].any()


def test_self_query_never_lists_the_row_itself(selfq):
    dist, idx = selfq['nn'].kneighbors(None, n_neighbors=5)
    assert np.all(idx != np.arange(NQ)[:, None]) and np.all(idx >= 0)
    twin = (np.arange(NQ) + 65) % NQ
    assert np.array_equal(idx[:, 0], twin) and np.all(dist[:, 0] == 0.0)          # the twin ties with the row at 0 and is listed
    widx, _ = R.topk_ref(selfq['M'], 5, np.arange(NQ), np.arange(NQ))
    assert np.array_equal(idx, widx)


# ---- 6. NaN and zero rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', METRICS)
def test_a_nan_row_is_never_listed_and_a_zero_row_is_at_cosine_distance_one(gpu_required, metric):
    rng = np.random.RandomState(6)
    Q, X = rng.randn(NQ, 20).astype(np.float32), rng.randn(NC, 20).astype(np.float32)
    X[17, 3] = np.nan
    X[150] = 0.0
    Q[9] = 0.0
    h = _lib.KNN(20, metric)
    h.set_database(X)
    h.set_queries(Q)
    M = h.matrix()
    assert np.all(np.isnan(M[:, 17])) and not np.isnan(np.delete(M, 17, axis=1)).any()
    idx, dist = h.topk(64)
    assert not np.any(idx == 17) and not np.isnan(dist).any()
    widx, wdist = R.topk_ref(M, 64)
    assert np.array_equal(idx, widx) and np.array_equal(bits(dist), bits(wdist))
    idx, _ = h.topk(64, np.zeros(NQ, np.int32), np.r_[np.ones(17, np.int32), 1, np.zeros(NC - 18, np.int32)])
    assert np.all((idx[:, :17] >= 0) & (idx[:, :17] < 17)) and np.all(idx[:, 17:] == -1)          # rows 0 .. 16 are the candidates left
    if metric == 'cosine':
        keep = np.arange(NC) != 17
        assert np.all(M[9][keep] == 1.0) and np.all(M[:, 150] == 1.0)
    h.close()


# ---- 7. votes ----------------------------------------------------------------------------------------------------------------------------
FILES = np.cumsum([0, 1, 40, 7, 22, 13, 30, 17]).astype(np.int64)          # ragged files of 1 .. 40 rows over the 130 queries


@pytest.mark.parametrize('C', (10, 50))
def test_votes_equal_the_oracle(exact, C):
    rng = np.random.RandomState(C)
    files = np.stack([FILES[:-1], FILES[1:]], axis=1)
    assert files[-1, 1] == NQ
    idx, _ = R.topk_ref(exact['want'], 50)          # the lists of case 1
    labels = rng.randint(0, C, NC)
    labels[idx[0, :3]] = (7, 3, 5)          # a forced three-way tie at size 3: the lowest class, 3, must win
    h = _lib.KNN(exact['D'], 'sqeuclidean')
    h.set_database(exact['X'].astype(np.float32), labels=labels)
    h.set_queries(exact['Q'].astype(np.float32))
    assert np.array_equal(h.topk(50)[0], idx)
    got = h.vote(50, SEARCH_KS, C, file_idxs=files, outputs=('counts', 'pred', 'file_counts', 'file_pred'))
    counts, pred, fcounts, fpred = R.vote_ref(idx, labels, SEARCH_KS, C, file_idxs=files)
    for name, want in (('counts', counts), ('pred', pred), ('file_counts', fcounts), ('file_pred', fpred)):
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want), name
    assert got['pred'][0, 1] == 3 and sorted(got['counts'][0, 1].nonzero()[0]) == [3, 5, 7]
    assert np.array_equal(got['counts'].sum(axis=2), np.broadcast_to(np.array(SEARCH_KS), (NQ, 6)))          # every list is full
    only = h.vote(50, (50,), C, file_idxs=files[2:4], outputs=('file_pred',))          # one size, some files, one output
    assert list(only) == ['file_pred'] and np.array_equal(only['file_pred'][:, 0], fpred[2:4, 5])
    h.close()


def test_library_refuses_bad_arguments(exact):
    """the C ABI's own checks: L3_EINVAL and a message that names the call"""
    import ctypes as C
    h = exact['h']
    lib, hd, ptr = h.lib, h.h, _lib._ptr
    i32 = lambda *v: np.array(v, np.int32)          # noqa: E731
    idx, dist, out = np.zeros((NQ, 64), np.int32), np.zeros((NQ, 64), np.float32), np.zeros(NQ * 8, np.int32)
    g = np.zeros(NC, np.int32)
    ks = i32(1, 3)
    fresh, other = C.c_void_p(), C.c_void_p()
    assert lib.l3_knn_create(0, 20, 0, C.byref(fresh)) == 0
    calls = [
        ('l3_knn_create', lambda: lib.l3_knn_create(0, 0, 0, C.byref(other))),
        ('l3_knn_create', lambda: lib.l3_knn_create(0, 8, 2, C.byref(other))),
        ('l3_knn_topk', lambda: lib.l3_knn_topk(hd, 0, None, None, ptr(idx), ptr(dist))),
        ('l3_knn_topk', lambda: lib.l3_knn_topk(hd, 65, None, None, ptr(idx), ptr(dist))),
        ('l3_knn_topk', lambda: lib.l3_knn_topk(hd, 5, ptr(g), None, ptr(idx), ptr(dist))),
        ('l3_knn_topk', lambda: lib.l3_knn_topk(fresh, 5, None, None, ptr(idx), ptr(dist))),          # nothing set
        ('l3_knn_vote', lambda: lib.l3_knn_vote(hd, 5, ptr(i32(3, 1)), 2, 10, None, None, None, 0, None, ptr(out), None, None)),
        ('l3_knn_vote', lambda: lib.l3_knn_vote(hd, 5, ptr(i32(1, 6)), 2, 10, None, None, None, 0, None, ptr(out), None, None)),
        ('l3_knn_vote', lambda: lib.l3_knn_vote(hd, 5, ptr(ks), 2, 10, None, ptr(g), None, 0, None, ptr(out), None, None)),
        ('l3_knn_vote', lambda: lib.l3_knn_vote(hd, 5, ptr(ks), 2, h.label_max, None, None, None, 0, None, ptr(out), None, None)),
        ('l3_knn_matrix', lambda: lib.l3_knn_matrix(hd, 0, NQ + 1, 0, 4, ptr(dist))),
        ('l3_knn_list', lambda: lib.l3_knn_list(hd, ptr(i32(0, NQ)), ptr(i32(0, 0)), 2, ptr(dist))),
        ('l3_op_knn_topk', lambda: lib.l3_op_knn_topk(0, ptr(dist), ptr(dist), 2, 2, 0, 0, 1, 0, None, None, ptr(idx), ptr(dist))),
        ('l3_op_knn_topk', lambda: lib.l3_op_knn_topk(0, ptr(dist), ptr(dist), 2, 2, 4, 0, 1, 257, None, None, ptr(idx), ptr(dist))),
    ]
    assert 1 <= h.label_max <= 9          # the largest label is outside [0, label_max)
    for name, call in calls:
        assert call() == -1, name
        assert name in lib.l3_last_error(None).decode(), name
    rows = np.zeros((4, 20), np.float32)
    assert lib.l3_knn_set_database(fresh, ptr(rows), 4, None) == 0 and lib.l3_knn_query_self(fresh) == 0
    assert lib.l3_knn_vote(fresh, 2, ptr(ks[:1]), 1, 10, None, None, None, 0, None, ptr(out), None, None) == -1          # no labels
    assert 'l3_knn_vote' in lib.l3_last_error(None).decode()
    assert lib.l3_knn_set_database(fresh, ptr(rows), 4, ptr(i32(0, 1, -1, 2))) == -1
    lib.l3_knn_destroy(fresh)
    assert np.array_equal(h.matrix(), exact['M'])          # untouched by the refusals


# ---- 8. through the layers ---------------------------------------------------------------------------------------------------------------
def test_classifier_on_device_features_equals_host_rows(real):
    X, Q = real['X'], real['Q']
    y = np.arange(NC) % 7
    on_host = knn.KNeighborsClassifier(n_neighbors=5, metric=real['metric'], num_classes=7).fit(X, y)
    fx, fq = usc.DeviceFeatures(X), usc.DeviceFeatures(Q)
    on_dev = knn.KNeighborsClassifier(n_neighbors=5, metric=real['metric'], num_classes=7).fit(fx, y)
    fx.close()          # the model owns its rows
    files = [(0, 50), (50, 130)]
    a = on_host.evaluate(Q, file_idxs=files, ks=(1, 5), outputs=knn.EVALUATE_OUTPUTS)
    b = on_dev.evaluate(fq, file_idxs=files, ks=(1, 5), outputs=knn.EVALUATE_OUTPUTS)
    assert a['predict'].shape == (2, NQ) and a['counts'].shape == (2, NQ, 7) and a['file_predict'].shape == (2, 2)
    for name in knn.EVALUATE_OUTPUTS:
        assert np.array_equal(a[name], b[name]), name
    idx, _ = R.topk_ref(real['M'], 5)
    counts, pred = R.vote_ref(idx, y, (1, 5), 7)
    assert np.array_equal(a['predict'], pred.T) and np.array_equal(a['counts'], np.moveaxis(counts, 1, 0))
    assert np.array_equal(on_host.predict(Q), pred[:, 1])
    proba = on_host.predict_proba(Q)
    assert proba.dtype == np.float64 and np.array_equal(proba, counts[:, 1] / 5.0)
    da, ia = on_host.kneighbors(Q)
    db, ib = pickle.loads(pickle.dumps(on_dev)).kneighbors(fq)          # the handle is rebuilt from the pickled rows
    assert np.array_equal(ia, ib) and np.array_equal(bits(da), bits(db)) and np.array_equal(ia, idx)
    assert np.array_equal(bits(on_host.distances(Q)), bits(real['M']))
    assert np.array_equal(bits(on_host.distances(Q, [3, 129], [199, 0])), bits(real['M'][[3, 129], [199, 0]]))
    fq.close(), on_host.close(), on_dev.close()


@pytest.fixture(scope='module')
def toy():
    """a three-class integer-valued split: 60 train, 30 valid and 30 test rows, the test rows in 6 files"""
    rng = np.random.RandomState(3)
    centres = rng.randint(-4, 5, (3, 16))

    def rows(n):
        y = np.arange(n) % 3
        return (centres[y] + rng.randint(-3, 4, (n, 16))).astype(np.float32), y

    (xt, yt), (xv, yv), (xs, ys) = rows(60), rows(30), rows(30)
    files = [(0, 3), (3, 10), (10, 14), (14, 20), (20, 29), (29, 30)]
    file_labels = np.array([np.bincount(ys[a:b]).argmax() for a, b in files])
    return (dict(features=xt, labels=yt), dict(features=xv, labels=yv), dict(features=xs, labels=file_labels, file_idxs=files))


def test_train_knn_equals_the_oracle(gpu_required, toy, tmp_path):
    model, train_m, valid_m, test_m = classifier.train_knn(*toy, str(tmp_path), n_neighbors=5, num_classes=3)
    want = _toy_oracle_any(toy, (5,))[0]
    np.testing.assert_equal([train_m, valid_m, test_m], want)
    with open(str(tmp_path / 'model.pkl'), 'rb') as fh:
        back = pickle.load(fh)
    assert np.array_equal(back.predict(toy[1]['features']), model.predict(toy[1]['features']))
    model.close(), back.close()


@pytest.mark.parametrize('with_valid_fold', (True, False))
def test_train_knn_search_equals_the_oracle(gpu_required, toy, tmp_path, with_valid_fold):
    ks = SEARCH_KS
    if with_valid_fold:
        searched = toy
        model, train_m, valid_m, test_m = classifier.train_knn_search(*toy, str(tmp_path), ks=ks, num_classes=3)
    else:
        model, train_m, valid_m, test_m = classifier.train_knn_search(toy[0], None, toy[2], str(tmp_path), ks=ks, num_classes=3,
                                                                      valid_ratio=0.25, split_random_state=11)
        ti, vi = usc.stratified_shuffle_split(toy[0]['labels'], 0.25, 11)
        searched = (dict(features=toy[0]['features'][ti], labels=toy[0]['labels'][ti]),
                    dict(features=toy[0]['features'][vi], labels=toy[0]['labels'][vi]), toy[2])
    want = _toy_oracle_any(searched, ks)
    chosen = R.search_choice_ref(ks, [w[1]['accuracy'] for w in want])
    assert train_m['search_params'] == ['n_neighbors'] and train_m['search_params_best_values'] == (chosen,)
    assert valid_m['search_params_best_values'] == (chosen,) and model.n_neighbors == chosen
    at = ks.index(chosen)
    for got, w in ((train_m, want[at][0]), (valid_m, want[at][1]), (test_m, want[at][2])):
        np.testing.assert_equal({k: v for k, v in got.items() if not k.startswith('search')}, w)
    np.testing.assert_equal(valid_m['search'], {(k,): w[1] for k, w in zip(ks, want)})
    np.testing.assert_equal(train_m['search'], {(k,): w[0] for k, w in zip(ks, want)})
    assert os.path.exists(str(tmp_path / 'model.pkl'))


def _toy_oracle_any(splits, ks):
    """_toy_oracle for a training part of any size (lists shorter than max(ks) end empty)"""
    train, valid, test = splits
    X = train['features'].astype(np.int64)
    n = len(X)
    kmax = max(ks)
    loo = np.arange(n)
    lists = [R.topk_ref(R.distances_ref(X, X, 'sqeuclidean'), kmax, loo, loo)[0],
             R.topk_ref(R.distances_ref(valid['features'].astype(np.int64), X, 'sqeuclidean'), kmax)[0],
             R.topk_ref(R.distances_ref(test['features'].astype(np.int64), X, 'sqeuclidean'), kmax)[0]]
    p_train, p_valid = R.vote_ref(lists[0], train['labels'], ks, 3)[1], R.vote_ref(lists[1], train['labels'], ks, 3)[1]
    p_test = R.vote_ref(lists[2], train['labels'], ks, 3, file_idxs=test['file_idxs'])[3]
    out = []
    for s in range(len(ks)):
        m = [classifier.compute_metrics(d['labels'], p[:, s], num_classes=3) for d, p in ((train, p_train), (valid, p_valid), (test, p_test))]
        m[0]['loss'] = m[1]['loss'] = 0
        out.append(m)
    return out


def _write_feature_tree(root, D=24, files_per_fold=6):
    """the 5-fold tree of test_foldbank_gpu's fold driver tests"""
    r = np.random.RandomState(0)
    centres = r.randn(50, D) * 2
    for fold in range(1, 6):
        d = os.path.join(root, 'fold%d' % fold)
        os.makedirs(d)
        for i in range(files_per_fold):
            label = (fold + i) % 3
            frames = (centres[label] + r.randn(r.randint(3, 9), D)).astype(np.float32)
            np.savez(os.path.join(d, 'clip%d.npz' % i), X=frames, y=np.array(label))


@pytest.mark.parametrize('search', (False, True))
def test_train_knn_fold_writes_its_directory(gpu_required, tmp_path, search):
    feats = str(tmp_path / 'features' / 'esc50' / 'l3' / 'x')
    _write_feature_tree(feats)
    if search:
        out = classifier.train_knn_search_fold(feats, str(tmp_path / 'out'), 2, ks=(1, 3, 5), preprocess_device=0, metric='cosine')
    else:
        out = classifier.train_knn_fold(feats, str(tmp_path / 'out'), 2, preprocess_device=0, n_neighbors=3)
    assert os.sep + 'knn' + os.sep in out and os.path.basename(os.path.dirname(out)) == 'fold2'
    assert {'config.json', 'model.pkl', 'results.pkl', 'stdizer.pkl', 'min_max_scaler.pkl'} <= set(os.listdir(out))
    import json
    with open(os.path.join(out, 'config.json')) as fh:
        config = json.load(fh)
    assert config['model_type'] == 'knn' and config['model_id'].endswith('knn') and config['parameter_search'] is search
    with open(os.path.join(out, 'results.pkl'), 'rb') as fh:
        results = pickle.load(fh)
    assert set(results) == {'train', 'valid', 'test'} and 0.0 <= results['test']['accuracy'] <= 1.0 and results['train']['loss'] == 0
    with open(os.path.join(out, 'model.pkl'), 'rb') as fh:
        model = pickle.load(fh)
    assert isinstance(model, knn.KNeighborsClassifier) and model.metric == ('cosine' if search else 'sqeuclidean')
    if search:
        assert config['ks'] == [1, 3, 5] and results['valid']['search_params'] == ['n_neighbors']
        assert model.n_neighbors == results['valid']['search_params_best_values'][0]
    else:
        assert config['n_neighbors'] == 3 and model.n_neighbors == 3


def test_cli_neighbors_round_trips_two_files(gpu_required, tmp_path):
    rng = np.random.RandomState(5)
    A, B = rng.randint(-4, 5, (9, 12)).astype(np.float32), rng.randint(-4, 5, (4, 12)).astype(np.float32)
    np.savez(str(tmp_path / 'A.npz'), X=A, y=np.array(3))
    np.savez(str(tmp_path / 'B.npz'), X=B, y=np.array(1))
    out = str(tmp_path / 'lists.npz')
    cli_knn.main(['neighbors', '--database', str(tmp_path / 'A.npz'), '--queries', str(tmp_path / 'B.npz'), '--k', '3', '--metric',
                  'sqeuclidean', '--out', out])
    with np.load(out) as got:
        widx, wdist = R.topk_ref(R.distances_ref(B.astype(np.int64), A.astype(np.int64), 'sqeuclidean'), 3)
        assert np.array_equal(got['idx'], widx) and np.array_equal(got['dist'].astype(np.float64), wdist)
        assert got['query_frame'].tolist() == [0, 1, 2, 3] and got['database_entry'].tolist() == [0] * 9
        assert got['database_label'].tolist() == [3] * 9 and got['database_names'].tolist() == ['A'] and got['query_names'].tolist() == ['B']
    # the same entry on both sides is one group: nothing of its own is listed
    cli_knn.main(['neighbors', '--database', str(tmp_path / 'A.npz'), str(tmp_path / 'B.npz'), '--queries', str(tmp_path / 'B.npz'),
                  '--k', '3', '--out', out])
    with np.load(out) as got:
        assert np.all(got['database_entry'][got['idx']] == 0)
