"""Nearest neighbours: what can be checked without a GPU -- the oracle against a brute-force double loop, the binding's
signature table against the header, the Python-side refusals, the search's choice rule, cli_knn's parser and pickling."""
import os
import pickle
import re

import numpy as np
import pytest

import knn_ref as R
from l3embedding_amd import _lib, classifier, cli_knn, knn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN_SYMBOLS = ('l3_knn_create', 'l3_knn_destroy', 'l3_knn_set_database', 'l3_knn_set_database_dev', 'l3_knn_set_queries',
               'l3_knn_set_queries_dev', 'l3_knn_query_self', 'l3_knn_matrix', 'l3_knn_list', 'l3_knn_topk', 'l3_knn_vote',
               'l3_op_knn_topk', 'l3_knn_time')


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['sqeuclidean', 'cosine'])
def test_oracle_agrees_with_a_double_loop(metric):
    rng = np.random.RandomState(79)
    Q, X = rng.randint(-2, 3, (7, 4)).astype(np.float32), rng.randint(-2, 3, (9, 4)).astype(np.float32)
    X[5] = X[2]          # a twin: ties
    M = R.distances_ref(Q, X, metric)
    for i in range(7):
        for j in range(9):
            q, c = Q[i].astype(np.float64), X[j].astype(np.float64)
            if metric == 'sqeuclidean':
                want = ((q - c) ** 2).sum()
            else:
                want = 1.0 - (q @ c) / np.sqrt((q @ q) * (c @ c)) if (q @ q) > 0 and (c @ c) > 0 else 1.0
            assert abs(M[i, j] - want) < 1e-12
    gq, gc = np.arange(7) % 3, np.arange(9) % 3
    for k in (1, 4, 9, 12):
        for groups in ((None, None), (gq, gc)):
            idx, dist = R.topk_ref(M, k, *groups)
            bidx, bdist = R.topk_bruteforce(M, k, *groups)
            assert np.array_equal(idx, bidx) and np.array_equal(dist, bdist)
    idx, dist = R.topk_ref(M, 12)
    assert np.all(idx[:, 9:] == -1) and np.all(np.isinf(dist[:, 9:])) and np.all(idx[:, :9] >= 0)


def test_oracle_skips_nan_and_orders_ties_by_index():
    M = np.array([[1.0, np.nan, 0.5, 0.5, 1.0]])
    idx, dist = R.topk_ref(M, 5)
    assert idx.tolist() == [[2, 3, 0, 4, -1]] and dist[0, 4] == np.inf


def test_oracle_votes():
    labels = np.array([0, 1, 1, 2, 0])
    idx = np.array([[0, 1, 2, -1], [3, 4, 0, 1], [-1, -1, -1, -1]])
    counts, pred, fc, fp = R.vote_ref(idx, labels, (1, 2, 4), 3, file_idxs=[(0, 2), (2, 3)])
    assert counts[0].tolist() == [[1, 0, 0], [1, 1, 0], [1, 2, 0]]
    assert pred.tolist() == [[0, 0, 1], [2, 0, 0], [-1, -1, -1]]          # 1-1 ties go to the lower class
    assert fc[0].tolist() == [[1, 0, 1], [2, 1, 1], [3, 3, 1]] and fp.tolist() == [[0, 0, 0], [-1, -1, -1]]


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
def test_every_symbol_is_declared_in_the_binding_and_the_header():
    with open(os.path.join(ROOT, 'include', 'l3hip.h')) as fh:
        header = fh.read()
    for name in KNN_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        found = re.search(r'\b(?:int|void) %s\(([^;]*)\);' % name, header)
        assert found, name
        assert len(found.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
    for name, value in (('L3_KNN_SQEUCLIDEAN', 0), ('L3_KNN_COSINE', 1), ('L3_KNN_TOPK_MAX', _lib.KNN_TOPK_MAX),
                        ('L3_KNN_MAX_SEGMENTS', _lib.KNN_MAX_SEGMENTS), ('L3_KNN_MAX_SIZES', _lib.KNN_MAX_SIZES),
                        ('L3_KNN_MAX_CLASSES', _lib.KNN_MAX_CLASSES)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name
    assert _lib.KNN_TOPK_MAX == _lib.PAIRS_TOPK_MAX == 64
    assert _lib.KNN_METRICS == {'sqeuclidean': 0, 'cosine': 1}


def test_binding_refuses_bad_arguments_before_the_device():
    with pytest.raises(ValueError):
        _lib.KNN(0)
    with pytest.raises(ValueError):
        _lib.KNN(8, metric='manhattan')
    h = _lib.KNN(8)
    for bad in (None, np.zeros((3, 8), np.float64), np.zeros((3, 7), np.float32), np.zeros((0, 8), np.float32), np.zeros(8, np.float32)):
        with pytest.raises(ValueError):
            h.set_database(bad)
    with pytest.raises(ValueError):
        h.set_database(np.zeros((3, 8), np.float32), labels=[0, 1])
    with pytest.raises(ValueError):
        h.set_database(np.zeros((3, 8), np.float32), labels=[0, -1, 1])
    with pytest.raises(ValueError):
        h.query_self()
    with pytest.raises(ValueError):
        h.topk(5)          # nothing set
    assert h.h is None          # no call reached the device
    for k in (0, 65, True, 2.0):
        with pytest.raises(ValueError):
            _lib.knn_check_k(k)
    for ks in ((), (0, 1), (3, 2), (2, 2), (1, 6), tuple(range(1, 10)), (1.5,)):
        with pytest.raises(ValueError):
            _lib.knn_check_sizes(ks, 5)
    assert _lib.knn_check_sizes((1, 3, 5), 5).tolist() == [1, 3, 5]
    with pytest.raises(ValueError):
        _lib._knn_groups(np.zeros(3, np.int32), None, 3, 4)
    with pytest.raises(ValueError):
        _lib._knn_groups(np.zeros(3, np.int32), np.zeros(3, np.int32), 3, 4)
    with pytest.raises(ValueError):
        _lib.op_knn_topk(np.zeros((2, 4)), np.zeros((3, 5)), 1)
    with pytest.raises(ValueError):
        _lib.op_knn_topk(np.zeros((2, 4)), np.zeros((3, 4)), 1, segments=257)


def test_python_classes_refuse_bad_arguments():
    with pytest.raises(ValueError):
        knn.NearestNeighbors(n_neighbors=0)
    with pytest.raises(ValueError):
        knn.NearestNeighbors(n_neighbors=65)
    with pytest.raises(ValueError):
        knn.NearestNeighbors(metric='l1')
    with pytest.raises(ValueError):
        knn.KNeighborsClassifier(num_classes=257)
    nn = knn.NearestNeighbors()
    with pytest.raises(ValueError):
        nn.kneighbors()          # not fitted
    with pytest.raises(ValueError):
        nn.fit(np.zeros((4, 3)))          # float64
    with pytest.raises(ValueError):
        nn.fit(np.zeros(3, np.float32))
    clf = knn.KNeighborsClassifier(num_classes=3)
    X = np.zeros((4, 3), np.float32)
    for y in ([0, 1, 2], [0, 1, 2, 3], [0, -1, 1, 2], [0.5, 1, 2, 0]):
        with pytest.raises(ValueError):
            clf.fit(X, y)
    with pytest.raises(ValueError):
        clf.fit(X, [0, 1, 2, 0], groups=[1, 2])
    clf.fit(X, [0, 1, 2, 0])
    assert clf._h is None and clf.classes_.tolist() == [0, 1, 2]          # host rows: nothing touched the device
    with pytest.raises(ValueError):
        clf.evaluate(outputs=('proba',))
    with pytest.raises(ValueError):
        clf.evaluate(ks=(5, 3))
    with pytest.raises(ValueError):
        clf.evaluate(ks=(1, 70))
    with pytest.raises(ValueError):
        clf.evaluate(X, groups=[0, 1, 2, 3])          # fit had no groups


def test_pickling_keeps_rows_and_labels_and_no_handle():
    X = np.arange(12, dtype=np.float32).reshape(4, 3)
    clf = knn.KNeighborsClassifier(n_neighbors=3, metric='cosine', num_classes=5).fit(X, [0, 4, 2, 0], groups=[7, 7, 8, 9])
    back = pickle.loads(pickle.dumps(clf))
    assert back._h is None and back.n_neighbors == 3 and back.metric == 'cosine' and back.shape_fit_ == (4, 3)
    assert np.array_equal(back._X, X) and back._labels.tolist() == [0, 4, 2, 0] and back._groups.tolist() == [7, 7, 8, 9]
    other = clf.with_neighbors(1)
    assert other.n_neighbors == 1 and other._X is clf._X and clf.n_neighbors == 3


# ---- the search ------------------------------------------------------------------------------------------------------------------------
def _chosen(ks, accuracies):
    """the size classifier._search keeps when the grid's validation accuracies are these (the body of train_knn_search)"""
    split = dict(features=np.zeros((2, 1), np.float32), labels=np.zeros(2, np.int64))

    def run_grid(train, valid):
        return [((k,), 'model%d' % k, {'accuracy': 0.0}, {'accuracy': a}, {}) for k, a in zip(ks, accuracies)]

    model, _, valid_metrics, _ = classifier._search(split, split, ['n_neighbors'], 0.15, None, False, run_grid, None)
    assert model == 'model%d' % valid_metrics['search_params_best_values'][0]
    return valid_metrics['search_params_best_values'][0]


def test_search_sizes_and_choice_rule():
    assert classifier.KNN_SEARCH_KS == (1, 3, 5, 10, 20, 50)
    ks = list(classifier.KNN_SEARCH_KS)
    for acc in ([0.5, 0.7, 0.7, 0.6, 0.7, 0.1], [0.9] * 6, [0.1, 0.2, 0.3, 0.4, 0.5, 0.6], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]):
        assert _chosen(ks, acc) == R.search_choice_ref(ks, acc)
    assert _chosen(ks, [0.5, 0.7, 0.7, 0.6, 0.7, 0.1]) == 3          # ties in accuracy pick the smaller k
    # from hand-made vote tables: labels 0 / 1; at k = 1 and at k = 5 two of three queries are right, at k = 3 none
    labels = np.array([0, 0, 1, 1, 1])
    idx = np.array([[0, 2, 3, 1, 4], [2, 0, 1, 3, 4], [0, 1, 2, 3, 4]])
    truth = np.array([0, 1, 1])
    _, pred = R.vote_ref(idx, labels, (1, 3, 5), 2)
    assert pred.tolist() == [[0, 1, 1], [1, 0, 1], [0, 0, 1]]
    acc = [classifier.compute_metrics(truth, pred[:, s], num_classes=2)['accuracy'] for s in range(3)]
    assert acc[0] == acc[2] > acc[1] == 0.0
    assert _chosen([1, 3, 5], acc) == R.search_choice_ref([1, 3, 5], acc) == 1
    for bad in ((), (0, 1), (1, 1), (1, 65), tuple(range(1, 10)), (1.0,)):
        with pytest.raises(ValueError):
            classifier._knn_sizes(bad)
    with pytest.raises(ValueError):          # train() keeps refusing every type but the MLP
        classifier.train('x/features/us8k/l3', 'out', 1, model_type='knn')


# ---- the command line --------------------------------------------------------------------------------------------------------------------
def test_cli_parser():
    cmd, args = cli_knn.parse_arguments(['fold', 'feats/features/us8k/l3', 'out', '3'])
    assert cmd == 'fold' and args['n_neighbors'] == 5 and args['metric'] == 'sqeuclidean' and args['parameter_search'] is False
    assert args['fold_num'] == 3 and args['feature_mode'] == 'framewise' and args['random_state'] == 20171021
    assert args['preprocess_device'] is None and args['non_overlap_chunk_size'] == 10 and args['use_min_max'] is False
    cmd, args = cli_knn.parse_arguments(['fold', '-knn', '10', '--metric', 'cosine', '--parameter-search', '-ppd', '0', 'f', 'o', '1'])
    assert args['n_neighbors'] == 10 and args['metric'] == 'cosine' and args['parameter_search'] is True and args['preprocess_device'] == 0
    cmd, args = cli_knn.parse_arguments(['neighbors', '--database', 'A.npz', '--queries', 'B.npz', '--k', '7', '--metric', 'cosine',
                                         '--out', 'lists.npz'])
    assert cmd == 'neighbors' and args == dict(database=['A.npz'], queries=['B.npz'], k=7, metric='cosine', device=0, out='lists.npz')
    for bad in (['fold', '-knn', '0', 'f', 'o', '1'], ['fold', '--metric', 'l1', 'f', 'o', '1'],
                ['neighbors', '--database', 'A.npz', '--queries', 'B.npz', '--k', '65', '--out', 'x.npz'], ['neighbors', '--out', 'x.npz'], []):
        with pytest.raises(SystemExit):
            cli_knn.parse_arguments(bad)
