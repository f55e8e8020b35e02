"""Scoring a forest at nested sizes on the GPU (l3_forest_score in csrc/forest.hip through forest.RandomForestClassifier.evaluate;
DESIGN.md 8j) and the parameter search over n_estimators built on it (classifier.train_rf_search / train_rf_search_fold): every
size's probabilities are the bits of predict_proba of the forest of its first trees and within 1e-12 of the NumPy oracle
(tests/forest_ref.py), the file means are the oracle's sequential means bit for bit (tests/forest_search_ref.py), the three row
sources, the row chunks, the tree passes and both row paths of the walk (LDS and global memory) give the same bits, and the one-pass
search equals the loop of train_rf over the grid in every number.  The shapes are the smallest at which each path can go wrong."""
import ctypes
import functools
import os
import pickle

import numpy as np
import pytest

import forest_ref as R
import forest_search_ref as S
from l3embedding_amd import _lib, classifier, forest, usc
from l3embedding_amd.forest import FITTED_ROWS, RandomForestClassifier

pytestmark = pytest.mark.gpu
SEED = 7
PASS = 64          # trees per pass of the scoring kernel (SCORE_CHUNK)
STAGE_D = 6144     # the widest row the walk stages in LDS by default (SCORE_STAGE_BYTES / 16)


def _data(n, D, C, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, C, n)
    return (rs.randn(C, D)[y] * 0.8 + rs.randn(n, D)).astype(np.float32), y


# name -> (n, D, classes, trees, prefixes)
CASES = {
    'seven_trees': (600, 12, 4, 7, (1, 3, 7)),
    'fifty_classes': (2000, 33, 50, 5, (2, 5)),                                           # D % 4 != 0, the widest class loop
    'three_passes': (300, 5, 3, 2 * PASS + 22, (PASS - 1, PASS, PASS + 1, 2 * PASS, 2 * PASS + 1, 2 * PASS + 22)),
    'wide_rows': (64, STAGE_D + 1, 3, 3, (1, 3)),                                         # the rows are read from global memory
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (X, y, the fitted forest, the oracle's probabilities of every prefix on X): computed once, shared, never written to"""
    n, D, C, T, prefixes = CASES[name]
    X, y = _data(n, D, C, SEED)
    m = RandomForestClassifier(n_estimators=T, random_state=SEED).fit(X, y)
    want = S.prefix_proba(m.estimators_, X, prefixes)
    for a in (X, y, want):
        a.setflags(write=False)
    return X, y, m, want


def _check(got, m, X, y, prefixes, want):
    """evaluate's proba / predict / correct of rows X against predict_proba of each prefix (bits) and the oracle (1e-12)"""
    assert got['proba'].dtype == np.float64 and got['proba'].shape == (len(prefixes), len(X), m.n_classes_)
    for g, p in enumerate(prefixes):
        assert np.array_equal(got['proba'][g], m.prefix(p).predict_proba(X)), 'prefix %d' % p
        assert np.abs(got['proba'][g] - want[g]).max() <= 1e-12
        assert np.array_equal(got['predict'][g], m.classes_[got['proba'][g].argmax(axis=1)])
        assert got['correct'][g] == (got['predict'][g] == y).sum()


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_prefix_is_predict_proba_of_its_trees(gpu_required, name):
    X, y, m, want = _case(name)
    prefixes = CASES[name][4]
    got = m.evaluate(X, y=y, prefixes=prefixes, outputs=('proba', 'predict', 'correct'))
    _check(got, m, X, y, prefixes, want)
    if name == 'wide_rows':          # the same model with the LDS budget raised to its rows: the staged path, the same bits
        staged = m.evaluate(X, y=y, prefixes=prefixes, outputs=('proba', 'predict', 'correct'), stage_bytes=16 * (STAGE_D + 1))
        assert all(np.array_equal(staged[k], got[k]) for k in got)
    if name == 'seven_trees':        # and with no budget at all: the global-memory path at a small width
        plain = m.evaluate(X, y=y, prefixes=prefixes, outputs=('proba', 'predict', 'correct'), stage_bytes=1)
        assert all(np.array_equal(plain[k], got[k]) for k in got)
        whole = m.evaluate(X, outputs=('proba',))['proba']
        assert whole.shape == (1, 600, 4) and np.array_equal(whole[0], m.predict_proba(X))


def test_a_single_row_and_ragged_row_chunks(gpu_required):
    X, y, m, want = _case('seven_trees')
    prefixes = CASES['seven_trees'][4]
    one = m.evaluate(X[:1], y=y[:1], prefixes=prefixes, outputs=('proba', 'predict', 'correct'))
    _check(one, m, X[:1], y[:1], prefixes, want[:, :1])
    # 599 rows in chunks of 250, 250 and 99: no chunk is a multiple of the workgroup's 4 rows
    whole = m.evaluate(X[:599], y=y[:599], prefixes=prefixes, outputs=('proba', 'predict', 'correct'))
    parts = m.evaluate(X[:599], y=y[:599], prefixes=prefixes, outputs=('proba', 'predict', 'correct'), chunk_rows=250)
    _check(parts, m, X[:599], y[:599], prefixes, want[:, :599])
    assert all(np.array_equal(parts[k], whole[k]) for k in whole)


def test_the_three_row_sources_give_the_same_bits(gpu_required):
    X, y, _, _ = _case('seven_trees')
    prefixes, outputs = (1, 3, 7), ('proba', 'predict', 'correct')
    m = RandomForestClassifier(n_estimators=7, random_state=SEED).fit(X, y)          # its own handle: the rows stay resident in it
    host = m.evaluate(X, y=y, prefixes=prefixes, outputs=outputs)
    resident = m.evaluate(FITTED_ROWS, y=y, prefixes=prefixes, outputs=outputs, chunk_rows=250)
    dev = usc.DeviceFeatures(X, device=0)
    try:
        on_device = m.evaluate(dev, y=y, prefixes=prefixes, outputs=outputs)
        fitted_there = RandomForestClassifier(n_estimators=7, random_state=SEED).fit(dev, y).evaluate(FITTED_ROWS, y=y, prefixes=prefixes,
                                                                                                     outputs=outputs)
    finally:
        dev.close()
    for other in (resident, on_device, fitted_there):
        assert all(np.array_equal(other[k], host[k]) for k in host)
    again = pickle.loads(pickle.dumps(m))
    assert np.array_equal(again.evaluate(X, prefixes=prefixes, outputs=('proba',))['proba'], host['proba'])
    with pytest.raises(ValueError, match='no longer on the GPU'):
        again.evaluate(FITTED_ROWS)


def test_file_means_are_the_sequential_means(gpu_required):
    X, y, m, want = _case('seven_trees')
    prefixes = CASES['seven_trees'][4]
    # files of 1 row and of 41 rows, one across the boundary of the 250-row chunks, rows before, between and after them in no file
    files = np.array([[3, 4], [4, 45], [230, 280], [286, 327], [500, 598]])
    for g in range(len(prefixes)):          # no fixture file is decided by less than 1e-9, so none is excused from the arg-max
        top = np.sort(S.file_mean(want[g], files), axis=1)
        assert (top[:, -1] - top[:, -2]).min() > 1e-9
    for chunk_rows in (0, 250):
        got = m.evaluate(X, file_idxs=files, prefixes=prefixes, outputs=('proba', 'file_mean', 'file_predict'), chunk_rows=chunk_rows)
        assert got['file_mean'].shape == (3, 5, 4)
        for g in range(len(prefixes)):
            assert np.array_equal(got['file_mean'][g], S.file_mean(got['proba'][g], files))
            assert np.array_equal(got['file_predict'][g], m.classes_[classifier._file_predictions(got['proba'][g], files)])
    only = m.evaluate(X, file_idxs=files, prefixes=prefixes, outputs=('file_predict',))['file_predict']          # no proba asked for
    assert np.array_equal(only, got['file_predict'])


def test_a_smaller_fit_has_the_prefixes_trees(gpu_required):
    X, y, m, _ = _case('seven_trees')
    small = RandomForestClassifier(n_estimators=3, random_state=SEED).fit(X, y)
    part = m.prefix(3)
    for k in R.TREE_ARRAYS:
        a, b = small.estimators_[k], part.estimators_[k]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32) if k == 'threshold' else a, b.view(np.uint32) if k == 'threshold' else b), k


def _raw_score(h, X, prefixes):
    """l3_forest_score of host rows for `pred` alone, past the wrapper's own look at the forest -> the return code"""
    x, p = np.ascontiguousarray(X, np.float32), np.asarray(prefixes, np.int32)
    pred = np.empty((p.size, len(x)), np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    return h.lib.l3_forest_score(h.h, vp(x), None, 0, len(x), x.shape[1], 0, vp(p), p.size, None, None, 0, 0, 0, vp(pred), None, None, None, None)


def test_bad_arguments_are_refused_and_the_model_still_scores(gpu_required):
    X, y, m, _ = _case('seven_trees')
    bare = _lib.Forest(0)
    assert _raw_score(bare, X, [1]) == -4          # L3_ESTATE: no forest
    bare.set_trees(m.estimators_, X.shape[1])
    files = np.array([[0, 10]])
    refusals = [
        (dict(resident=True, prefixes=[1]), 'error -4: .*no resident matrix'),
        (dict(X=X[:, :5], prefixes=[1]), 'error -1: .*features'),
        (dict(X=X, prefixes=[]), 'error -1: .*forest sizes'),
        (dict(X=X, prefixes=[3, 3]), 'error -1: .*prefix\\[1\\]'),
        (dict(X=X, prefixes=[3, 1]), 'error -1: .*prefix\\[1\\]'),
        (dict(X=X, prefixes=[0, 3]), 'error -1: .*prefix\\[0\\]'),
        (dict(X=X, prefixes=[8]), 'error -1: .*prefix\\[0\\]'),
        (dict(X=X, prefixes=[7], labels=np.where(y == 0, 4, y), outputs=('correct',)), 'error -1: .*labels'),
        (dict(X=X, prefixes=[7], labels=np.where(y == 0, -1, y), outputs=('correct',)), 'error -1: .*labels'),
        (dict(X=X, prefixes=[7], outputs=('correct',)), 'error -1: .*needs labels'),
        (dict(X=X, prefixes=[7], files=[[590, 601]], outputs=('file_mean',)), 'error -1: .*file 0'),
        (dict(X=X, prefixes=[7], files=[[5, 5]], outputs=('file_pred',)), 'error -1: .*file 0'),
        (dict(X=X, prefixes=[7], files=files, outputs=('pred',)), 'error -1: .*come together'),
        (dict(X=X, prefixes=[7], outputs=('file_mean',)), 'error -1: .*come together'),
        (dict(X=X, prefixes=[7], outputs=()), 'error -1: .*no output'),
    ]
    for kw, msg in refusals:
        with pytest.raises(_lib.L3Error, match=msg):
            bare.score(**kw)
    got = bare.score(X=X, prefixes=[7], labels=y, outputs=('proba', 'correct'))
    assert np.array_equal(got['proba'][0], m.predict_proba(X)) and got['correct'][0] == (m.predict(X) == y).sum()
    bare.close()


# ---- the parameter search over n_estimators, end to end ---------------------------------------------------------------------------
def _assert_metrics_equal(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if k == 'search':
            assert list(a[k]) == list(b[k])
            for point in a[k]:
                _assert_metrics_equal(a[k][point], b[k][point])
        elif k in ('search_params', 'search_params_best_values'):
            assert a[k] == b[k], k
        else:
            assert np.array_equal(np.asarray(a[k], np.float64), np.asarray(b[k], np.float64), equal_nan=True), k


@pytest.mark.parametrize('on_device', [False, True])
@pytest.mark.parametrize('on_cut', [False, True])
def test_search_equals_the_loop_over_train_rf(gpu_required, tmp_path, on_cut, on_device):
    X, y = _data(240, 9, 4, 0)
    files = np.array([[0, 1], [1, 9], [9, 20], [20, 30], [30, 35], [35, 40]])
    parts = [(X[:200], y[:200]), None, (X[200:], np.array([0, 1, 2, 3, 0, 1]))] if on_cut else \
        [(X[:160], y[:160]), (X[160:200], y[160:200]), (X[200:], np.array([0, 1, 2, 3, 0, 1]))]
    outcomes = []
    for run in ('loop', 'search'):
        splits = [None if p is None else dict(features=usc.DeviceFeatures(p[0], device=0) if on_device else p[0], labels=p[1]) for p in parts]
        splits[2]['file_idxs'] = files
        common = dict(num_classes=4, random_state=5, split_random_state=3 if on_cut else None, train_with_valid=True)
        out = str(tmp_path / run)
        os.makedirs(out)
        np.random.seed(9)
        with classifier._closing(splits):
            if run == 'loop':
                outcomes.append(classifier.train_param_search(*splits, out, train_func=classifier.train_rf,
                                                              search_space={'n_estimators': [3, 1, 5]}, **common))
            else:
                outcomes.append(classifier.train_rf_search(*splits, out, n_estimators_grid=[3, 1, 5], **common))
    want, got = outcomes
    for a, b in zip(got[1:], want[1:]):
        _assert_metrics_equal(a, b)
    assert list(got[2]['search']) == [(3,), (1,), (5,)] and got[0].n_estimators == got[2]['search_params_best_values'][0]
    for k in R.TREE_ARRAYS:
        assert np.array_equal(got[0].estimators_[k], want[0].estimators_[k]), k


@pytest.mark.parametrize('device', [None, 0])
def test_train_rf_search_fold_writes_the_fold(gpu_required, tmp_path, device):
    fdir = R.write_fold_tree(str(tmp_path))
    out = str(tmp_path / 'out')
    mdir = classifier.train_rf_search_fold(fdir, out, 1, preprocess_device=device, n_estimators_grid=(10, 4))
    assert sorted(os.listdir(mdir)) == ['config.json', 'min_max_scaler.pkl', 'model.pkl', 'results.pkl', 'stdizer.pkl']
    with open(os.path.join(mdir, 'results.pkl'), 'rb') as fh:
        results = pickle.load(fh)
    assert list(results['valid']['search']) == [(10,), (4,)] and results['valid']['loss'] == 0
    assert results['train']['accuracy'] > 0.9 and results['test']['accuracy'] > 0.5
    with open(os.path.join(mdir, 'model.pkl'), 'rb') as fh:
        assert (pickle.load(fh).n_estimators,) == results['valid']['search_params_best_values']
