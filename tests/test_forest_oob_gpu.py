"""Out-of-bag scoring of a forest at nested sizes on the GPU (l3_forest_oob in csrc/forest.hip through
forest.RandomForestClassifier.oob_evaluate and oob_score=True) and the parameter search over n_estimators decided by
it (classifier.train_rf_oob_search / train_rf_oob_fold): every size's sums and tree counts are the NumPy oracle's bit for bit
(tests/forest_oob_ref.py), and its score and decision function are those of a separate fit of that size with oob_score=True; the row
sources, the row chunks, the tree passes and both row paths of the walk (LDS and global memory) give the same bits; the one-pass
search chooses what the loop of separate fits chooses.  The shapes are test_forest_search_gpu.py's: the smallest at which each path
can go wrong."""
import ctypes
import functools
import json
import os
import pickle
import warnings

import numpy as np
import pytest

import forest_oob_ref as O
import forest_ref as R
from l3embedding_amd import _lib, classifier, forest, usc
from l3embedding_amd.forest import FITTED_ROWS, OOB_OUTPUTS, RandomForestClassifier

pytestmark = pytest.mark.gpu
SEED = 7
PASS = 64          # trees per pass of the scoring kernels (SCORE_CHUNK)
STAGE_D = 6144     # the widest row the walk stages in LDS by default (SCORE_STAGE_BYTES / 16)
HERE = os.path.dirname(os.path.abspath(__file__))


def _data(n, D, C, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, C, n)
    return (rs.randn(C, D)[y] * 0.8 + rs.randn(n, D)).astype(np.float32), y + 5          # classes_ are not the class indices


# name -> (n, D, classes, trees, prefixes)
CASES = {
    'seven_trees': (600, 12, 4, 7, (1, 3, 7)),                                            # at 1 tree most rows have no out-of-bag tree
    'fifty_classes': (2000, 33, 50, 5, (2, 5)),                                           # D % 4 != 0, the widest class loop
    'three_passes': (300, 5, 3, 2 * PASS + 22, (PASS - 1, PASS, PASS + 1, 2 * PASS, 2 * PASS + 1, 2 * PASS + 22)),
    'wide_rows': (64, STAGE_D + 1, 3, 3, (1, 3)),                                         # the rows are read from global memory
}


def _quiet(call, *args, **kw):
    """the call without the warning of rows that have no out-of-bag tree (the tests that mean it catch it themselves)"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return call(*args, **kw)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (X, y, the fitted forest, the oracle's (sums, n_oob) at every prefix): computed once, shared, never written to"""
    n, D, C, T, prefixes = CASES[name]
    X, y = _data(n, D, C, SEED)
    m = RandomForestClassifier(n_estimators=T, random_state=SEED).fit(X, y)
    want = O.oob_of_fit(m.estimators_, X, SEED, prefixes)
    for a in (X, y) + want:
        a.setflags(write=False)
    return X, y, m, want


def _check(got, m, y, want):
    """oob_evaluate's five outputs against the oracle's sums and tree counts (bits) and against each other"""
    sums, n_oob = want
    assert got['sums'].dtype == np.float64 and got['sums'].shape == sums.shape and np.array_equal(got['sums'], sums)
    assert got['n_oob'].dtype == np.int32 and np.array_equal(got['n_oob'], n_oob)
    assert np.array_equal(n_oob == 0, sums.sum(axis=2) == 0)
    for g in range(len(sums)):
        assert np.array_equal(got['predict'][g], m.classes_[sums[g].argmax(axis=1)])
        assert got['correct'][g] == (got['predict'][g] == y).sum()
        assert np.array_equal(got['decision'][g], O.decision(sums[g]), equal_nan=True)
        assert np.isnan(got['decision'][g][n_oob[g] == 0]).all() and not np.isnan(got['decision'][g][n_oob[g] > 0]).any()


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_prefix_is_the_oracle_and_a_separate_fit(gpu_required, name):
    X, y, m, want = _case(name)
    prefixes = CASES[name][4]
    got = _quiet(m.oob_evaluate, y=y, prefixes=prefixes, outputs=OOB_OUTPUTS)
    _check(got, m, y, want)
    for g, p in enumerate(prefixes):          # what sklearn's interface gives for a forest of p trees: the same bits
        alone = _quiet(RandomForestClassifier(n_estimators=p, random_state=SEED, oob_score=True).fit, X, y)
        assert alone.oob_score_ == np.mean(got['predict'][g] == y) == got['correct'][g] / len(y), 'prefix %d' % p
        assert np.array_equal(alone.oob_decision_function_, got['decision'][g], equal_nan=True), 'prefix %d' % p
        assert alone.oob_score_ < np.mean(alone.predict(X) == y)          # an inverted mask would score the rows of the bag
    if name == 'wide_rows':          # the same model with the LDS budget raised to its rows: the staged path, the same bits
        staged = _quiet(m.oob_evaluate, y=y, prefixes=prefixes, outputs=OOB_OUTPUTS, stage_bytes=16 * (STAGE_D + 1))
        assert all(np.array_equal(staged[k], got[k], equal_nan=True) for k in got)
    if name == 'seven_trees':
        bare = want[1][0] == 0          # one tree leaves about e^-1 of the rows out: the others have nothing to go by
        assert 0.55 < bare.mean() < 0.70
        assert not got['sums'][0][bare].any() and (got['predict'][0][bare] == m.classes_[0]).all()
        with pytest.warns(UserWarning, match='Some inputs do not have OOB scores'):
            m.oob_evaluate(prefixes=prefixes[:1], outputs=('decision',))
        # with no budget at all: the global-memory path at a small width
        plain = _quiet(m.oob_evaluate, y=y, prefixes=prefixes, outputs=OOB_OUTPUTS, stage_bytes=1)
        assert all(np.array_equal(plain[k], got[k], equal_nan=True) for k in got)
        whole = m.oob_evaluate(y=y)          # the defaults: the whole forest's hits
        assert sorted(whole) == ['correct'] and whole['correct'].shape == (1,) and whole['correct'][0] == got['correct'][2]


def test_a_single_row_and_ragged_row_chunks(gpu_required):
    X, y, _, _ = _case('seven_trees')
    prefixes = CASES['seven_trees'][4]
    # one row: it is in every bag, so no tree scores it
    one = _quiet(RandomForestClassifier(n_estimators=7, random_state=SEED, oob_score=True).fit, X[:1], y[:1])
    got = _quiet(one.oob_evaluate, y=y[:1], prefixes=prefixes, outputs=OOB_OUTPUTS)
    _check(got, one, y[:1], O.oob_of_fit(one.estimators_, X[:1], SEED, prefixes))
    assert not got['n_oob'].any() and one.oob_score_ == 1.0 and np.isnan(one.oob_decision_function_).all()
    # 599 rows in chunks of 250, 250 and 99: the second chunk starts at a row that is no multiple of 64, the third at none of 4's
    m = RandomForestClassifier(n_estimators=7, random_state=SEED).fit(X[:599], y[:599])
    whole = _quiet(m.oob_evaluate, y=y[:599], prefixes=prefixes, outputs=OOB_OUTPUTS)
    parts = _quiet(m.oob_evaluate, y=y[:599], prefixes=prefixes, outputs=OOB_OUTPUTS, chunk_rows=250)
    odd = _quiet(m.oob_evaluate, y=y[:599], prefixes=prefixes, outputs=OOB_OUTPUTS, chunk_rows=61, stage_bytes=1)
    _check(parts, m, y[:599], O.oob_of_fit(m.estimators_, X[:599], SEED, prefixes))
    for other in (parts, odd):
        assert all(np.array_equal(other[k], whole[k], equal_nan=True) for k in whole)


def test_the_row_sources_give_the_same_bits(gpu_required):
    X, y, _, want = _case('seven_trees')
    prefixes = (1, 3, 7)
    m = RandomForestClassifier(n_estimators=7, random_state=SEED).fit(X, y)          # its own handle: the rows stay resident in it
    resident = _quiet(m.oob_evaluate, y=y, prefixes=prefixes, outputs=OOB_OUTPUTS, chunk_rows=250)
    _check(resident, m, y, want)
    assert np.array_equal(m.evaluate(FITTED_ROWS)['predict'][0], m.predict(X))          # the out-of-bag pass left the rows in place
    dev = usc.DeviceFeatures(X, device=0)
    try:
        fitted_there = _quiet(RandomForestClassifier(n_estimators=7, random_state=SEED).fit(dev, y).oob_evaluate, y=y, prefixes=prefixes,
                              outputs=OOB_OUTPUTS)
        again = pickle.loads(pickle.dumps(m))
        with pytest.raises(ValueError, match='no longer on the GPU'):
            again.oob_evaluate(y=y)
        unpickled = _quiet(again.oob_evaluate, y=y, prefixes=prefixes, outputs=OOB_OUTPUTS, X=X)
        unpickled_there = _quiet(pickle.loads(pickle.dumps(m)).oob_evaluate, y=y, prefixes=prefixes, outputs=OOB_OUTPUTS, X=dev)
    finally:
        dev.close()
    passed = _quiet(m.oob_evaluate, y=y, prefixes=prefixes, outputs=OOB_OUTPUTS, X=X)
    for other in (resident, fitted_there, unpickled, unpickled_there):
        assert all(np.array_equal(other[k], passed[k], equal_nan=True) for k in passed)
    with pytest.raises(ValueError, match='no longer on the GPU'):          # rows passed in replace the fit's: they are vouched for, not known
        m.evaluate(FITTED_ROWS)


def test_hand_made_multiplicities_through_the_handle(gpu_required):
    """a tree with every row in its bag, a tree with none, 65 rows: a second 64-row block of the mask kernel with one row in it"""
    X, y, m, _ = _case('seven_trees')
    n, prefixes = 65, (1, 2, 3, 7)
    boot = np.random.RandomState(3).poisson(1.0, (7, n)).astype(np.uint16)
    boot[1] = np.maximum(boot[1], 1)
    boot[2] = 0
    boot[0, 64] = 0          # the last row is out of the first tree's bag
    want = O.oob(m.estimators_, X[:n], boot, prefixes)
    assert not want[1][1][boot[0] > 0].any() and np.array_equal(want[1][2], want[1][1] + 1)
    h = _lib.Forest(0)
    h.set_trees(m.estimators_, X.shape[1])
    h.set_data(X[:n])
    labels = np.searchsorted(m.classes_, y[:n])
    got = h.oob(boot, prefixes=prefixes, labels=labels, outputs=_lib.FOREST_OOB_OUTPUTS)
    assert np.array_equal(got['sums'], want[0]) and np.array_equal(got['n_oob'], want[1])
    assert np.array_equal(got['pred'], want[0].argmax(axis=2)) and got['pred'].dtype == np.int32
    assert np.array_equal(got['correct'], (got['pred'] == labels).sum(axis=1)) and got['correct'].dtype == np.int64
    only = h.oob(boot, prefixes=prefixes, outputs=('n_oob',))          # no sums asked for
    assert sorted(only) == ['n_oob'] and np.array_equal(only['n_oob'], want[1])
    h.close()


def _raw_oob(h, boot, prefixes):
    """l3_forest_oob for `pred` alone, past the wrapper's own look at the forest -> the return code"""
    b, p = np.ascontiguousarray(boot, np.uint16), np.asarray(prefixes, np.int32)
    pred = np.empty((p.size, b.shape[1]), np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    return h.lib.l3_forest_oob(h.h, vp(b), b.shape[0], vp(p), p.size, None, 0, 0, vp(pred), None, None, None)


def test_bad_arguments_are_refused_and_the_handle_still_scores(gpu_required):
    X, y, m, _ = _case('seven_trees')
    n = 65
    boot = forest.bootstrap_counts(forest.tree_seeds(SEED, 7), n)
    labels = np.searchsorted(m.classes_, y[:n])
    bare = _lib.Forest(0)
    assert _raw_oob(bare, boot, [1]) == -4          # L3_ESTATE: no forest
    bare.set_data(X[:n])
    assert _raw_oob(bare, boot, [1]) == -4          # a matrix alone is no forest
    bare.close()
    bare = _lib.Forest(0)
    bare.set_trees(m.estimators_, X.shape[1])
    with pytest.raises(_lib.L3Error, match='error -4: .*no resident matrix'):
        bare.oob(boot, prefixes=[1], outputs=('pred',))
    bare.set_data(X[:n, :5])
    with pytest.raises(_lib.L3Error, match='error -1: .*features'):
        bare.oob(boot, prefixes=[1], outputs=('pred',))
    bare.set_data(X[:n])
    refusals = [
        (dict(boot=boot[:6], prefixes=[1]), 'error -1: .*6 trees'),
        (dict(boot=np.vstack((boot, boot[:1])), prefixes=[1]), 'error -1: .*8 trees'),
        (dict(boot=boot, prefixes=[]), 'error -1: .*forest sizes'),
        (dict(boot=boot, prefixes=[3, 3]), 'error -1: .*prefix\\[1\\]'),
        (dict(boot=boot, prefixes=[3, 1]), 'error -1: .*prefix\\[1\\]'),
        (dict(boot=boot, prefixes=[0, 3]), 'error -1: .*prefix\\[0\\]'),
        (dict(boot=boot, prefixes=[8]), 'error -1: .*prefix\\[0\\]'),
        (dict(boot=boot, prefixes=[7], outputs=('correct',)), 'error -1: .*needs labels'),
        (dict(boot=boot, prefixes=[7], labels=np.where(labels == 0, 4, labels), outputs=('correct',)), 'error -1: .*labels'),
        (dict(boot=boot, prefixes=[7], labels=np.where(labels == 0, -1, labels), outputs=('correct',)), 'error -1: .*labels'),
        (dict(boot=boot, prefixes=[7], outputs=('pred',), chunk_rows=-1), 'error -1: .*chunk_rows'),
        (dict(boot=boot, prefixes=[7], outputs=()), 'error -1: .*no output'),
    ]
    for kw, msg in refusals:
        kw.setdefault('outputs', ('pred',))
        with pytest.raises(_lib.L3Error, match=msg):
            bare.oob(**kw)
    with pytest.raises(ValueError, match='boot must be'):
        bare.oob(boot[:, :64], prefixes=[7], outputs=('pred',))
    got = bare.oob(boot, prefixes=[3, 7], labels=labels, outputs=('sums', 'n_oob', 'correct', 'pred'))
    want = O.oob(m.estimators_, X[:n], boot, [3, 7])
    assert np.array_equal(got['sums'], want[0]) and np.array_equal(got['n_oob'], want[1])
    assert np.array_equal(got['correct'], (got['pred'] == labels).sum(axis=1))
    bare.close()


@pytest.mark.parametrize('name', ['gauss', 'relu'])
def test_the_out_of_bag_score_lies_below_the_training_accuracy(gpu_required, name):
    """no bar against sklearn's spread (DESIGN.md 8l records the figures): the trees are grown out, so the forest knows its own
    training rows, and only a tree that has not seen a row can miss it; an inverted mask would make the two scores equal"""
    g = np.load(os.path.join(HERE, 'golden', 'forest_%s.npz' % name))
    m = RandomForestClassifier(n_estimators=int(g['n_estimators']), random_state=0, oob_score=True).fit(g['X'], g['y'])
    train = np.mean(m.predict(g['X']) == g['y'])
    print('%s: out-of-bag %.4f, training %.4f' % (name, m.oob_score_, train))
    assert m.oob_score_ < train
    assert m.oob_decision_function_.shape == (len(g['y']), 10) and not np.isnan(m.oob_decision_function_).any()
    assert np.abs(m.oob_decision_function_.sum(axis=1) - 1).max() < 1e-12


# ---- the parameter search over n_estimators by out-of-bag accuracy, end to end ------------------------------------------------------
@pytest.mark.parametrize('device', [None, 0])
def test_train_rf_oob_fold_chooses_what_separate_fits_choose(gpu_required, tmp_path, device):
    fdir = R.write_fold_tree(str(tmp_path))
    out = str(tmp_path / 'out')
    grid = (4, 2, 6)
    np.random.seed(9)
    mdir = classifier.train_rf_oob_fold(fdir, out, 2, n_estimators_grid=grid, parameter_search_valid_fold=False, preprocess_device=device,
                                        bin_sample=64)          # no validation fold and no seed: nothing is cut off
    assert sorted(os.listdir(mdir)) == ['config.json', 'min_max_scaler.pkl', 'model.pkl', 'results.pkl', 'stdizer.pkl']
    with open(os.path.join(mdir, 'config.json')) as fh:
        config = json.load(fh)
    assert config['parameter_search'] is True and config['n_estimators_grid'] == list(grid) and config['selection'] == 'oob'
    assert config['parameter_search_valid_fold'] is False and config['parameter_search_valid_ratio'] is None
    assert 'parameter_search_split_seed' not in config and config['model_type'] == 'rf' and config['bin_sample'] == 64
    with open(os.path.join(mdir, 'results.pkl'), 'rb') as fh:
        results = pickle.load(fh)
    with open(os.path.join(mdir, 'model.pkl'), 'rb') as fh:
        model = pickle.load(fh)
    # the fold's training rows again: every fold but the second, preprocessed and shuffled from the same state
    np.random.seed(9)
    with classifier._closing(usc.get_split(fdir, 1, 'esc50', valid=False)) as splits:
        usc.preprocess_split_data(*splits, device=device)
        train = splits[0]
        assert splits[1] is None and len(train['labels']) == 4 * 45          # all four other folds train
        alone = [_quiet(RandomForestClassifier(n_estimators=n, random_state=20171021, oob_score=True, bin_sample=64).fit,
                        train['features'], train['labels']) for n in grid]
    scores = [m.oob_score_ for m in alone]
    best = int(np.argmax(scores))          # the earlier grid entry on ties
    record = results['train']
    assert list(record['oob_search']) == list(record['search']) == [(n,) for n in grid]
    assert [record['oob_search'][(n,)]['accuracy'] for n in grid] == scores
    assert record['search_params'] == ['n_estimators'] and record['search_params_best_values'] == (grid[best],)
    assert record['oob']['accuracy'] == scores[best] and len(record['oob']['class_accuracy']) == 50 and record['loss'] == 0
    assert 'loss' not in record['oob'] and record['oob']['accuracy'] <= record['accuracy'] == record['search'][(grid[best],)]['accuracy']
    assert results['valid']['search_params_best_values'] == (grid[best],) and list(results['valid']['search']) == [(n,) for n in grid]
    assert len(results['test']['class_accuracy']) == 50 and results['test']['accuracy'] > 0.5
    assert model.n_estimators == grid[best] and not hasattr(model, 'oob_score_')
    for k in R.TREE_ARRAYS:
        a, b = model.estimators_[k], alone[best].estimators_[k]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32) if k == 'threshold' else a, b.view(np.uint32) if k == 'threshold' else b), k


def test_train_rf_oob_search_with_a_validation_fold(gpu_required, tmp_path):
    """the validation rows are scored, and with train_with_valid trained on, but do not decide"""
    X, y = _data(240, 9, 4, 0)
    y = y - 5
    files = np.array([[0, 1], [1, 9], [9, 20], [20, 30], [30, 35], [35, 40]])
    train, valid = dict(features=X[:160], labels=y[:160]), dict(features=X[160:200], labels=y[160:200])
    test = dict(features=X[200:], labels=np.array([0, 1, 2, 3, 0, 1]), file_idxs=files)
    model, train_metrics, valid_metrics, test_metrics = classifier.train_rf_oob_search(train, valid, test, str(tmp_path), n_estimators_grid=[3, 1, 5],
                                                                                       num_classes=4, random_state=5, n_estimators=77)
    alone = [_quiet(RandomForestClassifier(n_estimators=n, random_state=5, oob_score=True).fit, X[:160], y[:160]) for n in (3, 1, 5)]
    best = int(np.argmax([m.oob_score_ for m in alone]))
    assert [train_metrics['oob_search'][(n,)]['accuracy'] for n in (3, 1, 5)] == [m.oob_score_ for m in alone]
    assert model.n_estimators == (3, 1, 5)[best] and valid_metrics['search_params_best_values'] == ((3, 1, 5)[best],)
    assert valid_metrics['accuracy'] == np.mean(alone[best].predict(X[160:200]) == y[160:200]) and valid_metrics['loss'] == 0
    assert test_metrics['accuracy'] == np.mean(classifier._file_predictions(alone[best].predict_proba(X[200:]), files) == test['labels'])
    np.random.seed(9)
    merged = classifier.train_rf_oob_search(train, valid, test, str(tmp_path), n_estimators_grid=[3, 1, 5], num_classes=4, random_state=5,
                                            train_with_valid=True)
    np.random.seed(9)
    mix = np.random.permutation(200)
    alone = [_quiet(RandomForestClassifier(n_estimators=n, random_state=5, oob_score=True).fit, X[:200][mix], y[:200][mix]) for n in (3, 1, 5)]
    assert [merged[1]['oob_search'][(n,)]['accuracy'] for n in (3, 1, 5)] == [m.oob_score_ for m in alone]
    with open(os.path.join(str(tmp_path), 'model.pkl'), 'rb') as fh:
        assert np.array_equal(pickle.load(fh).estimators_['counts'], merged[0].estimators_['counts'])
