"""Out-of-bag scoring of the random forest on the host: the oracle's aggregation (tests/forest_oob_ref.py) against the
installed scikit-learn's own oob_score_ and oob_decision_function_, cli_forest_oob's flag table, train_rf_oob_fold's refusals, and
the pickle and prefix rules of forest.RandomForestClassifier's out-of-bag attributes; then, with the device handle replaced by the
NumPy oracles, oob_score=True and oob_evaluate at every prefix against separate fits, and the search and its fold against the loop
of separate fits.  The kernels against the oracle are tests/test_forest_oob_gpu.py."""
import inspect
import json
import os
import pickle
import re
import warnings

import numpy as np
import pytest

import forest_oob_ref as O
import forest_ref as R
import forest_search_ref as S
from test_forest_host import OracleForest, _toy
from l3embedding_amd import _lib, classifier, cli_forest_oob, cli_forest_search, forest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize('trees', [3, 12])
def test_the_oracles_aggregation_is_sklearns(trees):
    """sklearn's own trees and bootstrap samples through the oracle's aggregation: its oob_score_ exactly, its decision to 1e-12"""
    from sklearn.ensemble import RandomForestClassifier
    g = np.load(os.path.join(HERE, 'golden', 'forest_gauss.npz'))
    X, y = g['X'][:300], g['y'][:300]
    n = len(X)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # at 3 trees sklearn warns of the rows without an out-of-bag tree
        clf = RandomForestClassifier(n_estimators=trees, oob_score=True, random_state=0).fit(X, y)
    masks = [np.bincount(np.random.RandomState(est.random_state).randint(0, n, n), minlength=n) == 0 for est in clf.estimators_]
    for mask, sample in zip(masks, clf.estimators_samples_):
        assert np.array_equal(mask, np.bincount(sample, minlength=n) == 0)
    sums, n_oob = O.aggregate([est.predict_proba(X) for est in clf.estimators_], masks, [trees])
    sums, n_oob = sums[0], n_oob[0]
    covered = n_oob > 0
    assert np.array_equal(covered, sums.sum(axis=1) > 0)
    assert np.mean(y == clf.classes_[sums.argmax(axis=1)]) == clf.oob_score_
    diff = np.abs(sums[covered] / n_oob[covered, None] - clf.oob_decision_function_[covered]).max()
    print('%d trees: %d rows without an out-of-bag tree, decision differs by %.3g' % (trees, (~covered).sum(), diff))
    assert diff <= 1e-12
    assert np.abs(O.decision(sums)[covered] - clf.oob_decision_function_[covered]).max() <= 1e-12
    assert np.isnan(O.decision(sums)[~covered]).all()
    if trees == 3:
        assert (~covered).sum() > 0


def test_cli_forest_oob_flag_table():
    args = cli_forest_oob.parse_arguments(['feats', 'out', '3'])
    assert args == dict(random_state=20171021, verbose=False, feature_mode='framewise', non_overlap=False, non_overlap_chunk_size=10,
                        use_min_max=False, preprocess_device=None, parameter_search_valid_fold=True,
                        parameter_search_train_with_valid=True, n_estimators_grid=[100, 500, 1000], features_dir='feats',
                        output_dir='out', fold_num=3)
    accepted = inspect.signature(classifier.train_rf_oob_fold).parameters
    assert all(k in accepted for k in args)
    # train_rf_search_fold's signature without the cut's ratio and seed, cli_forest_search's flags without them
    search = inspect.signature(classifier.train_rf_search_fold).parameters
    assert [k for k in search if k not in ('parameter_search_valid_ratio', 'parameter_search_split_seed')] == list(accepted)
    assert all(accepted[k].default == search[k].default for k in accepted if k != 'model_args')
    whole = cli_forest_search.parse_arguments(['feats', 'out', '3'])
    assert set(whole) - set(args) == {'parameter_search_valid_ratio', 'parameter_search_split_seed'}
    assert all(whole[k] == v for k, v in args.items())
    args = cli_forest_oob.parse_arguments(['--rf-num-estimators-grid', '7', '2', '-psnv', '-pstwv', '-ppd', '0', 'f', 'o', '1'])          # no seed asked for
    assert args['n_estimators_grid'] == [7, 2] and not args['parameter_search_valid_fold']
    assert not args['parameter_search_train_with_valid'] and args['preprocess_device'] == 0
    for argv in (['-psss', '5', 'f', 'o', '1'], ['-psvr', '0.2', 'f', 'o', '1'], ['-mt', 'rf', 'f', 'o', '1'], ['f', 'o'],
                 ['-rfne', '5', 'f', 'o', '1'], ['f', 'o', '1', '--rf-num-estimators-grid'],
                 ['--rf-num-estimators-grid', '3', '3', 'f', 'o', '1'], ['--rf-num-estimators-grid', '0', 'f', 'o', '1']):
        with pytest.raises(SystemExit) as e:
            cli_forest_oob.parse_arguments(argv)
        assert e.value.code == 2


def test_train_rf_oob_fold_refuses_before_anything_is_read(tmp_path):
    out = str(tmp_path / 'out')
    missing = str(tmp_path / 'features' / 'esc50' / 'l3' / 'nowhere')          # never opened: every refusal comes first
    for grid in ([], [0], [3, 3], [2.5], [True]):
        with pytest.raises(ValueError, match='n_estimators_grid'):
            classifier.train_rf_oob_fold(missing, out, 1, n_estimators_grid=grid)
    for cut in (dict(parameter_search_valid_ratio=0.2), dict(parameter_search_split_seed=4)):
        with pytest.raises(ValueError, match='cuts no validation rows off: %s' % list(cut)[0]):
            classifier.train_rf_oob_fold(missing, out, 1, parameter_search_valid_fold=False, **cut)
    with pytest.raises(ValueError, match='must name a dataset'):
        classifier.train_rf_oob_fold(str(tmp_path / 'features' / 'birds' / 'l3'), out, 1)
    assert not os.path.exists(out)
    # the fold's settings say that this search makes no cut: no seed is asked for; the searches on a cut still ask for theirs
    oob = dict(parameter_search=True, parameter_search_valid_fold=False, parameter_search_split_seed=None, search_without_cut=True)
    assert classifier._searches_without_valid_fold(oob) and not classifier._searches_on_a_cut(oob)
    with pytest.raises(ValueError) as e:
        classifier._searches_on_a_cut(dict(oob, search_without_cut=False))
    assert str(e.value) == classifier.NO_SSS
    assert classifier._searches_on_a_cut(dict(oob, search_without_cut=False, parameter_search_split_seed=3))
    assert not classifier._searches_without_valid_fold(dict(oob, parameter_search_valid_fold=True))


def _hand_made(n_estimators=3):
    """a fitted state made by hand: three stumps on feature 0 over two classes"""
    m = forest.RandomForestClassifier(n_estimators=n_estimators, random_state=4, oob_score=True)
    m.classes_, m.n_classes_, m.n_features_, m.max_features_ = np.array([5, 9]), 2, 2, 1
    T = n_estimators
    m.estimators_ = dict(tree_off=np.arange(0, 3 * T + 1, 3, dtype=np.int64), left=np.tile(np.array([1, -1, -1], np.int32), T),
                         right=np.tile(np.array([2, -1, -1], np.int32), T), feature=np.tile(np.array([0, -1, -1], np.int32), T),
                         threshold=np.tile(np.array([0.5, 0, 0], np.float32), T), bin=np.tile(np.array([0, -1, -1], np.int32), T),
                         counts=np.tile(np.array([[2, 2], [2, 0], [0, 2]], np.int32), (T, 1)),
                         n_distinct=np.tile(np.array([4, 2, 2], np.int32), T))
    m.level_stats_ = (np.array([3, 6]), np.array([0, 0]), np.array([0.1, 0.1]))
    m.oob_score_ = np.float64(0.75)
    m.oob_decision_function_ = np.array([[1.0, 0.0], [np.nan, np.nan], [0.0, 1.0], [0.5, 0.5]])
    return m


def test_out_of_bag_attributes_are_neither_pickled_nor_handed_to_a_prefix():
    m = _hand_made()
    again = pickle.loads(pickle.dumps(m))
    part = m.prefix(2)
    for other in (again, part, pickle.loads(pickle.dumps(part))):
        assert other.oob_score is True and not hasattr(other, 'oob_score_') and not hasattr(other, 'oob_decision_function_')
        assert np.array_equal(other.classes_, m.classes_) and other._h is None
    assert hasattr(again, 'level_stats_') and not hasattr(part, 'level_stats_') and part.n_estimators == 2
    assert m.oob_score_ == 0.75 and m.oob_decision_function_.shape == (4, 2)          # the model itself keeps its own
    # a model saved before oob_score existed: its state has no such key
    state = m.__getstate__()
    del state['oob_score']
    old = forest.RandomForestClassifier.__new__(forest.RandomForestClassifier)
    old.__setstate__(state)
    assert old.oob_score is False and old.n_estimators == 3
    assert forest.RandomForestClassifier().oob_score is False


def test_oob_evaluate_refuses_on_the_host():
    m = _hand_made()
    with pytest.raises(ValueError, match='not fitted'):
        forest.RandomForestClassifier().oob_evaluate()
    with pytest.raises(ValueError, match='unknown outputs'):
        m.oob_evaluate(outputs=('proba',))
    with pytest.raises(ValueError, match='needs y'):
        m.oob_evaluate()
    with pytest.raises(ValueError, match='no longer on the GPU'):
        m.oob_evaluate(outputs=('sums',))
    with pytest.raises(ValueError, match='expecting 2'):
        m.oob_evaluate(outputs=('sums',), X=np.zeros((4, 3), np.float32))
    m.random_state = None
    with pytest.raises(ValueError, match='int random_state'):
        m.oob_evaluate(outputs=('sums',), X=np.zeros((4, 2), np.float32))


def test_oob_decision_is_the_rule_and_warns():
    sums = np.array([[1.5, 0.5], [0.0, 0.0], [0.0, 3.0]])
    with pytest.warns(UserWarning, match='Some inputs do not have OOB scores'):
        got = forest.oob_decision(sums)
    assert np.array_equal(got, O.decision(sums), equal_nan=True) and np.isnan(got[1]).all() and got[0, 0] == 0.75
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert np.array_equal(forest.oob_decision(sums[[0, 2]]), [[0.75, 0.25], [0.0, 1.0]])


def test_the_oob_entry_is_declared_bound_and_cites_the_reference():
    with open(os.path.join(os.path.dirname(HERE), 'include', 'l3hip.h')) as fh:
        header = fh.read()
    comment = header[:header.index('int l3_forest_oob(')].rsplit('/*', 1)[1]
    assert 'classifier/train.py:169-227' in comment
    args = re.search(r'int l3_forest_oob\(([^;]*)\);', header).group(1).split(',')
    assert len(args) == len(_lib.SIGNATURES['l3_forest_oob'][1]) == 12
    assert tuple(a.split('*')[-1].strip() for a in args[-4:]) == _lib.FOREST_OOB_OUTPUTS


# ---- the layers above the handle, the handle replaced by the oracles ----------------------------------------------------------------
OobOracleForest = O.make_oracle_handle(S.make_oracle_handle(OracleForest))


@pytest.fixture
def oob_handle(monkeypatch):
    monkeypatch.setattr(_lib, 'Forest', OobOracleForest)


def _quiet(call, *args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return call(*args, **kw)


def test_every_prefix_is_a_separate_fit_with_oob_score(oob_handle):
    X, y = _toy()
    y = y + 5
    prefixes = (1, 3, 7)
    m = forest.RandomForestClassifier(n_estimators=7, random_state=2).fit(X, y)
    assert not hasattr(m, 'oob_score_')
    with pytest.warns(UserWarning, match='Some inputs do not have OOB scores'):
        got = m.oob_evaluate(y=y, prefixes=prefixes, outputs=forest.OOB_OUTPUTS)
    sums, n_oob = O.oob_of_fit(m.estimators_, X, 2, prefixes)
    assert np.array_equal(got['sums'], sums) and np.array_equal(got['n_oob'], n_oob) and (n_oob[0] == 0).mean() > 0.5
    for g, p in enumerate(prefixes):
        alone = _quiet(forest.RandomForestClassifier(n_estimators=p, random_state=2, oob_score=True).fit, X, y)
        assert alone.oob_score_ == np.mean(got['predict'][g] == y) == got['correct'][g] / len(y)
        assert np.array_equal(alone.oob_decision_function_, got['decision'][g], equal_nan=True)
        assert np.array_equal(got['decision'][g], O.decision(sums[g]), equal_nan=True)
        assert np.array_equal(got['predict'][g], m.classes_[sums[g].argmax(axis=1)])
        part = _quiet(m.prefix(p).oob_evaluate, X=X, outputs=('sums',))['sums']          # a prefix draws its own trees' samples
        assert np.array_equal(part[0], sums[g])
    again = pickle.loads(pickle.dumps(m))
    with pytest.raises(ValueError, match='no longer on the GPU'):
        again.oob_evaluate(y=y)
    assert np.array_equal(_quiet(again.oob_evaluate, X=X, prefixes=prefixes, outputs=('sums',))['sums'], sums)
    refit = _quiet(forest.RandomForestClassifier(n_estimators=3, random_state=2, oob_score=True).fit, X, y)
    refit.oob_score = False
    refit.fit(X, y)          # a fit without oob_score leaves no score of an earlier fit behind
    assert not hasattr(refit, 'oob_score_') and not hasattr(refit, 'oob_decision_function_')


@pytest.mark.parametrize('train_with_valid', [False, True])
def test_the_search_chooses_what_separate_fits_choose(oob_handle, tmp_path, train_with_valid):
    X, y = _toy(n=240)
    files = np.array([[0, 1], [1, 9], [9, 20], [20, 30], [30, 35], [35, 40]])
    train, valid = dict(features=X[:160], labels=y[:160]), dict(features=X[160:200], labels=y[160:200])
    test = dict(features=X[200:], labels=np.array([0, 1, 2, 3, 0, 1]), file_idxs=files)
    grid = [3, 1, 5]
    np.random.seed(9)
    model, train_metrics, valid_metrics, test_metrics = _quiet(
        classifier.train_rf_oob_search, train, valid, test, str(tmp_path), n_estimators_grid=grid, num_classes=4, random_state=5,
        train_with_valid=train_with_valid, bin_sample=100, n_estimators=77)
    np.random.seed(9)
    mix = np.random.permutation(200) if train_with_valid else np.arange(160)
    rows, labels = X[:200][mix], y[:200][mix]
    alone = [_quiet(forest.RandomForestClassifier(n_estimators=n, random_state=5, oob_score=True, bin_sample=100).fit, rows, labels)
             for n in grid]
    scores = [m.oob_score_ for m in alone]
    best = int(np.argmax(scores))
    assert [train_metrics['oob_search'][(n,)]['accuracy'] for n in grid] == scores and list(train_metrics['oob_search']) == [(n,) for n in grid]
    assert train_metrics['search_params'] == ['n_estimators'] and train_metrics['search_params_best_values'] == (grid[best],)
    assert valid_metrics['search_params_best_values'] == (grid[best],) and list(valid_metrics['search']) == [(n,) for n in grid]
    assert train_metrics['oob']['accuracy'] == scores[best] and train_metrics['loss'] == 0 and valid_metrics['loss'] == 0
    chosen = alone[best]
    assert model.n_estimators == grid[best] and all(np.array_equal(model.estimators_[k], chosen.estimators_[k]) for k in R.TREE_ARRAYS)
    assert train_metrics['accuracy'] == np.mean(chosen.predict(rows) == labels)
    assert valid_metrics['accuracy'] == np.mean(chosen.predict(X[160:200]) == y[160:200])
    assert test_metrics['accuracy'] == np.mean(classifier._file_predictions(chosen.predict_proba(X[200:]), files) == test['labels'])
    with open(os.path.join(str(tmp_path), 'model.pkl'), 'rb') as fh:
        assert pickle.load(fh).n_estimators == grid[best]
    # without validation rows the record keeps its keys
    _, _, no_valid, _ = _quiet(classifier.train_rf_oob_search, train, None, test, str(tmp_path), n_estimators_grid=grid, num_classes=4,
                               random_state=5, bin_sample=100)
    assert sorted(no_valid) == ['search', 'search_params', 'search_params_best_values'] and list(no_valid['search']) == [(n,) for n in grid]


def test_ties_go_to_the_earlier_grid_entry(oob_handle, tmp_path, monkeypatch):
    X, y = _toy(n=120)
    monkeypatch.setattr(classifier, 'compute_metrics', lambda y, pred, num_classes=10: {'accuracy': 0.5, 'class_accuracy': [0.5] * num_classes,
                                                                                       'average_class_accuracy': 0.5})
    for grid in ([3, 1, 5], [5, 3, 1]):
        model, train_metrics, _, _ = _quiet(classifier.train_rf_oob_search, dict(features=X, labels=y), None, None, str(tmp_path),
                                            n_estimators_grid=grid, num_classes=4)
        assert train_metrics['search_params_best_values'] == (grid[0],) and model.n_estimators == grid[0]


def test_train_rf_oob_fold_writes_the_fold_without_a_cut_or_a_seed(oob_handle, tmp_path):
    fdir = R.write_fold_tree(str(tmp_path))
    out = str(tmp_path / 'out')
    mdir = _quiet(classifier.train_rf_oob_fold, fdir, out, 2, n_estimators_grid=(4, 2, 6), parameter_search_valid_fold=False, bin_sample=64)
    assert os.path.relpath(mdir, out).split(os.sep)[:8] == ['classifier', 'esc50', 'l3', 'synthetic', 'framewise', 'overlap', 'no-min-max', 'rf']
    assert sorted(os.listdir(mdir)) == ['config.json', 'min_max_scaler.pkl', 'model.pkl', 'results.pkl', 'stdizer.pkl']
    with open(os.path.join(mdir, 'config.json')) as fh:
        config = json.load(fh)
    assert config['parameter_search'] is True and config['n_estimators_grid'] == [4, 2, 6] and config['selection'] == 'oob'
    assert config['parameter_search_valid_fold'] is False and config['parameter_search_valid_ratio'] is None
    assert 'parameter_search_split_seed' not in config and 'model_part' not in config and 'search_without_cut' not in config
    with open(os.path.join(mdir, 'results.pkl'), 'rb') as fh:
        results = pickle.load(fh)
    assert list(results['train']['oob_search']) == [(4,), (2,), (6,)] and results['train']['loss'] == 0
    assert len(results['test']['class_accuracy']) == 50 and 'accuracy' not in results['valid']
    with open(os.path.join(mdir, 'model.pkl'), 'rb') as fh:
        model = pickle.load(fh)
    assert (model.n_estimators,) == results['train']['search_params_best_values'] and model.random_state == 20171021
    # with the validation fold: scored, not deciding
    mdir = _quiet(classifier.train_rf_oob_fold, fdir, out, 1, n_estimators_grid=(2, 3))
    with open(os.path.join(mdir, 'results.pkl'), 'rb') as fh:
        results = pickle.load(fh)
    assert results['valid']['loss'] == 0 and list(results['valid']['search']) == [(2,), (3,)]
