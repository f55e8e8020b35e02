"""The random forest's parameter search over n_estimators on the host (forest.RandomForestClassifier.evaluate / prefix,
classifier.train_rf_search / train_rf_search_fold, cli_forest_search), the device handle replaced by the NumPy oracle
(tests/forest_search_ref.py): a prefix is the smaller fit, the one-pass search equals the loop of train_rf over the grid in every
number, the fold writes the reference's files.  The kernels against the oracle are tests/test_forest_search_gpu.py."""
import inspect
import json
import os
import pickle
import re

import numpy as np
import pytest

import forest_ref as R
import forest_search_ref as S
from test_forest_host import OracleForest, _toy
from l3embedding_amd import _lib, classifier, cli_classifier, cli_forest, cli_forest_search, forest

ScoringOracleForest = S.make_oracle_handle(OracleForest)


@pytest.fixture
def scoring_handle(monkeypatch):
    monkeypatch.setattr(_lib, 'Forest', ScoringOracleForest)
    ScoringOracleForest.scored = []


def _assert_trees_equal(got, want):
    assert sorted(got) == sorted(want)
    for k in R.TREE_ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if k == 'threshold':
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), k


def test_tree_seeds_of_a_smaller_forest_are_a_prefix():
    for seed in (0, 5, 12345678, 20171021):
        whole = forest.tree_seeds(seed, 1000)
        for n in (1, 3, 100, 500):
            assert np.array_equal(forest.tree_seeds(seed, n), whole[:n])


@pytest.mark.parametrize('n', [1, 3, 7])
def test_prefix_is_the_smaller_fit(scoring_handle, n):
    X, y = _toy()
    whole = forest.RandomForestClassifier(n_estimators=7, random_state=11, bin_sample=100).fit(X, y + 5)
    part = whole.prefix(n)
    _assert_trees_equal(part.estimators_, R.fit_forest(X, y, n, 11, 4, bin_sample=100))
    assert part.n_estimators == n and part._h is None and not part._resident and np.array_equal(part.classes_, whole.classes_)
    assert all(np.shares_memory(part.estimators_[k], whole.estimators_[k]) for k in R.TREE_ARRAYS)
    again = pickle.loads(pickle.dumps(part))
    _assert_trees_equal(again.estimators_, part.estimators_)
    want = R.predict_proba(R.fit_forest(X, y, n, 11, 4, bin_sample=100), X)
    assert np.array_equal(again.predict_proba(X), want) and np.array_equal(part.predict(X), 5 + want.argmax(axis=1))
    for bad in (0, 8):
        with pytest.raises(ValueError, match='prefix'):
            whole.prefix(bad)


def test_evaluate_against_predict_proba_of_each_prefix(scoring_handle):
    X, y = _toy()
    m = forest.RandomForestClassifier(n_estimators=7, random_state=2).fit(X, y + 5)
    files = np.array([[0, 1], [1, 42], [42, 240]])
    got = m.evaluate(X, y=y + 5, file_idxs=files, prefixes=(1, 3, 7), outputs=forest.EVALUATE_OUTPUTS)
    fitted = m.evaluate(forest.FITTED_ROWS, prefixes=(1, 3, 7), outputs=('proba',))['proba']
    for g, n in enumerate((1, 3, 7)):
        p = m.prefix(n).predict_proba(X)
        assert np.array_equal(got['proba'][g], p) and np.array_equal(fitted[g], p)
        assert np.array_equal(got['predict'][g], 5 + p.argmax(axis=1)) and got['correct'][g] == (p.argmax(axis=1) == y).sum()
        assert np.array_equal(got['file_predict'][g], 5 + classifier._file_predictions(p, files))
    whole = m.evaluate(X)
    assert sorted(whole) == ['predict'] and np.array_equal(whole['predict'], m.predict(X)[None])
    for kw, msg in ((dict(outputs=('votes',)), 'unknown outputs'), (dict(outputs=('file_mean',)), 'file_idxs'),
                    (dict(outputs=('correct',)), 'needs y'), (dict(y=y, outputs=('correct',)), 'not fitted on')):
        with pytest.raises(ValueError, match=msg):
            m.evaluate(X, **kw)
    with pytest.raises(ValueError, match='expecting 9'):
        m.evaluate(X[:, :4])
    with pytest.raises(ValueError, match='no longer on the GPU'):
        pickle.loads(pickle.dumps(m)).evaluate(forest.FITTED_ROWS)
    with pytest.raises(ValueError, match='no longer on the GPU'):
        m.prefix(3).evaluate(forest.FITTED_ROWS)


def _splits(n_files=6):
    X, y = _toy(n=240)
    files = np.array([[0, 1], [1, 9], [9, 20], [20, 30], [30, 35], [35, 40]][:n_files])
    train, valid = dict(features=X[:160], labels=y[:160]), dict(features=X[160:200], labels=y[160:200])
    test = dict(features=X[200:], labels=np.array([0, 1, 2, 3, 0, 1][:n_files]), file_idxs=files)
    return train, valid, test


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


@pytest.mark.parametrize('on_cut', [False, True])
@pytest.mark.parametrize('train_with_valid', [False, True])
def test_search_equals_the_loop_over_train_rf(scoring_handle, tmp_path, on_cut, train_with_valid):
    train, valid, test = _splits()
    if on_cut:
        train, valid = dict(features=np.vstack((train['features'], valid['features'])),
                            labels=np.concatenate((train['labels'], valid['labels']))), None
    common = dict(num_classes=4, random_state=5, split_random_state=3 if on_cut else None, train_with_valid=train_with_valid,
                  bin_sample=100)
    a_dir, b_dir = str(tmp_path / 'a'), str(tmp_path / 'b')
    os.makedirs(a_dir), os.makedirs(b_dir)
    np.random.seed(9)
    want = classifier.train_param_search(train, valid, test, a_dir, train_func=classifier.train_rf, search_space={'n_estimators': [3, 1, 5]},
                                         **common)
    ScoringOracleForest.scored = []
    np.random.seed(9)
    got = classifier.train_rf_search(train, valid, test, b_dir, n_estimators_grid=[3, 1, 5], n_estimators=77, **common)
    for a, b in zip(got[1:], want[1:]):
        _assert_metrics_equal(a, b)
    assert got[1]['search_params'] == ['n_estimators'] and list(got[2]['search']) == [(3,), (1,), (5,)]
    assert got[1]['loss'] == 0 and got[2]['loss'] == 0 and got[0].n_estimators == got[1]['search_params_best_values'][0]
    _assert_trees_equal(got[0].estimators_, want[0].estimators_)
    # one fit of 5 trees scored at (1, 3, 5): the training rows from the resident matrix, the validation and the test rows from the host
    assert ScoringOracleForest.scored[:3] == [('resident', (1, 3, 5)), ('host', (1, 3, 5)), ('host', (1, 3, 5))]
    assert len(ScoringOracleForest.scored) == (5 if train_with_valid else 3)
    with open(os.path.join(b_dir, 'model.pkl'), 'rb') as fh:
        _assert_trees_equal(pickle.load(fh).estimators_, got[0].estimators_)


def test_ties_go_to_the_earlier_grid_entry_and_bad_grids_are_refused(scoring_handle, tmp_path, monkeypatch):
    train, valid, test = _splits()
    monkeypatch.setattr(classifier, 'compute_metrics', lambda y, pred, num_classes=10: {'accuracy': 0.5, 'class_accuracy': [0.5] * num_classes,
                                                                                       'average_class_accuracy': 0.5})
    for grid in ([3, 1, 5], [5, 3, 1]):
        model, _, valid_metrics, _ = classifier.train_rf_search(train, valid, test, str(tmp_path), n_estimators_grid=grid, num_classes=4)
        assert valid_metrics['search_params_best_values'] == (grid[0],) and model.n_estimators == grid[0]
    monkeypatch.undo()
    for grid in ([], [0], [3, 3], [2.5], [True]):
        with pytest.raises(ValueError, match='n_estimators_grid'):
            classifier.train_rf_search(train, valid, test, str(tmp_path), n_estimators_grid=grid, num_classes=4)
    with pytest.raises(ValueError) as e:          # no validation fold and no seed for the cut
        classifier.train_rf_search(train, None, test, str(tmp_path), n_estimators_grid=[1, 2], num_classes=4)
    assert str(e.value) == classifier.NO_SSS


def test_train_rf_search_fold_writes_the_references_files(scoring_handle, tmp_path):
    fdir = R.write_fold_tree(str(tmp_path))
    out = str(tmp_path / 'out')
    mdir = classifier.train_rf_search_fold(fdir, out, 2, n_estimators_grid=(4, 2, 6), bin_sample=64)
    assert os.path.relpath(mdir, out).split(os.sep)[:8] == ['classifier', 'esc50', 'l3', 'synthetic', 'framewise', 'overlap', 'no-min-max', 'rf']
    assert sorted(os.listdir(mdir)) == ['config.json', 'min_max_scaler.pkl', 'model.pkl', 'results.pkl', 'stdizer.pkl']
    with open(os.path.join(mdir, 'config.json')) as fh:
        config = json.load(fh)
    assert config['parameter_search'] is True and config['n_estimators_grid'] == [4, 2, 6] and config['model_type'] == 'rf'
    assert config['bin_sample'] == 64 and 'n_estimators' not in config and 'model_part' not in config
    with open(os.path.join(mdir, 'results.pkl'), 'rb') as fh:
        results = pickle.load(fh)
    assert list(results['valid']['search']) == [(4,), (2,), (6,)] and list(results['train']['search']) == [(4,), (2,), (6,)]
    assert results['valid']['search_params'] == ['n_estimators'] and results['train']['loss'] == 0 and results['valid']['loss'] == 0
    assert len(results['test']['class_accuracy']) == 50
    with open(os.path.join(mdir, 'model.pkl'), 'rb') as fh:
        model = pickle.load(fh)
    assert (model.n_estimators,) == results['valid']['search_params_best_values'] and model.random_state == 20171021
    # on a cut: refused without its seed before anything is written, run with it
    with pytest.raises(ValueError) as e:
        classifier.train_rf_search_fold(fdir, str(tmp_path / 'none'), 1, parameter_search_valid_fold=False)
    assert str(e.value) == classifier.NO_SSS and not os.path.exists(str(tmp_path / 'none'))
    mdir = classifier.train_rf_search_fold(fdir, out, 1, n_estimators_grid=(2, 3), parameter_search_valid_fold=False,
                                           parameter_search_split_seed=4, parameter_search_train_with_valid=True)
    with open(os.path.join(mdir, 'results.pkl'), 'rb') as fh:
        assert list(pickle.load(fh)['valid']['search']) == [(2,), (3,)]
    # the fold without a search still refuses one, in the driver's own part too
    with pytest.raises(ValueError, match='not built'):
        classifier._rf_part((None, None, None), str(tmp_path), dict(parameter_search=True))


def test_cli_forest_search_flag_table():
    args = cli_forest_search.parse_arguments(['feats', 'out', '3'])
    assert args == dict(random_state=20171021, verbose=False, feature_mode='framewise', non_overlap=False, non_overlap_chunk_size=10,
                        use_min_max=False, preprocess_device=None, parameter_search_valid_fold=True, parameter_search_valid_ratio=0.15,
                        parameter_search_train_with_valid=True, parameter_search_split_seed=None, n_estimators_grid=[100, 500, 1000],
                        features_dir='feats', output_dir='out', fold_num=3)
    accepted = inspect.signature(classifier.train_rf_search_fold).parameters
    assert all(k in accepted for k in args) and 'parameter_search' not in accepted and 'n_estimators' not in accepted
    # cli_forest's flags without -rfne, the search's flags with cli_classifier's dests and defaults
    plain, single = cli_forest.parse_arguments(['feats', 'out', '3']), cli_classifier.parse_arguments(['-mt', 'mlp', 'feats', 'out', '3'])
    assert set(plain) - set(args) == {'n_estimators'} and all(args[k] == v for k, v in plain.items() if k != 'n_estimators')
    assert all(single[k] == args[k] for k in args if k != 'n_estimators_grid')
    args = cli_forest_search.parse_arguments(['--rf-num-estimators-grid', '7', '2', '-psnv', '-psss', '5', '-psvr', '0.2', '-pstwv', '-ppd', '0',
                                              'f', 'o', '1'])
    assert args['n_estimators_grid'] == [7, 2] and not args['parameter_search_valid_fold'] and args['parameter_search_split_seed'] == 5
    assert args['parameter_search_valid_ratio'] == 0.2 and not args['parameter_search_train_with_valid'] and args['preprocess_device'] == 0
    for argv in (['-mt', 'rf', 'f', 'o', '1'], ['f', 'o'], ['f', 'o', '1', '--rf-num-estimators-grid'], ['-rfne', '5', 'f', 'o', '1'],
                 ['--rf-num-estimators-grid', '3', '3', 'f', 'o', '1'], ['--rf-num-estimators-grid', '0', 'f', 'o', '1'], ['-psnv', 'f', 'o', '1']):
        with pytest.raises(SystemExit) as e:
            cli_forest_search.parse_arguments(argv)
        assert e.value.code == 2


def test_the_oracles_file_mean_is_numpys():
    """the rows added one after the other in row order: what np.mean(axis=0) gives on a C-contiguous (rows, C) slice, bit for bit"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'forest_gauss.npz'))
    f = R.fit_forest(g['X'][:300], g['y'][:300], 5, 0, 10)
    proba = R.predict_proba(f, g['Xt'])
    files = [(0, 1), (1, 42), (42, 83), (83, len(proba))]
    assert len(proba) - 83 > 100
    got = S.file_mean(proba, files)
    assert np.array_equal(got, np.stack([proba[s:e].mean(axis=0) for s, e in files]))
    assert np.array_equal(got.argmax(axis=1), classifier._file_predictions(proba, files))
    rs = np.random.RandomState(1)
    for shape in ((41, 10), (1000, 50)):
        p = rs.rand(*shape)
        assert np.array_equal(S.file_mean(p, [(0, shape[0])])[0], p.mean(axis=0))


def test_the_score_entry_is_declared_bound_and_cites_the_reference():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'l3hip.h')) as fh:
        header = fh.read()
    assert 'l3_forest_score' in _lib.SIGNATURES
    comment = header[:header.index('int l3_forest_score(')].rsplit('/*', 1)[1]
    assert 'classifier/train.py:193-227, 623-630' in comment
    args = re.search(r'int l3_forest_score\(([^;]*)\);', header).group(1).split(',')
    assert len(args) == len(_lib.SIGNATURES['l3_forest_score'][1]) == 19
    assert tuple(a.split('*')[-1].strip() for a in args[-5:]) == _lib.FOREST_SCORE_OUTPUTS
