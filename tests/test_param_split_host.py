"""The parameter search without a validation fold, without a GPU: usc.stratified_shuffle_split against sklearn's own indices
(tests/golden/stratified_split.npz, written by tests/golden/make_split_golden.py; sklearn is not imported here), the cut and the
retrain of classifier.train_param_search with a stand-in for the fit, the fold drivers and both command lines with the split's
seed, and the host half of l3_feat_split in a stand-alone program under the address and undefined-behaviour sanitizers.

The classifiers themselves fit on the GPU only (test_param_split_gpu.py); here the fits are replaced by stand-ins that compute
their metrics from the splits they are given."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from param_split_ref import GRID_POINTS, load_config, load_pickle, write_tree
from l3embedding_amd import classifier, cli_classifier, cli_cross_validate, usc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'stratified_split.npz'))


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return write_tree(tmp_path_factory.mktemp('param_split'))


# ---- usc.stratified_shuffle_split ---------------------------------------------------------------------------------------------------
def test_split_equals_sklearn(golden):
    assert int(golden['n_cases']) == 10 and str(golden['sklearn_version']) == '1.7.2'
    for k in range(int(golden['n_cases'])):
        labels, ratio, seed = golden['case%d_labels' % k], float(golden['case%d_ratio' % k]), int(golden['case%d_seed' % k])
        train, valid = usc.stratified_shuffle_split(labels, ratio, seed)
        assert train.dtype == np.int64 and valid.dtype == np.int64
        np.testing.assert_array_equal(train, golden['case%d_train' % k], err_msg='case %d' % k)
        np.testing.assert_array_equal(valid, golden['case%d_valid' % k], err_msg='case %d' % k)
        # disjoint, of sklearn's sizes, and the same again from the same seed
        n = labels.size
        assert valid.size == math.ceil(ratio * n) and train.size == n - valid.size
        assert np.unique(np.concatenate((train, valid))).size == n
        again = usc.stratified_shuffle_split(labels, ratio, seed)
        np.testing.assert_array_equal(again[0], train)
        np.testing.assert_array_equal(again[1], valid)
    # what the table of cases is there for
    assert [golden['case%d_train' % k].size for k in (0, 2, 4, 6, 8)] == [11, 340, 7, 85, 2]
    assert np.unique(golden['case0_labels'][golden['case0_valid']]).size == 2          # one of three classes is absent
    assert not np.array_equal(golden['case4_train'], golden['case5_train'])


def test_split_refusals(golden):
    assert int(golden['n_refusals']) == 2
    for k in range(2):
        with pytest.raises(ValueError) as e:
            usc.stratified_shuffle_split(golden['refusal%d_labels' % k], float(golden['refusal%d_ratio' % k]), 0)
        assert str(e.value) == str(golden['refusal%d_message' % k])
    labels = np.arange(8) % 2
    with pytest.raises(ValueError, match='random_state'):
        usc.stratified_shuffle_split(labels, 0.25)
    for ratio in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError, match=r'\(0, 1\) range'):
            usc.stratified_shuffle_split(labels, ratio, 0)
    # string labels are classes like any other (np.unique)
    train, valid = usc.stratified_shuffle_split(np.array(['b', 'a'] * 6), 0.25, 1)
    assert train.size == 9 and valid.size == 3


# ---- train_param_search with a stand-in for the fit ---------------------------------------------------------------------------------
def _search_data(n=40, D=3, seed=0):
    r = np.random.RandomState(seed)
    return ({'features': r.randn(n, D).astype(np.float32), 'labels': np.arange(n) % 4, 'file_idxs': 'not read by the search'},
            {'features': r.randn(5, D).astype(np.float32), 'labels': np.arange(5) % 4})


ACCURACY = {(1e-3, 0.1): 0.7, (1e-3, 0.2): 0.9, (1e-2, 0.1): 0.9, (1e-2, 0.2): 0.1}          # a tie: the first point wins
GRID = {'learning_rate': [1e-3, 1e-2], 'weight_decay': [0.1, 0.2]}


def _recording_fit(calls):
    def fit(tr, va, te, md, **kw):
        calls.append((tr, va, te, dict(kw)))
        acc = ACCURACY[(kw['learning_rate'], kw['weight_decay'])]
        return ('model%d' % len(calls), {'accuracy': acc + 0.01, 'n': len(tr['labels'])}, {'accuracy': acc} if va else {},
                {'accuracy': acc / 2, 'call': len(calls)})
    return fit


@pytest.mark.parametrize('train_with_valid', [True, False])
def test_search_cuts_the_training_rows(tmp_path, train_with_valid):
    train_data, test_data = _search_data()
    X, y = train_data['features'].copy(), train_data['labels'].copy()
    train_idx, valid_idx = usc.stratified_shuffle_split(y, 0.15, 3)
    assert valid_idx.size == 6 and train_idx.size == 34
    calls = []
    model, train_metrics, valid_metrics, test_metrics = classifier.train_param_search(
        train_data, None, test_data, str(tmp_path), _recording_fit(calls), GRID, valid_ratio=0.15, train_with_valid=train_with_valid,
        split_random_state=3, batch_size=7)
    assert len(calls) == 4 + (1 if train_with_valid else 0)
    for (tr, va, te, kw), point in zip(calls, [(1e-3, 0.1), (1e-3, 0.2), (1e-2, 0.1), (1e-2, 0.2)]):
        assert sorted(tr) == sorted(va) == ['features', 'labels'] and te is test_data
        np.testing.assert_array_equal(tr['features'].view(np.uint32), X[train_idx].view(np.uint32))
        np.testing.assert_array_equal(va['features'].view(np.uint32), X[valid_idx].view(np.uint32))
        np.testing.assert_array_equal(tr['labels'], y[train_idx])
        np.testing.assert_array_equal(va['labels'], y[valid_idx])
        assert (kw['learning_rate'], kw['weight_decay'], kw['batch_size']) == point + (7,)
        assert 'split_random_state' not in kw and 'valid_ratio' not in kw
    best = (1e-3, 0.2)
    if train_with_valid:
        tr, va, te, kw = calls[4]          # the whole training set as it is, no validation data, the chosen point
        assert tr is train_data and va is None and te is test_data
        assert (kw['learning_rate'], kw['weight_decay']) == best
        assert model == 'model5' and train_metrics['n'] == 40 and test_metrics['call'] == 5
    else:
        assert model == 'model2' and train_metrics['n'] == 34 and test_metrics['call'] == 2
    # the training data is as it was, and the records have the keys of the validation-fold path
    np.testing.assert_array_equal(train_data['features'], X)
    np.testing.assert_array_equal(train_data['labels'], y)
    with_fold = classifier.train_param_search(train_data, {'features': X[:4], 'labels': y[:4]}, test_data, str(tmp_path),
                                              _recording_fit([]), GRID, train_with_valid=False)
    assert sorted(train_metrics) == sorted(with_fold[1]) and sorted(valid_metrics) == sorted(with_fold[2])
    for m in (train_metrics, valid_metrics):
        assert m['search_params'] == ['learning_rate', 'weight_decay'] and m['search_params_best_values'] == best
        assert list(m['search']) == [(1e-3, 0.1), (1e-3, 0.2), (1e-2, 0.1), (1e-2, 0.2)]
    assert valid_metrics['accuracy'] == 0.9 and valid_metrics['search'][(1e-2, 0.2)] == {'accuracy': 0.1}
    assert train_metrics['search'][best]['n'] == 34


def test_search_without_a_seed_still_refuses(tmp_path):
    train_data, test_data = _search_data()
    for search in (lambda **kw: classifier.train_param_search(train_data, None, test_data, str(tmp_path), _recording_fit([]), GRID, **kw),
                   lambda **kw: classifier.train_svm_search(train_data, None, test_data, str(tmp_path), **kw)):
        with pytest.raises(ValueError) as e:
            search()
        assert str(e.value) == classifier.NO_SSS
        with pytest.raises(ValueError) as e:
            search(split_random_state=None)
        assert str(e.value) == classifier.NO_SSS


# ---- the fold drivers, with stand-ins for the fits ------------------------------------------------------------------------------------
def _stand_in_metrics(data):
    x = np.asarray(data['features'], np.float64)
    return {'accuracy': float(np.tanh(np.abs(x).mean())), 'loss': float((x ** 2).mean()) + float(np.sum(data['labels'])), 'rows': len(x)}


def _stand_in_train_mlp(seen):
    def fit(train_data, valid_data, test_data, model_dir, **kwargs):
        seen.append((len(train_data['labels']), len(valid_data['labels']) if valid_data else None))
        return (None,) + tuple(_stand_in_metrics(d) if d else {} for d in (train_data, valid_data, test_data))
    return fit


SEARCH = dict(parameter_search=True, parameter_search_valid_fold=False)


@pytest.mark.parametrize('train_with_valid', [False, True])
def test_train_with_a_split_seed(tree, tmp_path, monkeypatch, train_with_valid):
    seen = []
    monkeypatch.setattr(classifier, 'train_mlp', _stand_in_train_mlp(seen))
    np.random.seed(2)
    fold_dir = classifier.train(tree, str(tmp_path), 2, model_type='mlp', parameter_search_split_seed=4,
                                parameter_search_train_with_valid=train_with_valid, **SEARCH)
    config = load_config(fold_dir)
    assert config['parameter_search_split_seed'] == 4 and config['parameter_search_valid_fold'] is False
    assert 'preprocess_device' not in config
    # the whole training side (four folds, no validation fold), cut 85 / 15 for the nine grid points, whole for the retrain
    np.random.seed(2)
    splits = usc.get_split(tree, 1, 'esc50', valid=False)
    assert splits[1] is None
    usc.preprocess_split_data(*splits)
    n = len(splits[0]['labels'])
    n_valid = math.ceil(0.15 * n)
    assert seen == [(n - n_valid, n_valid)] * GRID_POINTS + ([(n, None)] if train_with_valid else [])
    results = load_pickle(os.path.join(fold_dir, 'results.pkl'))
    train_idx, valid_idx = usc.stratified_shuffle_split(splits[0]['labels'], 0.15, 4)
    cut = {'features': splits[0]['features'][valid_idx], 'labels': splits[0]['labels'][valid_idx]}
    assert results['valid']['search'][(1e-5, 1e-5)] == _stand_in_metrics(cut)
    assert results['train']['rows'] == (n if train_with_valid else n - n_valid)
    assert results['valid']['search_params'] == ['learning_rate', 'weight_decay']


@pytest.mark.parametrize('model_type', ['mlp', 'svm'])
def test_cross_validate_with_a_split_seed(tree, tmp_path, monkeypatch, model_type):
    seen = []
    monkeypatch.setattr(classifier, 'train_mlp', _stand_in_train_mlp(seen))
    # the SVM's search: the grid's fit and its scoring replaced, the cut and the choice its own
    monkeypatch.setattr(classifier._svm, 'fit_grid', lambda X, y, Cs, **kw: [('svc', c, len(y)) for c in Cs])
    monkeypatch.setattr(classifier, '_svm_metrics_on_device',
                        lambda clf, tr, va, te, num_classes: tuple(_stand_in_metrics(d) if d else {} for d in (tr, va, te)))
    args = dict(model_type=model_type, preprocess_device=None, folds=[1, 3], fold_seed=5, feature_mode='stats',
                parameter_search_split_seed=4, parameter_search_train_with_valid=True, **SEARCH)
    out = classifier.cross_validate(tree, str(tmp_path / 'cv'), **args)
    record = load_pickle(os.path.join(out, 'results.pkl'))
    assert record['folds'] == [1, 3]
    for fold_num, fold_dir in zip(record['folds'], record['fold_dirs']):
        assert load_config(fold_dir)['parameter_search_split_seed'] == 4
        results = load_pickle(os.path.join(fold_dir, 'results.pkl'))
        assert results['train']['rows'] == 24 and results['valid']['rows'] == 4          # 24 files: 20 / 4, retrained on all
        assert results['train']['search'][results['train']['search_params_best_values']]['rows'] == 20
        # the separate per-fold call after the same seed gives the same results
        np.random.seed(5)
        one = classifier.train if model_type == 'mlp' else classifier.train_svm_fold
        alone = one(tree, str(tmp_path / 'alone'), fold_num, **{k: v for k, v in args.items() if k not in ('folds', 'fold_seed') and
                                                               (k != 'model_type' or model_type == 'mlp')})
        assert load_pickle(os.path.join(alone, 'results.pkl')) == results
    if model_type == 'svm':
        assert os.path.exists(os.path.join(record['fold_dirs'][0], 'model.pkl'))
        assert load_pickle(os.path.join(record['fold_dirs'][0], 'model.pkl'))[2] == 24          # the refit on the whole training side


def test_fold_drivers_without_a_seed_still_refuse(tree, tmp_path):
    for call in (lambda: classifier.train(tree, str(tmp_path), 1, model_type='mlp', **SEARCH),
                 lambda: classifier.train_svm_fold(tree, str(tmp_path), 1, **SEARCH),
                 lambda: classifier.cross_validate(tree, str(tmp_path), model_type='mlp', preprocess_device=None, **SEARCH),
                 lambda: classifier.cross_validate(tree, str(tmp_path), preprocess_device=None, parameter_search_split_seed=None, **SEARCH)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == classifier.NO_SSS
    assert not os.path.exists(os.path.join(str(tmp_path), 'classifier'))


# ---- the command lines ------------------------------------------------------------------------------------------------------------
def test_cli_split_seed(capsys):
    flags = ['-ps', '-psnv', '--parameter-search-split-seed', '4']
    args = cli_classifier.parse_arguments(['-mt', 'mlp'] + flags + ['f', 'o', '1'])
    assert args['parameter_search'] and args['parameter_search_valid_fold'] is False and args['parameter_search_split_seed'] == 4
    for mt in ('mlp', 'svm'):
        args = cli_cross_validate.parse_arguments(['-mt', mt] + flags + ['f', 'o'])
        assert args['parameter_search_valid_fold'] is False and args['parameter_search_split_seed'] == 4
    assert cli_classifier.parse_arguments(['-mt', 'mlp', 'f', 'o', '1'])['parameter_search_split_seed'] is None
    assert cli_cross_validate.parse_arguments(['f', 'o'])['parameter_search_split_seed'] is None
    # without the seed: status 2 and the message as before; the single-fold driver still runs the MLP alone
    for parse, argv in ((cli_classifier.parse_arguments, ['-mt', 'mlp', '-ps', '-psnv', 'f', 'o', '1']),
                        (cli_cross_validate.parse_arguments, ['-ps', '-psnv', 'f', 'o'])):
        with pytest.raises(SystemExit) as e:
            parse(argv)
        assert e.value.code == 2 and ('-psnv: ' + classifier.NO_SSS) in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli_classifier.parse_arguments(['-mt', 'svm'] + flags + ['f', 'o', '1'])
    assert e.value.code == 2 and 'only the mlp classifier is built' in capsys.readouterr().err
    import inspect
    for fn in (classifier.train, classifier.train_svm_fold, classifier.cross_validate):
        assert inspect.signature(fn).parameters['parameter_search_split_seed'].default is None


# ---- the host half of l3_feat_split under the sanitizers ------------------------------------------------------------------------------
def test_split_plan_under_sanitizers(tmp_path):
    """csrc/feat_split.h (the checks of the two index tables and the launch geometry) in a stand-alone program of its own, built
    with -fsanitize=address,undefined: an index of -1 and of n in either table, n_a = 0, n_b > 0 with a NULL table, the forms of
    an empty B, the geometry at D = 1 and D = 2^21, and a valid cut copied on the host by the plan"""
    compilers = [c for c in (os.environ.get('CXX'), 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if c and shutil.which(c)]
    assert compilers, 'no host C++ compiler found'
    exe = str(tmp_path / 'feat_split_main')
    built = None
    for cxx in compilers:
        built = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                                os.path.join(HERE, 'host', 'feat_split_main.cpp'), '-o', exe], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stdout.decode(errors='replace')
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0 and run.stdout.decode().strip() == 'OK', run.stdout.decode(errors='replace')
