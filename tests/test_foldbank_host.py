"""usc.FoldBank, classifier.aggregate_metrics / cross_validate and cli_cross_validate without a GPU: the bank with device=None against
usc.get_split on small written trees (equal element for element and bit for bit), aggregate_metrics against the reference's own
(tests/golden/ref_aggregate.npz), the cross-validation record, the command line, and the host half of l3_feat_assemble in a
stand-alone program under the address and undefined-behaviour sanitizers.

The classifiers themselves fit on the GPU only, so cross_validate's folds against separate train / train_svm_fold calls are in
test_foldbank_gpu.py; here the two fit functions are replaced by a stand-in that computes its metrics from the splits it is given."""
import json
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

from foldbank_ref import assert_same_split, write_tree
from l3embedding_amd import classifier, cli_cross_validate, usc

HERE = os.path.dirname(os.path.abspath(__file__))
STATS = ('mean', 'var', 'min', '25_%ile', '75_%ile', 'median', 'max')


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp('foldbank')
    return {'esc50': write_tree(root / 'a', 'esc50'), 'us8k': write_tree(root / 'b', 'us8k', seed=1),
            'frames': write_tree(root / 'c', 'esc50', seed=2, per_frame_labels=True),
            'dcase2013': write_tree(root / 'd', 'dcase2013', seed=3)}


@pytest.mark.parametrize('valid', [True, False])
@pytest.mark.parametrize('tree', ['esc50', 'us8k', 'frames'])
def test_split_equals_get_split(trees, tree, valid):
    dataset = 'us8k' if tree == 'us8k' else 'esc50'
    with usc.FoldBank(trees[tree], dataset, device=None) as bank:
        assert bank.num_folds == usc.DATASET_NUM_FOLDS[dataset]
        for test_fold in range(bank.num_folds):
            if tree == 'us8k' and (test_fold == 4 or (valid and test_fold == 5)):
                continue          # fold 5 as a test or validation fold: below
            got = bank.split(test_fold, valid=valid)
            want = usc.get_split(trees[tree], test_fold, dataset, valid=valid)
            for g, w in zip(got, want):
                assert_same_split(g, w)
        # a split is the caller's: changing it leaves the bank as it was
        got = bank.split(0, valid=valid)
        got[0]['features'][:] = 0
        assert_same_split(bank.split(0, valid=valid)[0], usc.get_split(trees[tree], 0, dataset, valid=valid)[0])


def test_fold_of_augmented_files_only(trees):
    """us8k fold 5 holds augmented copies only: a training fold like any other, and as a validation or test fold get_fold finds
    no file to take the label shape from (IndexError); the bank fails the same way"""
    with usc.FoldBank(trees['us8k'], 'us8k', device=None) as bank:
        train = bank.split(0)[0]
        assert 'clip1_ps2.npz' in train['filenames']
        for test_fold, valid in ((4, True), (4, False), (5, True)):
            with pytest.raises(IndexError):
                usc.get_split(trees['us8k'], test_fold, 'us8k', valid=valid)
            with pytest.raises(IndexError):
                bank.split(test_fold, valid=valid)
        assert_same_split(bank.split(5, valid=False)[0], usc.get_split(trees['us8k'], 5, 'us8k', valid=False)[0])


def test_augmented_files_are_skipped_and_renumbered(trees):
    with usc.FoldBank(trees['us8k'], 'us8k', device=None) as bank:
        _, held, test = bank.split(1)
        for d in (held, test):
            assert len(d['filenames']) == 6 and len(d['file_idxs']) == 4 and d['file_idxs'][0, 0] == 0
            assert d['file_idxs'][-1, 1] == len(d['features'])


def test_dcase2013_without_training_fold(trees):
    with usc.FoldBank(trees['dcase2013'], 'dcase2013', device=None) as bank:
        for test_fold in (0, 1):
            with pytest.raises(ValueError) as want:
                usc.get_split(trees['dcase2013'], test_fold, 'dcase2013', valid=True)
            with pytest.raises(ValueError) as got:
                bank.split(test_fold, valid=True)
            assert str(got.value) == str(want.value)
            for g, w in zip(bank.split(test_fold, valid=False), usc.get_split(trees['dcase2013'], test_fold, 'dcase2013', valid=False)):
                assert_same_split(g, w)


def test_bank_misuse(trees):
    with pytest.raises(ValueError, match='unknown dataset'):
        usc.FoldBank(trees['esc50'], 'nope', device=None)
    bank = usc.FoldBank(trees['esc50'], 'esc50', device=None)
    bank.close()
    bank.close()
    with pytest.raises(ValueError, match='closed'):
        bank.split(0)


# ---- aggregate_metrics ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 5, 10])
def test_aggregate_metrics_equals_the_reference(n):
    fx = np.load(os.path.join(HERE, 'golden', 'ref_aggregate.npz'))
    keys = ('accuracy', 'loss', 'class_accuracy', 'average_class_accuracy')
    folds = []
    for i in range(n):
        folds.append({k: (fx['n%d_in_%s' % (n, k)][i].tolist() if k == 'class_accuracy' else fx['n%d_in_%s' % (n, k)][i]) for k in keys})
    folds[-1]['only_in_the_last_fold'] = 1.0          # the keys are the first fold's
    with np.errstate(all='ignore'):
        got = classifier.aggregate_metrics(folds)
    assert tuple(got) == keys
    for k in keys:
        assert tuple(got[k]) == STATS
        np.testing.assert_array_equal(np.array([got[k][s] for s in STATS], np.float64), fx['n%d_out_%s' % (n, k)], err_msg=k)


# ---- cross_validate's driver, with a stand-in for the fits ---------------------------------------------------------------------------
def _stand_in_metrics(data, num_classes):
    x = np.asarray(data['features'], np.float64)
    return {'accuracy': float(np.tanh(np.abs(x).mean())), 'class_accuracy': [float(x[:, 0].sum() + c) for c in range(num_classes)],
            'average_class_accuracy': float(x.sum()), 'loss': float((x ** 2).mean()) + float(np.sum(data['labels']))}


def _stand_in_train_svm(train_data, valid_data, test_data, model_dir, num_classes=10, **kwargs):
    assert kwargs.pop('evaluate_on_device') is True
    return (None,) + tuple(_stand_in_metrics(d, num_classes) if d else {} for d in (train_data, valid_data, test_data))


def _stand_in_svm_search(train_data, valid_data, test_data, model_dir, num_classes=10, **kwargs):
    _, tr, va, te = _stand_in_train_svm(train_data, valid_data, test_data, model_dir, num_classes, evaluate_on_device=True)
    record = {'search_params': ['C'], 'search_params_best_values': (1,), 'search': {(1,): dict(va), (10,): dict(va)}}
    tr.update(record), va.update(record)
    return None, tr, va, te


def _load(path):
    with open(path, 'rb') as fh:
        return pickle.load(fh)


@pytest.mark.parametrize('parameter_search', [False, True])
def test_cross_validate_driver_and_record(trees, tmp_path, monkeypatch, parameter_search):
    monkeypatch.setattr(classifier, 'train_svm', _stand_in_train_svm)
    monkeypatch.setattr(classifier, 'train_svm_search', _stand_in_svm_search)
    args = dict(feature_mode='stats', use_min_max=True, non_overlap=True, non_overlap_chunk_size=2, parameter_search=parameter_search)
    out = classifier.cross_validate(trees['esc50'], str(tmp_path / 'cv'), model_type='svm', fold_seed=11, preprocess_device=None, **args)
    assert os.path.dirname(out) == os.path.join(str(tmp_path / 'cv'), 'classifier', 'esc50/l3/x', 'stats', 'non-overlap', 'min-max', 'svm',
                                                 'cross_validation')
    record = _load(os.path.join(out, 'results.pkl'))
    assert sorted(record) == ['aggregate', 'fold_dirs', 'folds', 'test', 'train', 'valid']
    assert record['folds'] == [1, 2, 3, 4, 5] and len(record['fold_dirs']) == 5

    # every fold equals the separate per-fold call made after the same seed: results and both scalers
    for fold_num, fold_dir in zip(record['folds'], record['fold_dirs']):
        assert os.path.basename(os.path.dirname(fold_dir)) == 'fold%d' % fold_num
        assert sorted(os.listdir(fold_dir)) == ['config.json', 'min_max_scaler.pkl', 'results.pkl', 'stdizer.pkl']
        np.random.seed(11)
        alone = classifier.train_svm_fold(trees['esc50'], str(tmp_path / 'alone'), fold_num, preprocess_device=None, **args)
        assert os.path.relpath(alone, str(tmp_path / 'alone')).split(os.sep)[:-1] == \
            os.path.relpath(fold_dir, str(tmp_path / 'cv')).split(os.sep)[:-1]
        assert _load(os.path.join(fold_dir, 'results.pkl')) == _load(os.path.join(alone, 'results.pkl'))
        for name in ('stdizer.pkl', 'min_max_scaler.pkl'):
            a, b = vars(_load(os.path.join(fold_dir, name))), vars(_load(os.path.join(alone, name)))
            assert sorted(a) == sorted(b)
            for k in a:
                np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=name + ' ' + k)
        config = json.load(open(os.path.join(fold_dir, 'config.json')))
        config_alone = json.load(open(os.path.join(alone, 'config.json')))
        for k in ('model_dir', 'output_dir'):
            config.pop(k), config_alone.pop(k)
        assert config == config_alone

    # the record: the folds' metrics as their files hold them, and their aggregates without histories and search records
    numeric = ['accuracy', 'class_accuracy', 'average_class_accuracy', 'loss']
    for part in ('train', 'valid', 'test'):
        per_fold = [_load(os.path.join(d, 'results.pkl'))[part] for d in record['fold_dirs']]
        assert record[part] == per_fold
        if parameter_search and part != 'test':
            assert 'search' in per_fold[0] and 'search_params_best_values' in per_fold[0]
        assert list(record['aggregate'][part]) == numeric
        want = classifier.aggregate_metrics([{k: m[k] for k in numeric} for m in per_fold])
        for k in numeric:
            assert tuple(record['aggregate'][part][k]) == STATS
            for s in STATS:
                assert record['aggregate'][part][k][s] == want[k][s]

    as_json = json.load(open(os.path.join(out, 'results.json')))
    assert sorted(as_json) == sorted(record)
    assert as_json['folds'] == record['folds'] and as_json['fold_dirs'] == record['fold_dirs']
    for part in ('train', 'valid', 'test'):
        assert as_json['aggregate'][part] == {k: {s: float(v) for s, v in stats.items()} for k, stats in record['aggregate'][part].items()}
        assert [m['accuracy'] for m in as_json[part]] == [m['accuracy'] for m in record[part]]
    if parameter_search:
        assert sorted(as_json['valid'][0]['search']) == ['(1,)', '(10,)']


def test_cross_validate_folds_and_global_state(trees, tmp_path, monkeypatch):
    monkeypatch.setattr(classifier, 'train_svm', _stand_in_train_svm)
    out = classifier.cross_validate(trees['esc50'], str(tmp_path / 'a'), folds=[4, 2], fold_seed=None, preprocess_device=None)
    record = _load(os.path.join(out, 'results.pkl'))
    assert record['folds'] == [4, 2]
    assert [os.path.basename(os.path.dirname(d)) for d in record['fold_dirs']] == ['fold4', 'fold2']
    # fold_seed None: the folds draw from the global state one after the other, as consecutive per-fold calls do
    np.random.seed(3)
    out = classifier.cross_validate(trees['esc50'], str(tmp_path / 'b'), folds=[4, 2], preprocess_device=None)
    state = np.random.get_state()
    np.random.seed(3)
    alone = [classifier.train_svm_fold(trees['esc50'], str(tmp_path / 'c'), f) for f in (4, 2)]
    np.testing.assert_array_equal(state[1], np.random.get_state()[1])
    for d, a in zip(_load(os.path.join(out, 'results.pkl'))['fold_dirs'], alone):
        assert _load(os.path.join(d, 'results.pkl')) == _load(os.path.join(a, 'results.pkl'))


def test_cross_validate_refusals(trees, tmp_path):
    with pytest.raises(ValueError) as want:
        classifier.train(trees['esc50'], str(tmp_path), 1, model_type='rf')
    with pytest.raises(ValueError) as got:
        classifier.cross_validate(trees['esc50'], str(tmp_path), model_type='rf', preprocess_device=None)
    assert str(got.value) == str(want.value)
    with pytest.raises(ValueError) as got:
        classifier.cross_validate(trees['esc50'], str(tmp_path), parameter_search=True, parameter_search_valid_fold=False,
                                  preprocess_device=None)
    assert str(got.value) == classifier.NO_SSS
    with pytest.raises(ValueError, match='fold 6 of esc50'):
        classifier.cross_validate(trees['esc50'], str(tmp_path), folds=[1, 6], preprocess_device=None)
    assert not os.path.exists(os.path.join(str(tmp_path), 'classifier'))


def test_preprocess_refuses_device_features_on_the_host():
    class Resident(usc.DeviceFeatures):
        def __init__(self):
            self.device = 0
    split = {'features': Resident(), 'labels': np.zeros(2), 'file_idxs': np.array([[0, 2]])}
    with pytest.raises(ValueError, match='device is None'):
        usc.preprocess_split_data(split, None, dict(split), device=None)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_cli_parsing():
    from l3embedding_amd import cli_classifier
    args = cli_cross_validate.parse_arguments(['-mt', 'mlp', '-e', '7', '--folds', '3', '1', '--fold-seed', '9', 'feats', 'out'])
    assert args['folds'] == [3, 1] and args['fold_seed'] == 9 and args['model_type'] == 'mlp' and args['num_epochs'] == 7
    assert args['features_dir'] == 'feats' and args['output_dir'] == 'out' and 'fold_num' not in args
    args = cli_cross_validate.parse_arguments(['feats', 'out'])
    assert args['folds'] is None and args['fold_seed'] is None and args['model_type'] == 'svm' and args['preprocess_device'] == 0
    assert cli_cross_validate.parse_arguments(['-ppd', '-1', 'feats', 'out'])['preprocess_device'] is None
    # the flag table is cli_classifier's: the same names and, but for the preprocessing device, the same defaults
    single = cli_classifier.parse_arguments(['-mt', 'mlp', 'feats', 'out', '1'])
    assert set(args) == (set(single) - {'fold_num'}) | {'folds', 'fold_seed'}
    assert {k: v for k, v in args.items() if k in single and k not in ('model_type', 'preprocess_device')} == \
        {k: v for k, v in single.items() if k in args and k not in ('model_type', 'preprocess_device')}
    assert single['preprocess_device'] is None
    for argv in (['-mt', 'rf', 'feats', 'out'], ['-psnv', 'feats', 'out'], ['feats', 'out', '3'], ['--folds', 'feats', 'out']):
        with pytest.raises(SystemExit) as e:
            cli_cross_validate.parse_arguments(argv)
        assert e.value.code == 2
    import inspect
    accepted = inspect.signature(classifier.cross_validate).parameters
    assert all(k in accepted for k in ('folds', 'fold_seed', 'preprocess_device', 'features_dir', 'output_dir', 'model_type'))


# ---- the host half of l3_feat_assemble under the sanitizers ---------------------------------------------------------------------------
def test_assemble_plan_under_sanitizers(tmp_path):
    """csrc/feat_assemble.h (the segment checks and the prefix of output rows) in a stand-alone program of its own, built with
    -fsanitize=address,undefined: every refusal of l3_feat_assemble and a valid list, copied on the host by the table"""
    compilers = [c for c in (os.environ.get('CXX'), 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++') if c and shutil.which(c)]
    assert compilers, 'no host C++ compiler found'
    exe = str(tmp_path / 'feat_assemble_main')
    built = None
    for cxx in compilers:
        built = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                                os.path.join(HERE, 'host', 'feat_assemble_main.cpp'), '-o', exe], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stdout.decode(errors='replace')
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert run.returncode == 0 and run.stdout.decode().strip() == 'OK', run.stdout.decode(errors='replace')
