"""Host side of the downstream classifier: fold reading (data/usc/folds.py), preprocessing (data/usc/features.py), metrics
(classifier/metrics.py), the keras-2.0.x callback rules train_mlp relies on, and the 06_train_classifier.py command line."""
import os

import numpy as np
import pytest

from l3embedding_amd import classifier, cli_classifier, usc


def _save(d, name, X, y):
    np.savez(os.path.join(d, name), X=np.asarray(X, np.float32), y=y)


@pytest.fixture
def us8k_dir(tmp_path):
    root = tmp_path / 'features' / 'us8k' / 'l3' / 'x'
    for f in range(10):
        d = root / ('fold%d' % (f + 1))
        d.mkdir(parents=True)
        _save(str(d), 'a%d.npz' % f, np.full((3, 2), f), np.array(f % 10))
        _save(str(d), 'b%d_aug.npz' % f, np.full((2, 2), 100 + f), np.array(f % 10))
    return str(root)


def test_get_fold_listdir_order_and_us8k_skip(us8k_dir):
    fd = os.path.join(us8k_dir, 'fold4')
    names = os.listdir(fd)
    d = usc.get_fold(us8k_dir, 3)
    assert d['filenames'] == names                     # every file listed, the skipped one included
    assert d['features'].shape == (3, 2) and np.all(d['features'] == 3)
    np.testing.assert_array_equal(d['file_idxs'], [[0, 3]])
    np.testing.assert_array_equal(d['labels'], [3])
    aug = usc.get_fold(us8k_dir, 3, augment=True)
    order = [n for n in names]
    rows = [3 if n.startswith('a') else 2 for n in order]
    np.testing.assert_array_equal(aug['file_idxs'], np.column_stack((np.cumsum([0] + rows[:-1]), np.cumsum(rows))))
    assert aug['features'].shape == (5, 2)


def test_get_split_offsets_and_augment_on_train_only(us8k_dir):
    train, valid, test = usc.get_split(us8k_dir, 4, 'us8k')
    # test fold 5 (index 4), valid fold index 3, train the other eight folds with their augmented files
    assert test['features'].shape == (3, 2) and np.all(test['features'] == 4)
    assert valid['features'].shape == (3, 2) and np.all(valid['features'] == 3)
    assert train['features'].shape == (8 * 5, 2)
    assert train['file_idxs'].shape == (16, 2)
    np.testing.assert_array_equal(train['file_idxs'][:, 1][:-1], train['file_idxs'][:, 0][1:])   # contiguous across folds
    assert train['file_idxs'][-1, 1] == 40
    assert len(train['filenames']) == 16
    with pytest.raises(ValueError):
        usc.get_split(us8k_dir, 0, 'nope')


def test_per_frame_labels_and_non_us8k_no_skip(tmp_path):
    root = tmp_path / 'features' / 'esc50' / 'x'
    for f in range(5):
        d = root / ('fold%d' % (f + 1))
        d.mkdir(parents=True)
        _save(str(d), 'c_%d.npz' % f, np.ones((4, 3)) * f, np.arange(4) + f)     # per-frame labels, '_' not skipped
    d = usc.get_fold(str(root), 2)
    np.testing.assert_array_equal(d['labels'], [2, 3, 4, 5])
    assert d['features'].shape == (4, 3)


def test_dcase2013_with_valid_fold_raises(tmp_path):
    root = tmp_path / 'features' / 'dcase2013' / 'x'
    for f in range(2):
        d = root / ('fold%d' % (f + 1))
        d.mkdir(parents=True)
        _save(str(d), 'f.npz', np.ones((2, 3)), np.array(1))
    with pytest.raises(ValueError, match='No training fold left'):
        usc.get_split(str(root), 0, 'dcase2013', valid=True)
    train, valid, test = usc.get_split(str(root), 0, 'dcase2013', valid=False)
    assert valid is None and train['features'].shape == (2, 3)
    assert usc.DATASET_NUM_FOLDS == {'us8k': 10, 'esc50': 5, 'dcase2013': 2}


def test_stats_features_against_scipy():
    stats = pytest.importorskip('scipy.stats')
    x = np.random.RandomState(0).randn(37, 6) ** 3
    got = usc.compute_stats_features(x)
    exp = np.concatenate((x.min(0), x.max(0), np.median(x, 0), x.mean(0), x.var(0), stats.skew(x, axis=0),
                          stats.kurtosis(x, axis=0)))
    np.testing.assert_allclose(got, exp, rtol=1e-10, atol=1e-12)


def test_stats_features_constant_column():
    x = np.ones((5, 2))
    x[:, 1] = [1, 2, 3, 4, 10]
    got = usc.compute_stats_features(x).reshape(7, 2)
    assert got[5, 0] == 0.0 and got[6, 0] == -3.0
    assert got[4, 0] == 0.0


def test_scalers_against_sklearn():
    pre = pytest.importorskip('sklearn.preprocessing')
    r = np.random.RandomState(1)
    X = (r.randn(50, 4) * [1, 10, 0.1, 0]).astype(np.float32)
    Y = r.randn(7, 4).astype(np.float32)
    for ours, theirs in ((usc.StandardScaler(), pre.StandardScaler()), (usc.MinMaxScaler(), pre.MinMaxScaler())):
        np.testing.assert_allclose(ours.fit_transform(X), theirs.fit_transform(X), rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(ours.transform(Y), theirs.transform(Y), rtol=1e-6, atol=1e-6)


def test_scalers_constant_column_and_population_variance():
    X = np.array([[1.0, 5.0], [3.0, 5.0]])
    s = usc.StandardScaler().fit(X)
    np.testing.assert_array_equal(s.var_, [1.0, 0.0])
    np.testing.assert_array_equal(s.scale_, [1.0, 1.0])
    np.testing.assert_array_equal(s.transform(X), [[-1.0, 0.0], [1.0, 0.0]])
    mm = usc.MinMaxScaler().fit(X)
    np.testing.assert_array_equal(mm.transform(X), [[0.0, 0.0], [1.0, 0.0]])


def test_remove_overlap_and_expand_labels():
    data = {'features': np.arange(25, dtype=float).reshape(25, 1), 'file_idxs': np.array([[0, 12], [12, 25]]),
            'labels': np.array([7, 2])}
    usc.remove_data_overlap(data, chunk_size=5)
    np.testing.assert_array_equal(data['features'][:, 0], [0, 5, 10, 12, 17, 22])
    np.testing.assert_array_equal(data['file_idxs'], [[0, 3], [3, 6]])
    usc.expand_framewise_labels(data)
    np.testing.assert_array_equal(data['labels'], [7, 7, 7, 2, 2, 2])


def test_preprocess_split_stats_mode_and_shuffle():
    r = np.random.RandomState(0)
    tr = {'features': r.randn(10, 3), 'labels': np.array([0, 1]), 'file_idxs': np.array([[0, 4], [4, 10]])}
    te = {'features': r.randn(6, 3), 'labels': np.array([1, 0]), 'file_idxs': np.array([[0, 3], [3, 6]])}
    np.random.seed(3)
    usc.preprocess_split_data(tr, None, te, feature_mode='stats')
    assert tr['features'].shape == (2, 21) and te['features'].shape == (2, 21)
    np.testing.assert_allclose(tr['features'].mean(0), 0, atol=1e-12)
    with pytest.raises(ValueError):
        usc.preprocess_split_data({'features': np.ones((2, 1)), 'labels': np.array([0]), 'file_idxs': np.array([[0, 2]])},
                                  None, {'features': np.ones((2, 1)), 'labels': np.array([0]), 'file_idxs': np.array([[0, 2]])},
                                  feature_mode='bogus')


def test_compute_metrics_by_hand():
    y = np.array([0, 0, 1, 2, 2, 2])
    pred = np.array([0, 1, 1, 2, 0, 2])
    m = classifier.compute_metrics(y, pred, num_classes=3)
    assert m['accuracy'] == pytest.approx(4 / 6)
    np.testing.assert_allclose(m['class_accuracy'], [0.5, 1.0, 2 / 3])
    assert m['average_class_accuracy'] == pytest.approx((0.5 + 1 + 2 / 3) / 3)
    onehot = classifier.one_hot(y, 3)
    probs = classifier.one_hot(pred, 3) * 0.9 + 0.01
    assert classifier.compute_metrics(onehot, probs, num_classes=3)['accuracy'] == m['accuracy']


class _Stub(object):
    stop_training = False


def _run_early_stopping(val_losses, patience):
    es = classifier.EarlyStopping(monitor='val_loss', patience=patience)
    es.set_model(_Stub())
    es.on_train_begin()
    for epoch, v in enumerate(val_losses):
        es.on_epoch_end(epoch, {'val_loss': v})
        if es.model.stop_training:
            return epoch
    return None


def test_early_stopping_keras20_rule():
    # [3P] keras 2.0.x: the counter is tested before it is incremented: with patience 2 training stops at the THIRD epoch in a
    # row without improvement (epoch index 4 here), not the second
    assert _run_early_stopping([1.0, 0.9, 0.95, 0.96, 0.97, 0.98, 0.99], patience=2) == 4
    assert _run_early_stopping([1.0, 1.0], patience=0) == 1
    assert _run_early_stopping([1.0, 0.9, 0.8, 0.7], patience=0) is None
    assert _run_early_stopping([1.0, 1.1, 0.5, 0.6, 0.7, 0.8], patience=2) == 5


def test_checkpoint_idx_is_first_minimum():
    mc = classifier.MetricCallback()
    mc.on_train_begin()
    for e, v in enumerate([0.9, 0.5, 0.7, 0.5, 0.6]):
        mc.on_epoch_end(e, {'loss': 1.0, 'acc': 0.5, 'val_loss': v, 'val_acc': 0.1})
    assert int(np.argmin(mc.valid_loss)) == 1


def test_validation_split_takes_the_last_rows(monkeypatch):
    seen = {}

    class FakeMLP(object):
        def __init__(self, D, C, batch, weight_decay=0, seed=0, device=0):
            self.batch = batch

        def set_data(self, X, y, Xv, yv):
            seen.update(X=X, y=y, Xv=Xv, yv=yv)

        def epoch(self, perm, lr, t0):
            seen.setdefault('perms', []).append(np.array(perm))
            return dict(loss=1.0, acc=0.0, val_loss=1.0, val_acc=0.0)

    monkeypatch.setattr(classifier._lib, 'MLP', FakeMLP)
    m, _, _ = classifier.construct_mlp_model((2,), num_classes=3)
    X = np.arange(40, dtype=np.float32).reshape(20, 2)
    y = classifier.one_hot(np.arange(20) % 3, 3)
    m.compile(lr=1e-3)
    m.fit(X, y, batch_size=4, epochs=2, validation_split=0.15, random_state=5)
    split_at = int(20 * 0.85)
    assert split_at == 17
    np.testing.assert_array_equal(seen['X'], X[:17])
    np.testing.assert_array_equal(seen['Xv'], X[17:])
    np.testing.assert_array_equal(seen['yv'], np.arange(17, 20) % 3)
    rs = np.random.RandomState(5)
    np.testing.assert_array_equal(seen['perms'][0], rs.permutation(17))
    np.testing.assert_array_equal(seen['perms'][1], rs.permutation(17))
    assert m.iterations == 2 * 5


def test_cli_flags_and_defaults():
    a = vars(cli_classifier.build_parser().parse_args(['feat', 'out', '3']))
    assert a['num_epochs'] == 150 and a['train_batch_size'] == 64 and a['patience'] == 20
    assert a['model_type'] == 'svm' and a['feature_mode'] == 'framewise'
    assert a['learning_rate'] == 1e-4 and a['weight_decay'] == 1e-5 and a['random_state'] == 20171021
    assert a['parameter_search'] is False and a['parameter_search_valid_fold'] is True
    assert a['parameter_search_train_with_valid'] is True and a['parameter_search_valid_ratio'] == 0.15
    assert a['C'] == 1.0 and a['tol'] == 1e-5 and a['max_iterations'] == -1 and a['kernel'] == 'rbf'
    assert a['n_estimators'] == 100 and a['non_overlap'] is False and a['non_overlap_chunk_size'] == 10
    assert a['use_min_max'] is False and a['fold_num'] == 3
    b = vars(cli_classifier.build_parser().parse_args(
        ['-mt', 'mlp', '-e', '5', '-tbs', '32', '-eap', '3', '-ps', '-pstwv', '-lr', '0.1', '-wd', '0.2', '-fm', 'stats', '-no',
         '-nocs', '4', '-umm', '-r', '9', '-v', 'f', 'o', '1']))
    assert (b['model_type'], b['num_epochs'], b['train_batch_size'], b['patience']) == ('mlp', 5, 32, 3)
    assert b['parameter_search'] and not b['parameter_search_train_with_valid']
    assert (b['learning_rate'], b['weight_decay'], b['feature_mode'], b['random_state']) == (0.1, 0.2, 'stats', 9)
    assert b['non_overlap'] and b['non_overlap_chunk_size'] == '4' and b['use_min_max'] and b['verbose']


@pytest.mark.parametrize('argv,msg', [(['f', 'o', '1'], "only the mlp classifier is built (model_type 'svm'"),
                                      (['-mt', 'rf', 'f', 'o', '1'], "only the mlp classifier is built (model_type 'rf'"),
                                      (['-mt', 'mlp', '-ps', '-psnv', 'f', 'o', '1'], 'StratifiedShuffleSplit')])
def test_cli_rejects_what_is_not_built(capsys, argv, msg):
    with pytest.raises(SystemExit) as ei:
        cli_classifier.parse_arguments(argv)
    assert ei.value.code == 2
    assert msg in capsys.readouterr().err


def test_train_rejects_bad_dataset_and_model(tmp_path):
    with pytest.raises(ValueError, match='only the mlp'):
        classifier.train(str(tmp_path / 'features' / 'us8k'), str(tmp_path), 1, model_type='svm')
    with pytest.raises(ValueError, match='must name a dataset'):
        classifier.train(str(tmp_path / 'features' / 'other' / 'x'), str(tmp_path), 1, model_type='mlp')
    with pytest.raises(ValueError, match='StratifiedShuffleSplit'):
        classifier.train_param_search({}, None, {}, str(tmp_path), None, {'a': [1]})


def _fake_train(tr, va, te, md, **kw):
    acc = {(1e-3, 0.1): 0.7, (1e-3, 0.2): 0.9, (1e-2, 0.1): 0.9, (1e-2, 0.2): 0.1}[(kw['learning_rate'], kw['weight_decay'])]
    return ('model', kw['learning_rate'], kw['weight_decay'], va is None), {'rows': len(tr['labels'])}, {'accuracy': acc}, \
        {'accuracy': acc / 2}


def test_param_search_picks_first_best_and_retrains_on_train_plus_valid():
    tr = {'features': np.zeros((6, 2)), 'labels': np.arange(6)}
    va = {'features': np.ones((3, 2)), 'labels': np.arange(3)}
    grid = {'learning_rate': [1e-3, 1e-2], 'weight_decay': [0.1, 0.2]}
    model, trm, vam, tem = classifier.train_param_search(tr, va, {'x': 1}, '.', _fake_train, grid, train_with_valid=False)
    assert model == ('model', 1e-3, 0.2, False)          # 0.9 first reached at (1e-3, 0.2); (1e-2, 0.1) ties later
    assert trm['search_params_best_values'] == (1e-3, 0.2) and vam['accuracy'] == 0.9 and tem['accuracy'] == 0.45
    assert set(vam['search']) == {(1e-3, 0.1), (1e-3, 0.2), (1e-2, 0.1), (1e-2, 0.2)}
    assert trm['search_params'] == ['learning_rate', 'weight_decay']
    model, trm, _, _ = classifier.train_param_search(tr, va, {'x': 1}, '.', _fake_train, grid, train_with_valid=True)
    assert model == ('model', 1e-3, 0.2, True) and trm['rows'] == 9       # retrained on train + valid, no validation data


def test_fit_with_another_batch_size_after_training_raises(monkeypatch):
    class FakeMLP(object):
        def __init__(self, D, C, batch, weight_decay=0, seed=0, device=0):
            self.batch = batch

        def set_data(self, *a):
            pass

        def epoch(self, perm, lr, t0):
            return dict(loss=1.0, acc=0.0, val_loss=1.0, val_acc=0.0)

        def get_weights(self):
            return [np.zeros(s, np.float32) for s in classifier._lib.mlp_shapes(2, 3)]

        def close(self):
            pass

    monkeypatch.setattr(classifier._lib, 'MLP', FakeMLP)
    m, _, _ = classifier.construct_mlp_model((2,), num_classes=3)
    X, y = np.zeros((8, 2), np.float32), classifier.one_hot(np.arange(8) % 3, 3)
    m.fit(X, y, batch_size=4, epochs=1, validation_split=0.25)
    m.fit(X, y, batch_size=4, epochs=1, validation_split=0.25)       # same batch size: the optimizer state carries on
    with pytest.raises(ValueError, match='reset its optimizer state'):
        m.fit(X, y, batch_size=2, epochs=1, validation_split=0.25)
