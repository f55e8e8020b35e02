"""The host side of the SVM's one-pass grid over C (svm.fit_grid, classifier.train_svm_search / train_svm_fold), without a GPU: the
problems and cross-validation jobs the grid hands to the device against those SVC.fit hands over per cost (a recording stand-in for
_lib.SVM), argument errors, and the fold driver's path and config.json."""
import inspect
import json
import os

import numpy as np
import pytest

from l3embedding_amd import _build, _lib, classifier, svm


class RecordingSVM(object):
    """Stands in for _lib.SVM and records what it is asked: alpha is a fixed function of the problem's rows and its cost, so that
    the same problem at the same cost gives the same support vectors whichever call it arrives in"""
    log = []

    def __init__(self, device=0):
        self.X = None

    def set_data(self, X):
        self.X = np.asarray(X, np.float32)
        RecordingSVM.log.append(('set_data', self.X.shape))

    def fit(self, kernel, problems, cost=1.0, tol=1e-3, max_iter=-1, q=0):
        costs = np.broadcast_to(np.asarray(cost, np.float64), (len(problems),))
        RecordingSVM.log.append(('fit', [(r.copy(), s.copy(), float(c)) for (r, s), c in zip(problems, costs)]))
        alphas = [np.where((rows * 7 + int(c * 10)) % 3 > 0, min(c, 0.5), 0.0) for (rows, _), c in zip(problems, costs)]
        P = len(problems)
        rho = np.array([int(rows.sum()) % 7 * 0.25 + c * 0.01 for (rows, _), c in zip(problems, costs)])
        return alphas, rho, np.array([rows.size for rows, _ in problems], np.int64), np.ones(P, np.int32), np.zeros(P)

    def _dec(self, held, sv, coef, rho):
        return (np.asarray(held, np.float64) % 5 - 2.0) * 0.3 + float(np.sum(coef)) * 0.01 - rho

    def decision(self, kernel, sv_start, coef, rho, X=None, x_idx=None, SV=None, sv_idx=None):
        RecordingSVM.log.append(('decision', (np.array(x_idx), np.array(sv_idx), int(sv_start[1]), np.array(coef).ravel(), float(rho[0]))))
        return self._dec(x_idx, sv_idx, coef, rho[0])[:, None]

    def cv_decision(self, kernel, jobs):
        RecordingSVM.log.append(('cv_decision', [(np.array(h), np.array(sv), int(npos), np.array(cf), float(rho))
                                                 for h, sv, npos, cf, rho in jobs]))
        return [self._dec(h, sv, cf, rho) for h, sv, npos, cf, rho in jobs]

    def close(self):
        pass


def _data(nc=4, n=90, D=5, seed=0):
    r = np.random.RandomState(seed)
    y = np.concatenate((np.arange(n - 3) % (nc - 1), np.full(3, nc - 1)))       # the last class has 3 rows
    r.shuffle(y)
    return r.randn(n, D).astype(np.float32), y * 2 + 5


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert np.array_equal(u, v)


def test_grid_assembles_what_fit_assembles_per_cost(monkeypatch):
    monkeypatch.setattr(_lib, 'SVM', RecordingSVM)
    X, y = _data()
    Cs = (0.1, 1, 10)
    RecordingSVM.log = []
    alone = [svm.SVC(C=c, probability=True, random_state=7).fit(X, y) for c in Cs]
    log = RecordingSVM.log
    RecordingSVM.log = []
    grid = svm.fit_grid(X, y, Cs, platt='host', probability=True, random_state=7)
    glog = RecordingSVM.log
    # the matrix goes up once, everything is solved in one call and scored in one call
    assert [k for k, _ in glog] == ['set_data', 'fit', 'cv_decision']
    fits = [v for k, v in log if k == 'fit']
    assert len(fits) == len(Cs)
    _same(glog[1][1], [pr for f in fits for pr in f])
    assert [c for f in fits for _, _, c in f] == [c for _, _, c in glog[1][1]]
    decisions = [v for k, v in log if k == 'decision']
    _same(glog[2][1], decisions)
    assert len(decisions) > 0 and len(decisions) % len(Cs) == 0
    for m, a in zip(grid, alone):
        for name in ('support_', 'dual_coef_', 'intercept_', 'probA_', 'probB_', 'n_iter_', 'n_support_', 'classes_'):
            assert np.array_equal(getattr(m, name), getattr(a, name)), name
        assert m._resident and m._h is grid[0]._h


def test_grid_helpers_are_the_ones_fit_uses():
    _, y = _data()
    _, yenc = np.unique(y, return_inverse=True)
    groups, pairs, problems, folds = svm.grid_problems(yenc, 4, (1, 2, 3), True, 7)
    assert pairs == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and len(folds) == 3
    cv, sub = svm.cv_problems(problems, 7)
    for f in folds:
        assert len(f[0]) == len(cv) == 5 * len(pairs) and len(f[1]) == len(sub)
        for (p, held, job), (p2, held2, job2) in zip(f[0], cv):
            assert p == p2 and job == job2 and np.array_equal(held, held2)
    assert all(f == ([], []) for f in svm.grid_problems(yenc, 4, (1, 2), False, 7)[3])
    # held-out positions of a pair cover its rows once
    for p in range(len(pairs)):
        held = np.concatenate([h for q, h, _ in cv if q == p])
        assert np.array_equal(np.sort(held), np.arange(problems[p][0].size))


def test_cost_batches():
    assert svm._cost_batches([10, 10, 10, 10, 10], None) == [[0, 1, 2, 3, 4]]
    assert svm._cost_batches([10, 10, 10, 10, 10], 20) == [[0, 1], [2, 3], [4]]
    assert svm._cost_batches([10, 10, 10], 5) == [[0], [1], [2]]
    assert svm._cost_batches([10, 10, 10], 30) == [[0, 1, 2]]


def test_handle_remembers_whose_model_it_holds(monkeypatch):
    class Handle(object):
        sets = 0

        def set_model(self, *a, **kw):
            Handle.sets += 1

    h = Handle()
    models = []
    for c in (1.0, 2.0):
        m = svm.SVC(C=c)
        m._h, m.probability = h, False
        m._sv_start, m._dual_coef_, m._intercept_ = np.zeros(3, np.int64), np.zeros((1, 0)), np.zeros(1)
        m._gamma, m.support_, m.support_vectors_ = 0.5, np.zeros(0, np.int32), np.zeros((0, 2), np.float32)
        models.append(m)
    a, b = models
    for m, want in ((a, 1), (a, 1), (b, 2), (b, 2), (a, 3), (b, 4), (b, 4)):
        m._ensure_model()
        assert Handle.sets == want
    assert a.__getstate__()['_key'] is None and a._key is not None


def test_argument_errors(monkeypatch):
    monkeypatch.setattr(_lib, 'SVM', RecordingSVM)
    X, y = _data()
    with pytest.raises(ValueError, match='Cs is empty'):
        svm.fit_grid(X, y, ())
    for bad in (0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='C <= 0'):
            svm.fit_grid(X, y, (1.0, bad))
    with pytest.raises(ValueError, match='platt must be one of'):
        svm.fit_grid(X, y, (1.0,), platt='numpy')
    with pytest.raises(ValueError, match='come as Cs'):
        svm.fit_grid(X, y, (1.0,), C=2.0)
    with pytest.raises(ValueError, match='kernel must be one of'):
        svm.fit_grid(X, y, (1.0,), kernel='cosine')
    with pytest.raises(ValueError, match='one label per row'):
        svm.fit_grid(X, y[:-1], (1.0,))
    with pytest.raises(ValueError, match='greater than one'):
        svm.fit_grid(X, np.zeros(len(X)), (1.0,))
    with pytest.raises(ValueError, match='validation fold'):
        classifier.train_svm_search({'features': X, 'labels': y}, None, None, '.')


def test_signatures_and_build_flags():
    sig = inspect.signature(svm.fit_grid)
    assert list(sig.parameters)[:4] == ['X', 'y', 'Cs', 'platt'] and sig.parameters['platt'].default == 'device'
    sig = inspect.signature(classifier.train_svm_search)
    assert list(sig.parameters)[:7] == ['train_data', 'valid_data', 'test_data', 'model_dir', 'Cs', 'train_with_valid', 'platt']
    assert sig.parameters['Cs'].default == (0.1, 1, 10, 100, 1000) and sig.parameters['train_with_valid'].default is False
    assert 'preprocess_device' in inspect.signature(classifier.train_svm_fold).parameters
    for name in ('cv_decision', 'fit'):
        assert callable(getattr(_lib.SVM, name))
    assert callable(_lib.svm_sigmoid_train)
    for sym in ('l3_svm_fit_costs', 'l3_svm_cv_decision', 'l3_op_svm_sigmoid_train'):
        assert sym in _lib.SIGNATURES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['svm_eval.hip']


def test_train_svm_fold_path_and_config(monkeypatch, tmp_path):
    """the directory and config.json of train(), with svm in the path; the fit itself is stubbed"""
    fdir = os.path.join(str(tmp_path), 'features', 'us8k', 'l3', 'x')
    seen = {}

    def fake_split(features_dir, fold_idx, dataset, valid=True):
        seen['split'] = (features_dir, fold_idx, dataset, valid)
        return {'features': np.zeros((4, 3), np.float32), 'labels': np.arange(4)}, {'v': 1}, {'t': 1}

    def fake_preprocess(*splits, **kw):
        seen['preprocess'] = kw
        return 'minmax', 'std'

    def fake_train_svm(train, valid, test, model_dir, **kw):
        seen['train_svm'] = kw
        return 'model', {'accuracy': 1.0}, {}, {}

    def fake_search(train, valid, test, model_dir, **kw):
        seen['search'] = kw
        return 'model', {'accuracy': 0.5}, {}, {}

    monkeypatch.setattr(classifier, 'get_split', fake_split)
    monkeypatch.setattr(classifier, 'preprocess_split_data', fake_preprocess)
    monkeypatch.setattr(classifier, 'train_svm', fake_train_svm)
    monkeypatch.setattr(classifier, 'train_svm_search', fake_search)
    out = str(tmp_path / 'out')
    mdir = classifier.train_svm_fold(fdir, out, 3, use_min_max=True, preprocess_device=0, C=4.0, kernel='linear')
    parts = os.path.relpath(mdir, out).split(os.sep)
    assert parts[:8] == ['classifier', 'us8k', 'l3', 'x', 'framewise', 'overlap', 'min-max', 'svm'] and parts[8] == 'fold3'
    assert sorted(os.listdir(mdir)) == ['config.json', 'min_max_scaler.pkl', 'results.pkl', 'stdizer.pkl']
    with open(os.path.join(mdir, 'config.json')) as fh:
        config = json.load(fh)
    assert set(config) == {'username', 'features_dir', 'output_dir', 'model_dir', 'model_id', 'fold_num', 'parameter_search',
                           'parameter_search_valid_fold', 'parameter_search_valid_ratio', 'parameter_search_train_with_valid',
                           'model_type', 'feature_mode', 'train_batch_size', 'patience', 'non_overlap', 'non_overlap_chunk_size',
                           'random_state', 'verbose', 'git_commit', 'gsheet_id', 'google_dev_app_name', 'preprocess_device', 'C',
                           'kernel'}
    assert config['model_type'] == 'svm' and config['model_id'].endswith('min-max/svm') and config['C'] == 4.0
    assert seen['split'] == (fdir, 2, 'us8k', True) and seen['preprocess']['device'] == 0
    assert seen['train_svm'] == dict(evaluate_on_device=True, random_state=20171021, num_classes=10, verbose=False, C=4.0,
                                     kernel='linear')
    mdir = classifier.train_svm_fold(fdir, out, 1, parameter_search=True, parameter_search_train_with_valid=True, platt='host')
    assert seen['search'] == dict(train_with_valid=True, platt='host', random_state=20171021, num_classes=10, verbose=False)
    with open(os.path.join(mdir, 'config.json')) as fh:
        assert 'preprocess_device' not in json.load(fh)
    with pytest.raises(ValueError, match='StratifiedShuffleSplit'):
        classifier.train_svm_fold(fdir, out, 1, parameter_search=True, parameter_search_valid_fold=False)
    # train() itself still runs the MLP alone
    with pytest.raises(ValueError, match='only the mlp classifier is built'):
        classifier.train(fdir, out, 1, model_type='svm')
