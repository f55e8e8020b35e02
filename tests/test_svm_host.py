"""The SVM classifier's host side (classifier/train.py:79-166, l3embedding_amd/svm.py), without a GPU: the float64 restatement
(tests/svm_ref.py) against the scikit-learn fixtures of tests/golden/svm_*.npz, libsvm's probability coupling and sklearn's
ovr transform reproduced from sklearn's own decision values, hinge_loss, and train_svm's metric and per-file shell with a fake
solver handle."""
import os
import pickle

import numpy as np
import pytest

import svm_ref as ref
from l3embedding_amd import _lib, classifier, svm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SETS = [('c4', 'linear'), ('c4', 'poly'), ('c4', 'rbf'), ('c4', 'sigmoid'), ('c2', 'rbf'), ('c2', 'linear'), ('c12', 'rbf')]


def _fixture(name):
    return np.load(os.path.join(GOLDEN, 'svm_%s.npz' % name))


def _libsvm_ovo(z, kind):
    """sklearn's recorded decision values in libsvm's sign (n, P): sklearn negates the binary one"""
    ovo = z[kind + '_ovo'].reshape(len(z['Xt']), -1)
    return -ovo if np.unique(z['y']).size == 2 else ovo


@pytest.mark.parametrize('name,kind', SETS)
def test_reference_solver_meets_sklearn(name, kind):
    z = _fixture(name)
    X, y, Xt = z['X'], z['y'], z['Xt']
    gamma = 1.0 / X.shape[1]
    co, C, tol = float(z[kind + '_coef0']), float(z[kind + '_C']), float(z[kind + '_tol'])
    classes, support, n_support, coef, rho = ref.ovo_fit(X, y, kind, gamma, C, tol, coef0=co)
    dec = ref.ovo_decision(Xt, X[support], n_support, coef, rho, kind, gamma, coef0=co)
    calib = float(z[kind + '_calib'])
    assert calib > 0
    assert np.max(np.abs(dec - _libsvm_ovo(z, kind))) <= 2 * calib


@pytest.mark.parametrize('name,kind', SETS)
def test_coupling_reproduces_sklearn_predict_proba(name, kind):
    z = _fixture(name)
    nc = np.unique(z['y']).size
    dec = _libsvm_ovo(z, kind)
    got = svm.pairwise_coupling(dec, z[kind + '_probA'], z[kind + '_probB'], nc)
    np.testing.assert_allclose(got, z[kind + '_proba'], rtol=0, atol=1e-10)
    np.testing.assert_allclose(ref.predict_proba(dec, z[kind + '_probA'], z[kind + '_probB'], nc), z[kind + '_proba'], rtol=0,
                               atol=1e-10)


@pytest.mark.parametrize('name', ['c4', 'c12'])
def test_ovr_transform_reproduces_sklearn(name):
    z = _fixture(name)
    nc = np.unique(z['y']).size
    ovo = z['rbf_ovo']
    np.testing.assert_allclose(svm.ovr_decision_function(ovo < 0, -ovo, nc), z['rbf_ovr'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.ovr_decision_function(ovo < 0, -ovo, nc), z['rbf_ovr'], rtol=0, atol=1e-12)


def test_sigmoid_train_matches_the_loop_restatement():
    r = np.random.RandomState(4)
    dec = r.randn(200) * 2
    labels = np.where(dec + r.randn(200) > 0, 1, -1)
    A, B = svm.sigmoid_train(dec, labels)
    rA, rB = ref.sigmoid_train(list(dec), list(labels))
    assert abs(A - rA) < 1e-9 and abs(B - rB) < 1e-9
    np.testing.assert_allclose(svm.sigmoid_predict(dec, A, B), [ref.sigmoid_predict(d, rA, rB) for d in dec], rtol=0, atol=1e-12)


def test_hinge_loss_multiclass_and_binary():
    r = np.random.RandomState(5)
    y = r.randint(0, 4, 50)
    dec = r.randn(50, 4)
    assert abs(svm.hinge_loss(y, dec, labels=np.arange(4)) - ref.hinge_loss(y, dec, np.arange(4))) < 1e-12
    yb = r.randint(3, 5, 40)
    db = r.randn(40)
    assert abs(svm.hinge_loss(yb, db) - ref.hinge_loss(yb, db, [3, 4])) < 1e-12
    # labels beyond the classes present widen the decision matrix as sklearn's do
    assert svm.hinge_loss([0, 1, 2], np.eye(3) * 3, labels=[0, 1, 2]) == 0.0


class FakeSVM(object):
    """Stands in for _lib.SVM: every problem's alpha is 0.5 on its first row of each sign, rho 0; decision values come from a
    nearest-centroid rule so that the shell's bookkeeping is what is tested"""
    instances = []

    def __init__(self, device=0):
        FakeSVM.instances.append(self)
        self.X = None

    def set_data(self, X):
        self.X = np.asarray(X, np.float32)

    def fit(self, kernel, problems, cost=1.0, tol=1e-3, max_iter=-1, q=0):
        alphas = []
        for rows, s in problems:
            a = np.zeros(rows.size)
            a[np.flatnonzero(s > 0)[0]] = 0.5
            a[np.flatnonzero(s < 0)[0]] = 0.5
            alphas.append(a)
        P = len(problems)
        return alphas, np.zeros(P), np.ones(P, np.int64), np.ones(P, np.int32), np.zeros(P)

    def decision(self, kernel, sv_start, coef, rho, X=None, x_idx=None, SV=None, sv_idx=None):
        X = self.X[x_idx] if X is None else np.asarray(X)
        SV = self.X[sv_idx] if SV is None else np.asarray(SV)
        ncls = len(sv_start) - 1
        cent = [SV[sv_start[c]:sv_start[c + 1]].mean(axis=0) for c in range(ncls)]
        dist = np.stack([((X - c) ** 2).sum(1) for c in cent], axis=1)
        return np.stack([dist[:, j] - dist[:, i] for i in range(ncls) for j in range(i + 1, ncls)], axis=1)

    def close(self):
        pass


def test_train_svm_metrics_and_file_shell(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, 'SVM', FakeSVM)
    r = np.random.RandomState(2)
    cent = np.eye(3, 4) * 5
    y = np.repeat(np.arange(3), 20)
    X = (cent[y] + r.randn(60, 4) * 0.1).astype(np.float32)
    yt = np.repeat(np.arange(3), 6)
    Xt = (cent[yt] + r.randn(18, 4) * 0.1).astype(np.float32)
    train = {'features': X, 'labels': y}
    test = {'features': Xt, 'labels': np.array([0, 1, 2]), 'file_idxs': [(0, 6), (6, 12), (12, 18)]}
    model, tr, va, te = classifier.train_svm(train, train, test, str(tmp_path), C=2.0, num_classes=3)
    assert tr['accuracy'] == 1.0 and va['accuracy'] == 1.0 and te['accuracy'] == 1.0
    assert tr['loss'] == pytest.approx(svm.hinge_loss(y, model.decision_function(X), labels=np.arange(3)))
    assert model.C == 2.0 and model.probability and model.random_state == 12345678
    assert list(model.n_support_) == [1, 1, 1] and model.dual_coef_.shape == (2, 3)
    with open(os.path.join(str(tmp_path), 'model.pkl'), 'rb') as fh:
        again = pickle.load(fh)
    assert again._h is None and np.array_equal(again.support_, model.support_)
    np.testing.assert_allclose(model.predict_proba(Xt).sum(axis=1), 1.0, atol=1e-12)


def test_train_param_search_accepts_train_svm(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, 'SVM', FakeSVM)
    r = np.random.RandomState(3)
    y = np.repeat(np.arange(2), 10)
    X = (np.eye(2, 3)[y] * 4 + r.randn(20, 3) * 0.1).astype(np.float32)
    data = {'features': X, 'labels': y}
    test = {'features': X[:4], 'labels': np.array([0]), 'file_idxs': [(0, 4)]}
    _, tr, va, _ = classifier.train_param_search(data, data, test, str(tmp_path), train_func=classifier.train_svm,
                                                 search_space={'C': [0.1, 1, 10, 100, 1000]}, num_classes=2)
    assert tr['search_params'] == ['C'] and set(va['search']) == {(c,) for c in (0.1, 1, 10, 100, 1000)}


def test_binary_model_uses_sklearn_sign(monkeypatch):
    monkeypatch.setattr(_lib, 'SVM', FakeSVM)
    X = np.array([[0.0, 0], [0.1, 0], [5, 0], [5.1, 0]], np.float32)
    m = svm.SVC(gamma='auto').fit(X, np.array([7, 7, 9, 9]))
    d = m.decision_function(np.array([[5.0, 0], [0.0, 0]], np.float32))
    assert d.shape == (2,) and d[0] > 0 > d[1]             # positive means classes_[1]
    assert list(m.predict(np.array([[5.0, 0]], np.float32))) == [9]
    assert m.intercept_.shape == (1,) and np.array_equal(m.dual_coef_, -m._dual_coef_)
