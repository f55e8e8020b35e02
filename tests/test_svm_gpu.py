"""The SVM classifier on the GPU (classifier/train.py:79-166, csrc/svm.hip): the kernel-row launch and one local SMO solve against
the float64 restatement in tests/svm_ref.py, SVC.fit against the scikit-learn fixtures of tests/golden/svm_*.npz, an optimality
certificate at scale that does not depend on any solver's path, determinism, and train_svm end to end with the parameter search.
Nothing here needs sklearn: the fixtures hold its answers."""
import logging
import os
import pickle

import numpy as np
import pytest

import svm_ref as ref
from l3embedding_amd import _lib, classifier, svm
from l3embedding_amd.svm import SVC

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LOG = logging.getLogger(__name__)


def _fixture(name):
    return np.load(os.path.join(GOLDEN, 'svm_%s.npz' % name))


def _params(z, kind):
    return dict(kernel=kind, C=float(z[kind + '_C']), tol=float(z[kind + '_tol']), coef0=float(z[kind + '_coef0']),
                degree=int(z[kind + '_degree']))


def _dk_ddot(kind, K, dot, gamma, coef0, degree):
    """|dK / d(u.v)| in float64: how far a rounding of the dot product moves the kernel value"""
    if kind == 'linear':
        return np.ones_like(K)
    if kind == 'poly':
        return np.abs(degree * gamma * (gamma * dot + coef0) ** (degree - 1))
    if kind == 'rbf':
        return 2 * gamma * K
    return gamma * (1 - K * K)


# bound: |K_gpu - K| <= 2.5e-7 sqrt(D) |dK/d dot| S + 1e-6 |K| + 1e-7, S = sum |u_k v_k| (rbf: + |u|^2 + |v|^2, the norms it
# subtracts): one serial fp32 MFMA chain of D / 2 steps per dot product (a random walk of roundings, ~4 u sqrt(D) S), then one
# fp32 kernel-function evaluation.  Measured on MI355X: at most 0.25 of the bound (linear, D = 6144: 4e-6 S)
@pytest.mark.parametrize('kind', ref.KINDS)
@pytest.mark.parametrize('D', [64, 512, 6144])
def test_kernel_rows_match_float64(gpu_required, kind, D):
    r = np.random.RandomState(D + len(kind))
    n_x = 300
    x = (r.randn(n_x, D) / np.sqrt(D) * 3).astype(np.float32)
    a_idx = r.randint(0, n_x, 130).astype(np.int32)         # more than one group of 128 rows, ragged
    b_idx = r.randint(0, n_x, 77).astype(np.int32)
    gamma, coef0, degree = 1.0 / D * 4, 0.5, 3
    got = _lib.op_svm_kernel_rows(x, a_idx, b_idx, kind, gamma=gamma, coef0=coef0, degree=degree)
    A, B = x[a_idx].astype(np.float64), x[b_idx].astype(np.float64)
    exact = ref.kernel_matrix(A, B, kind, gamma, coef0, degree)
    S = np.abs(A) @ np.abs(B).T
    if kind == 'rbf':
        S = S + (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :]
    bound = 2.5e-7 * np.sqrt(D) * _dk_ddot(kind, exact, A @ B.T, gamma, coef0, degree) * S + 1e-6 * np.abs(exact) + 1e-7
    err = np.abs(got - exact)
    LOG.info('%s D=%d: max err %.3g, max err / bound %.3g', kind, D, err.max(), (err / bound).max())
    assert np.all(err <= bound), float((err / bound).max())


def test_local_smo_matches_reference_solver(gpu_required):
    z = _fixture('c4')
    X, y = z['X'], z['y']
    rows = np.concatenate((np.flatnonzero(y == 0)[:50], np.flatnonzero(y == 1)[:46]))
    s = np.where(y[rows] == 0, 1, -1).astype(np.int8)
    K = _lib.op_svm_kernel_rows(X, rows, rows, 'rbf', gamma=1.0 / 64)
    for C, eps in ((1.0, 1e-3), (0.3, 1e-5)):
        a, upd = _lib.op_svm_smo(K, s, np.zeros(s.size), -np.ones(s.size), cost=C, eps=eps)
        ra, _, rupd = ref.solve(K.astype(np.float64), s, C, eps)
        assert upd == rupd
        np.testing.assert_allclose(a, ra, rtol=0, atol=1e-9 * C)
        gap, lo, hi, eq = ref.optimality(K.astype(np.float64), s, a, C)
        assert gap < eps and lo >= 0 and hi <= 0 and eq <= 1e-9 * C * s.size


@pytest.mark.parametrize('name,kind', [('c4', 'linear'), ('c4', 'poly'), ('c4', 'rbf'), ('c4', 'sigmoid'), ('c2', 'rbf'),
                                       ('c2', 'linear'), ('c12', 'rbf')])
def test_svc_matches_sklearn_fixture(gpu_required, name, kind):
    z = _fixture(name)
    X, y, Xt = z['X'], z['y'], z['Xt']
    p = _params(z, kind)
    m = SVC(probability=True, gamma='auto', random_state=0, **p).fit(X, y)
    calib = float(z[kind + '_calib'])
    ovo_sk = z[kind + '_ovo']
    nc = np.unique(y).size
    ovo = m.decision_function(Xt) if nc == 2 else None
    if nc > 2:
        m.decision_function_shape = 'ovo'
        ovo = m.decision_function(Xt)
        m.decision_function_shape = 'ovr'
        ovr = m.decision_function(Xt)
        # a pairwise vote may flip where sklearn's own value lies within the calibration distance of 0
        steady = np.min(np.abs(ovo_sk), axis=1) >= calib
        assert np.max(np.abs(ovr - z[kind + '_ovr'])[steady]) <= 2 * calib
    dist = float(np.max(np.abs(ovo - ovo_sk)))
    LOG.info('%s %s: decision distance %.3g (calibration %.3g)', name, kind, dist, calib)
    assert dist <= 2 * calib, (dist, calib)
    np.testing.assert_allclose(m.intercept_, z[kind + '_intercept'], rtol=0, atol=2 * calib)
    pred, pred_sk = m.predict(Xt), z[kind + '_predict']
    sk_margin = np.min(np.abs(ovo_sk.reshape(len(Xt), -1)), axis=1)
    differ = pred != pred_sk
    assert np.all(sk_margin[differ] < calib), (differ.sum(), sk_margin[differ])
    # the coupling of these decision values with sklearn's own Platt parameters: only the decision values differ
    dec = ovo.reshape(len(Xt), -1) * (-1 if nc == 2 else 1)
    coupled = svm.pairwise_coupling(dec, z[kind + '_probA'], z[kind + '_probB'], nc)
    cdist = float(np.max(np.abs(coupled - z[kind + '_proba'])))
    assert cdist <= 1e-2, cdist
    # end to end the cross-validation folds differ too (np.random.RandomState, not libsvm's rand()): other folds move sklearn's
    # own probabilities by up to proba_spread on the same set (0.010 - 0.052 on these fixtures)
    proba = m.predict_proba(Xt)
    pdist = float(np.max(np.abs(proba - z[kind + '_proba'])))
    spread = float(z[kind + '_proba_spread'])
    LOG.info('%s %s: predict_proba distance %.3g (sklearn decision values coupled: %.3g; sklearn fold spread %.3g)', name, kind,
             pdist, cdist, spread)
    assert pdist <= 2 * spread, (pdist, spread)
    assert m.dual_coef_.shape == z[kind + '_dual_coef'].shape[:1] + m.support_.shape
    assert m.probA_.shape == z[kind + '_probA'].shape


def _clusters(n, D, C, seed):
    r = np.random.RandomState(seed)
    centres = r.randn(C, D) * 0.25
    y = np.arange(n) % C
    r.shuffle(y)
    X = (centres[y] + r.randn(n, D) / np.sqrt(D) * 2.5).astype(np.float32)
    return X, y.astype(np.int32)


@pytest.mark.parametrize('tol', [1e-3, 1e-5])
def test_optimality_certificate_at_scale(gpu_required, tol):
    """n = 8000, D = 512, 10 classes: every one-vs-one problem's returned alpha is optimal to tol on the fp32 kernel matrix the
    GPU computes (the gradient recomputed in float64 from alpha), whatever path the solver took"""
    X, y = _clusters(8000, 512, 10, 1)
    gamma, C = 1.0 / 512, 1.0
    h = _lib.SVM()
    h.set_data(X)
    groups = [np.flatnonzero(y == c).astype(np.int32) for c in range(10)]
    problems = []
    for i in range(10):
        for j in range(i + 1, 10):
            problems.append((np.concatenate((groups[i], groups[j])),
                             np.concatenate((np.ones(groups[i].size), -np.ones(groups[j].size))).astype(np.int8)))
    alphas, rho, upd, outer, gaps = h.fit(_lib.svm_kernel('rbf', gamma), problems, cost=C, tol=tol)
    worst, worst64 = 0.0, 0.0
    for (rows, s), a in zip(problems, alphas):
        K = _lib.op_svm_kernel_rows(X, rows, rows, 'rbf', gamma=gamma).astype(np.float64)
        gap, lo, hi, eq = ref.optimality(K, s, a, C)
        assert gap <= tol and lo >= 0 and hi <= 0 and eq <= 1e-9 * max(C * a.sum(), 1e-300), (gap, lo, hi, eq)
        worst = max(worst, gap)
        K64 = ref.kernel_matrix(X[rows], X[rows], 'rbf', gamma)
        worst64 = max(worst64, ref.optimality(K64, s, a, C)[0])
    LOG.info('tol %g: worst gap %.3g on the fp32 kernel, %.3g on the exact one; outer iterations %d..%d, updates %d..%d', tol,
             worst, worst64, outer.min(), outer.max(), upd.min(), upd.max())
    print('certificate tol %g: worst gap fp32 kernel %.3g, float64 kernel %.3g, outer %d..%d, updates %d..%d' % (
        tol, worst, worst64, outer.min(), outer.max(), upd.min(), upd.max()))


def test_fit_is_deterministic(gpu_required):
    z = _fixture('c12')
    X, y, Xt = z['X'], z['y'], z['Xt']
    runs = []
    for _ in range(2):
        m = SVC(probability=True, gamma='auto', random_state=3).fit(X, y)
        runs.append((m.dual_coef_, m.intercept_, m.probA_, m.probB_, m.decision_function(Xt), m.predict_proba(Xt)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_set_data_again_on_one_handle_equals_a_fresh_handle(gpu_required):
    """set_data frees the resident matrix and its norms and allocates new ones: a larger set, then a smaller one, on the same
    handle; the solver and the decision values over the resident rows are those of a fresh handle, bit for bit.  D = 20 is no
    multiple of 4 (the scalar loads of the kernel rows)."""
    kern = _lib.svm_kernel('rbf', 1.0 / 20)
    kept = _lib.SVM()
    for n, seed in ((64, 5), (300, 6), (40, 7)):
        X, y = _clusters(n, 20, 3, seed)
        groups = [np.flatnonzero(y == c).astype(np.int32) for c in range(3)]
        problems = [(np.concatenate((groups[i], groups[j])),
                     np.concatenate((np.ones(groups[i].size), -np.ones(groups[j].size))).astype(np.int8))
                    for i in range(3) for j in range(i + 1, 3)]
        sv_idx = np.concatenate(groups)
        sv_start = np.concatenate([[0], np.cumsum([g.size for g in groups])])
        r = np.random.RandomState(seed)
        coef, rho = r.randn(2, n), r.randn(3)
        out = []
        for h in (kept, _lib.SVM()):
            h.set_data(X)
            assert (h.n, h.D) == (n, 20)
            alphas, rho_fit = h.fit(kern, problems)[:2]
            out.append((np.concatenate(alphas), rho_fit,
                        h.decision(kern, sv_start, coef, rho, x_idx=np.arange(n, dtype=np.int32), sv_idx=sv_idx),
                        h.decision(kern, sv_start, coef, rho, X=X[::-1], sv_idx=sv_idx)))
            if h is not kept:
                h.close()
        for a, b in zip(*out):
            assert a.size and np.isfinite(a).all() and np.array_equal(a, b), n
    kept.close()


def test_pickles_without_handle_and_predicts_again(gpu_required, tmp_path):
    z = _fixture('c4')
    m = SVC(probability=True, gamma='auto', random_state=1).fit(z['X'], z['y'])
    d = m.decision_function(z['Xt'])
    blob = pickle.dumps(m)
    m2 = pickle.loads(blob)
    assert m2._h is None
    assert np.array_equal(m2.decision_function(z['Xt']), d)
    assert np.array_equal(m2.predict(z['Xt']), m.predict(z['Xt']))


def test_max_iter_caps_updates_and_warns(gpu_required, caplog):
    z = _fixture('c4')
    with caplog.at_level(logging.WARNING, logger='classifier'):
        m = SVC(max_iter=5, gamma='auto').fit(z['X'], z['y'])
    assert np.all(m.n_iter_ <= 5)
    assert any('max_iter=5' in rec.getMessage() for rec in caplog.records)


def _write_fold_dir(root, D=32, C=3, files=4, frames=6, seed=0):
    """features/us8k/l3/synthetic/fold1..fold10/*.npz as usc_generate writes them (X frames, y the class)"""
    r = np.random.RandomState(seed)
    centres = r.randn(C, D) * 1.2
    fdir = os.path.join(root, 'features', 'us8k', 'l3', 'synthetic')
    for f in range(10):
        d = os.path.join(fdir, 'fold%d' % (f + 1))
        os.makedirs(d)
        for c in range(C):
            for k in range(files):
                np.savez(os.path.join(d, '%d-%d-%d.npz' % (f, c, k)), X=(centres[c] + r.randn(frames, D)).astype(np.float32),
                         y=np.array(c))
    return fdir


def test_train_svm_and_parameter_search_end_to_end(gpu_required, tmp_path):
    from l3embedding_amd.usc import get_split, preprocess_split_data
    fdir = _write_fold_dir(str(tmp_path))
    splits = get_split(fdir, 2, 'us8k', valid=True)
    preprocess_split_data(*splits, feature_mode='framewise', non_overlap=False, non_overlap_chunk_size=10, use_min_max=False)
    mdir = str(tmp_path / 'model')
    os.makedirs(mdir)
    model, train_m, valid_m, test_m = classifier.train_svm(*splits, mdir, C=1.0, num_classes=10)
    assert os.path.exists(os.path.join(mdir, 'model.pkl'))
    with open(os.path.join(mdir, 'model.pkl'), 'rb') as fh:
        again = pickle.load(fh)
    assert np.array_equal(again.predict(splits[0]['features']), model.predict(splits[0]['features']))
    assert train_m['accuracy'] > 0.9 and valid_m['accuracy'] > 0.5 and 0 <= train_m['loss'] < 1
    assert len(test_m['class_accuracy']) == 10 and test_m['accuracy'] > 0.5
    model, train_m, valid_m, test_m = classifier.train_param_search(*splits, mdir, train_func=classifier.train_svm,
                                                                    search_space={'C': [0.1, 1, 10]}, num_classes=10,
                                                                    train_with_valid=True)
    assert train_m['search_params'] == ['C'] and train_m['search_params_best_values'][0] in (0.1, 1, 10)
    assert set(valid_m['search']) == {(0.1,), (1,), (10,)}
    assert test_m['accuracy'] > 0.5
