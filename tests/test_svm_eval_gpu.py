"""Scoring an SVM on the GPU (csrc/svm_eval.hip; l3_op_svm_tail, l3_svm_score, SVC.evaluate, train_svm(evaluate_on_device=True)):
the vote, sklearn's ovr decision values, the hinge loss, Platt's pair probabilities, libsvm's pairwise coupling and the per-file
means against tests/svm_ref.py and svm.py's own NumPy functions, bit for bit where the arithmetic is the same operations
(everything but the one exp of a pair probability)."""
import logging
import os
import pickle

import numpy as np
import pytest

import svm_ref as ref
from l3embedding_amd import _lib, classifier, svm
from l3embedding_amd.svm import SVC
from l3embedding_amd.usc import DeviceFeatures

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LOG = logging.getLogger(__name__)
U = 2.0 ** -53
CLASSES = [2, 3, 10, 50, 64]
ROWS = [1, 31, 33, 70]
# one-row files, ragged files of 1 ... 40 rows, ranges that leave rows out
FILES = {1: [(0, 1)], 31: [(0, 31)], 33: [(0, 1), (5, 33)], 70: [(0, 1), (1, 2), (2, 42), (42, 45), (50, 69), (69, 70)]}
_CASES = {}


def _bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _inputs(C, n):
    """dec ~ N(0, s^2), s cycling through 0.3, 1.5, 5; from three rows on, row 1 is all zeros and row 2 is +-1e3 (probabilities at
    both clips); Platt's A in [-3, -0.5], B ~ 0.3 N(0, 1); labels that take every class they can"""
    r = np.random.RandomState(1000 * C + n)
    P = C * (C - 1) // 2
    dec = r.randn(n, P) * np.array([0.3, 1.5, 5.0])[np.arange(n) % 3][:, None]
    if n >= 3:
        dec[1] = 0.0
        dec[2] = np.where(np.arange(P) % 2 == 0, 1e3, -1e3)          # alternating, so that two pairs already show both clips
    A, B = r.uniform(-3, -0.5, P), 0.3 * r.randn(P)
    y = ((np.arange(n) * 7) % C).astype(np.int32)
    return dec, A, B, y


def _case(C, n):
    """one l3_op_svm_tail call per shape, shared by the tests below and left unchanged"""
    if (C, n) not in _CASES:
        dec, A, B, y = _inputs(C, n)
        out = _lib.op_svm_tail(dec, C, A, B, labels=y, files=FILES[n])
        _CASES[(C, n)] = (dec, A, B, y, out)
    return _CASES[(C, n)]


def _coupling_margin(r):
    """an instrumented copy of svm_ref.multiclass_probability's loop -> the smallest | max_t |Qp[t] - pQp| - eps | over the
    stopping tests the row went through (how far the row is from taking one sweep more or fewer)"""
    k = r.shape[0]
    sq = r * r
    Q = -(r.T * r)
    Q[np.arange(k), np.arange(k)] = sq.sum(axis=0) - np.diag(sq)
    p = np.full(k, 1.0 / k)
    eps, margin = 0.005 / k, np.inf
    for _ in range(max(100, k)):
        Qp = Q @ p
        pQp = p @ Qp
        err = np.abs(Qp - pQp).max()
        margin = min(margin, abs(err - eps))
        if err < eps:
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            Qp = (Qp + diff * Q[t]) / (1 + diff)
            p /= (1 + diff)
    return margin


def _r_matrix(pp, C):
    r = np.zeros((C, C))
    k = 0
    for i in range(C):
        for j in range(i + 1, C):
            r[i, j], r[j, i] = pp[k], 1 - pp[k]
            k += 1
    return r


@pytest.mark.parametrize('C', CLASSES)
def test_vote_and_ovr_values(gpu_required, C):
    for n in ROWS:
        dec, _, _, _, out = _case(C, n)
        assert np.array_equal(out['pred'], ref.ovo_vote(dec, C)), n
        want = -dec.ravel() if C == 2 else svm.ovr_decision_function(dec < 0, -dec, C)
        assert _bits(out['ovr'], want), n


def test_vote_special_rows(gpu_required):
    """all decisions exactly 0: every pair votes for its higher class, so the last class wins the vote, while sklearn's ovr votes
    (dec < 0) all go to the lower class; a three-way tie goes to the lowest class"""
    for C in CLASSES:
        dec, _, _, _, out = _case(C, 33)
        assert not dec[1].any() and out['pred'][1] == C - 1
        if C > 2:
            assert out['ovr'][1].argmax() == 0
    cyc = np.array([[1.0, -1.0, 1.0], [-2.0, 3.0, -0.5]])          # (0,1) (0,2) (1,2): one vote each
    out = _lib.op_svm_tail(cyc, 3, outputs=('pred',))
    assert out['pred'].tolist() == [0, 0]


@pytest.mark.parametrize('C', CLASSES)
def test_hinge_terms_and_mean(gpu_required, C):
    """terms: bits (one-row calls); mean: within n u sum|term| / n of svm.hinge_loss, the distance of two float64 sums of n terms"""
    for n in ROWS:
        dec, _, _, y, out = _case(C, n)
        terms = np.empty(n)
        for i in range(n):
            got = _lib.op_svm_tail(dec[i:i + 1], C, labels=y[i:i + 1], outputs=('hinge_sum',))['hinge_sum']
            if C == 2:
                want = max(0.0, 1.0 - (1.0 if y[i] == 1 else -1.0) * out['ovr'][i])
            else:
                want = ref.hinge_loss(y[i:i + 1], out['ovr'][i:i + 1], np.arange(C))
            assert _bits(got, want), (n, i, got, want)
            terms[i] = got
        if n == 1:
            continue              # sklearn's hinge_loss reads the class count off y_true: one row has no multiclass form
        mean = svm.hinge_loss(y, out['ovr'], labels=np.arange(C))
        dist = abs(out['hinge_sum'] / n - mean)
        LOG.info('C=%d n=%d: hinge mean distance %.3g (bound %.3g)', C, n, dist, U * np.abs(terms).sum())
        assert dist <= n * U * np.abs(terms).sum() / n, (n, dist)


@pytest.mark.parametrize('C', CLASSES)
def test_pair_probabilities(gpu_required, C):
    """f = dec * A + B is two roundings on both sides; then one exp (1 ulp on the device as the ROCm math library documents it, not
    verified on this chip; glibc's own last place on the host), an add and a divide within u each: 4 u, asserted with a factor of
    two.  Measured on MI355X on these inputs: 2.2 - 3.0 u (profiles/r16_svm_eval.txt)."""
    worst = 0.0
    for n in ROWS:
        dec, A, B, _, out = _case(C, n)
        want = np.clip(svm.sigmoid_predict(dec, A, B), svm.MIN_PROB, 1 - svm.MIN_PROB)
        got = out['pair_proba']
        assert got.min() >= svm.MIN_PROB and got.max() <= 1 - svm.MIN_PROB
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
        if n >= 3:                # +-1e3: both clips, exactly
            clips = set(np.unique(got[2]))
            assert clips <= {svm.MIN_PROB, 1 - svm.MIN_PROB} and (C == 2 or len(clips) == 2)
    LOG.info('C=%d: pair probability relative distance %.3g u', C, worst / U)
    print('pair probability relative distance, C=%d: %.3f u' % (C, worst / U))
    assert worst <= 8 * U, worst / U


@pytest.mark.parametrize('C', CLASSES)
def test_coupling_bits_and_iterations(gpu_required, C):
    """the GPU's own pair probabilities through svm_ref.multiclass_probability, row by row: equal bits, equal sweep counts.
    No row that needs the iteration cap is among them: a search on the CPU with the scalar loop (random rows at every scale above,
    transitive, cyclic and one-against-all tournaments up to +-1e3, 3 to 16 classes) found no row past 4 sweeps, so that case is
    dropped; the cap itself is max(100, k) in the kernel as in the loop.  Sweep counts: every row against the scalar loop itself."""
    hist = {}
    for n in ROWS:
        _, _, _, _, out = _case(C, n)
        for i in range(n):
            r = _r_matrix(out['pair_proba'][i], C)
            assert _bits(out['proba'][i], ref.multiclass_probability(r)), (n, i)
            assert out['iters'][i] == _sweeps(r), (n, i)
            hist[int(out['iters'][i])] = hist.get(int(out['iters'][i]), 0) + 1
    print('coupling sweeps histogram, C=%d: %s' % (C, sorted(hist.items())))


def _sweeps(r):
    """svm_ref.multiclass_probability's loop on Python floats (the same float64 operations in the same order), counting its
    update sweeps"""
    k = r.shape[0]
    r = r.tolist()
    Q = [[0.0] * k for _ in range(k)]
    p = [1.0 / k] * k
    for t in range(k):
        for j in range(t):
            Q[t][t] += r[j][t] * r[j][t]
            Q[t][j] = Q[j][t]
        for j in range(t + 1, k):
            Q[t][t] += r[j][t] * r[j][t]
            Q[t][j] = -r[j][t] * r[t][j]
    eps = 0.005 / k
    for it in range(max(100, k)):
        Qp = [0.0] * k
        pQp = 0.0
        for t in range(k):
            Qt, s = Q[t], 0.0
            for j in range(k):
                s += Qt[j] * p[j]
            Qp[t] = s
            pQp += p[t] * s
        if max(abs(Qp[t] - pQp) for t in range(k)) < eps:
            return it
        for t in range(k):
            Qt = Q[t]
            diff = (-Qp[t] + pQp) / Qt[t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Qt[t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Qt[j]) / (1 + diff)
                p[j] /= (1 + diff)
    return max(100, k)


def _proba_close(proba, dec, A, B, C):
    """end to end against svm.pairwise_coupling within 1e-12, rows with a borderline stopping test (within 1e-10) left out, at
    most 1 % of them"""
    want = svm.pairwise_coupling(dec, A, B, C)
    pp = np.clip(svm.sigmoid_predict(dec, A, B), svm.MIN_PROB, 1 - svm.MIN_PROB)
    steady = np.array([_coupling_margin(_r_matrix(pp[i], C)) >= 1e-10 for i in range(dec.shape[0])])
    assert (~steady).sum() <= 0.01 * steady.size, (~steady).sum()
    dist = float(np.max(np.abs(proba - want)[steady])) if steady.any() else 0.0
    assert dist <= 1e-12, dist
    return dist


@pytest.mark.parametrize('C', CLASSES)
def test_probabilities_end_to_end(gpu_required, C):
    for n in ROWS:
        dec, A, B, _, out = _case(C, n)
        _proba_close(out['proba'], dec, A, B, C)
        np.testing.assert_allclose(out['proba'].sum(axis=1), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize('C', CLASSES)
def test_file_means_and_classes(gpu_required, C):
    for n in ROWS:
        _, _, _, _, out = _case(C, n)
        proba = out['proba']
        for f, (s, e) in enumerate(FILES[n]):
            total = np.zeros(C)
            for row in range(s, e):
                total = total + proba[row]
            assert _bits(out['file_proba'][f], total / (e - s)), (n, f)
        want = classifier._file_predictions(proba, FILES[n])
        top = np.sort(out['file_proba'], axis=1)
        clear = top[:, -1] - top[:, -2] > 1e-12
        assert np.array_equal(out['file_pred'][clear], want[clear]), n
    tie = _lib.op_svm_tail(np.zeros((2, 1)), 2, [-1.0], [0.0], files=[(0, 2)], outputs=('file_proba', 'file_pred'))
    assert tie['file_proba'].tolist() == [[0.5, 0.5]] and tie['file_pred'].tolist() == [0]      # the lower class on a tie


def test_tail_is_deterministic_and_checks_its_arguments(gpu_required):
    dec, A, B, y, out = _case(10, 70)
    again = _lib.op_svm_tail(dec, 10, A, B, labels=y, files=FILES[70])
    for k in out:
        assert np.array_equal(np.asarray(out[k]), np.asarray(again[k])), k
    with pytest.raises(_lib.L3Error):
        _lib.op_svm_tail(dec, 10, labels=y + 10, outputs=('hinge_sum',))
    with pytest.raises(_lib.L3Error):
        _lib.op_svm_tail(dec, 10, A, B, files=[(3, 3)], outputs=('file_pred',))
    with pytest.raises(_lib.L3Error):
        _lib.op_svm_tail(dec, 10, A, B, files=[(0, 71)], outputs=('file_pred',))
    with pytest.raises(_lib.L3Error):
        _lib.op_svm_tail(dec, 10, outputs=('proba',))


def test_score_two_row_blocks_equals_decision_then_tail(gpu_required):
    """C = 64, D = 8, two support vectors per class, n = 8400: the decision launch works in blocks of 8320 rows there, so the pass
    runs two blocks, a file spans their boundary and the hinge chunks of 256 rows do not line up with it"""
    C, D, n = 64, 8, 8400
    P = C * (C - 1) // 2
    r = np.random.RandomState(5)
    SV = r.randn(2 * C, D).astype(np.float32)
    cs = np.arange(C + 1, dtype=np.int64) * 2
    coef, rho = r.randn(C - 1, 2 * C), 0.1 * r.randn(P)
    A, B = r.uniform(-3, -0.5, P), 0.3 * r.randn(P)
    X = r.randn(n, D).astype(np.float32)
    y = r.randint(0, C, n).astype(np.int32)
    files = [(0, 40), (8300, 8400), (8399, 8400)]
    kp = _lib.svm_kernel('rbf', 1.0 / D)
    h = _lib.SVM()
    pred = np.empty(n, np.int32)
    assert h.lib.l3_svm_score(h.h, _lib._ptr(X), None, None, 0, 0, n, D, None, None, 0, _lib._ptr(pred), None, None, None, None,
                              None) == -4                    # L3_ESTATE: no model yet
    h.set_model(kp, cs, coef, rho, SV=SV, probA=A, probB=B)
    got = h.score(X=X, labels=y, files=files)
    dec = h.decision(kp, cs, coef, rho, X=X, SV=SV)
    want = _lib.op_svm_tail(dec, C, A, B, labels=y, files=files)
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    # the same rows as a resident matrix through indices, and from a device matrix
    h.set_data(X)
    feat = _lib.Features(X)
    for kw in (dict(x_idx=np.arange(n, dtype=np.int32)), dict(feat=feat)):
        other = h.score(labels=y, files=files, outputs=('pred', 'hinge_sum', 'file_proba'), **kw)
        for k in other:
            assert np.array_equal(np.asarray(other[k]), np.asarray(got[k])), (sorted(kw), k)
    part = h.score(feat=feat, lo=100, hi=133, outputs=('ovr',))
    assert np.array_equal(part['ovr'], got['ovr'][100:133])
    with pytest.raises(_lib.L3Error):
        h.score(feat=feat, lo=10, hi=n + 1, outputs=('pred',))
    no_prob = _lib.SVM()
    no_prob.set_model(kp, cs, coef, rho, SV=SV)
    assert np.array_equal(no_prob.score(X=X[:50], outputs=('pred',))['pred'], got['pred'][:50])
    with pytest.raises(_lib.L3Error):
        no_prob.score(X=X[:50], outputs=('proba',))


def _fixture(name, drop=0):
    z = np.load(os.path.join(GOLDEN, 'svm_%s.npz' % name))
    D = z['X'].shape[1] - drop
    return z['X'][:, :D].copy(), z['y'], z['Xt'][:, :D].copy()


_MODELS = {}


def _model(name, drop):
    if (name, drop) not in _MODELS:
        X, y, Xt = _fixture(name, drop)
        _MODELS[(name, drop)] = (SVC(probability=True, gamma='auto', random_state=0).fit(X, y), X, y, Xt)
    return _MODELS[(name, drop)]


MODELS = [('c2', 0), ('c4', 0), ('c4', 1), ('c12', 0)]          # ('c4', 1): D = 63, not a multiple of 4
ALL = svm.EVALUATE_OUTPUTS


def _files_of(n):
    return np.array([(0, 1), (1, 30), (30, n - 5)], np.int64)


@pytest.mark.parametrize('name,drop', MODELS)
def test_evaluate_equals_the_host_methods(gpu_required, name, drop):
    m, X, y, Xt = _model(name, drop)
    C = m.classes_.size
    yt = m.classes_[np.arange(len(Xt)) % C]
    files = _files_of(len(Xt))
    got = m.evaluate(Xt, y=yt, file_idxs=files, outputs=ALL)
    assert np.array_equal(got['predict'], m.predict(Xt))
    ovr = m.decision_function(Xt)
    assert _bits(got['decision_function'], ovr)
    loss = svm.hinge_loss(yt, ovr, labels=m.classes_)
    terms_sum = loss * len(Xt)
    assert abs(got['hinge_loss'] - loss) <= len(Xt) * U * terms_sum / len(Xt) + 0.0
    dec = m._ovo(Xt)
    _proba_close(got['predict_proba'], dec, m.probA_, m.probB_, C)
    for f, (s, e) in enumerate(files):
        total = np.zeros(C)
        for row in range(s, e):
            total = total + got['predict_proba'][row]
        assert _bits(got['file_proba'][f], total / (e - s))
    top = np.sort(got['file_proba'], axis=1)
    clear = top[:, -1] - top[:, -2] > 1e-12
    want = m.classes_[classifier._file_predictions(got['predict_proba'], files)]
    assert np.array_equal(got['file_predict'][clear], want[clear])
    only = m.evaluate(Xt, outputs=('predict',))
    assert sorted(only) == ['predict'] and np.array_equal(only['predict'], got['predict'])


@pytest.mark.parametrize('name,drop', MODELS)
def test_device_features_fit_and_evaluate_equal_the_host(gpu_required, name, drop):
    m, X, y, Xt = _model(name, drop)
    on_dev = SVC(probability=True, gamma='auto', random_state=0).fit(DeviceFeatures(X), y)
    for attr in ('support_', 'support_vectors_', 'n_support_', 'dual_coef_', 'intercept_', 'probA_', 'probB_'):
        assert np.array_equal(getattr(on_dev, attr), getattr(m, attr)), attr
    C = m.classes_.size
    yt = m.classes_[np.arange(len(Xt)) % C]
    files = _files_of(len(Xt))
    feats = DeviceFeatures(Xt)
    host = m.evaluate(feats.to_host(), y=yt, file_idxs=files, outputs=ALL)
    for model in (m, on_dev):
        dev = model.evaluate(feats, y=yt, file_idxs=files, outputs=ALL)
        for k in ALL:
            assert np.array_equal(np.asarray(dev[k]), np.asarray(host[k])), k
    assert np.array_equal(on_dev.predict(feats), host['predict'])
    assert _bits(on_dev.decision_function(feats), host['decision_function'])
    assert _bits(on_dev.predict_proba(feats), host['predict_proba'])


def test_pickled_model_evaluates_to_the_same_bits(gpu_required):
    m, X, y, Xt = _model('c4', 1)
    files = _files_of(len(Xt))
    yt = m.classes_[np.arange(len(Xt)) % 4]
    before = m.evaluate(Xt, y=yt, file_idxs=files, outputs=ALL)
    again = pickle.loads(pickle.dumps(m))
    assert again._h is None and not again._model_set
    after = again.evaluate(Xt, y=yt, file_idxs=files, outputs=ALL)
    for k in ALL:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    calls = []
    real = again._h.set_model
    again._h.set_model = lambda *a, **kw: (calls.append(1), real(*a, **kw))
    again.evaluate(Xt, outputs=('predict',))
    assert not calls                                          # the model is set once, not per call


def _splits(seed=0, D=30, C=3, files=5, frames=6):
    r = np.random.RandomState(seed)
    centres = r.randn(C, D) * 1.2
    out = []
    for _ in range(3):
        feats, labels, idxs = [], [], []
        for c in range(C):
            for _k in range(files):
                idxs.append((len(feats) * frames, (len(feats) + 1) * frames))
                feats.append((centres[c] + r.randn(frames, D)).astype(np.float32))
                labels.append(c)
        out.append(dict(features=np.concatenate(feats), labels=np.array(labels), file_idxs=np.array(idxs, np.int64)))
    return out


def test_train_svm_on_device_equals_the_default_path(gpu_required, tmp_path):
    from l3embedding_amd.usc import preprocess_split_data
    results = []
    for on_device in (False, True):
        np.random.seed(3)
        splits = _splits()
        preprocess_split_data(*splits, feature_mode='framewise', non_overlap=False, non_overlap_chunk_size=10, use_min_max=False,
                              device=0)
        assert isinstance(splits[0]['features'], DeviceFeatures)
        mdir = str(tmp_path / ('model%d' % on_device))
        os.makedirs(mdir)
        results.append(classifier.train_svm(*splits, mdir, C=1.0, num_classes=3, evaluate_on_device=on_device))
        assert os.path.exists(os.path.join(mdir, 'model.pkl'))
        n_rows = [len(s['labels']) for s in splits[:2]]
    (_, tr0, va0, te0), (_, tr1, va1, te1) = results
    for a, b, n in ((tr0, tr1, n_rows[0]), (va0, va1, n_rows[1])):
        assert sorted(a) == sorted(b)
        assert a['accuracy'] == b['accuracy'] and a['class_accuracy'] == b['class_accuracy']
        assert abs(a['loss'] - b['loss']) <= n * U * (a['loss'] * n) / n + 0.0
    assert sorted(te0) == sorted(te1) and te0['accuracy'] == te1['accuracy']
