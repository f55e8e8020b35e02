"""The SVM's grid over C fitted in one pass (svm.fit_grid, classifier.train_svm_search / train_svm_fold) and the three entry points
under it, each against what the piecemeal path computes:

  1  l3_svm_fit_costs: one cost per problem, bit-equal to one l3_svm_fit call per cost
  2  l3_svm_cv_decision: the held-out decision values of many binary models in one launch, bit-equal to l3_svm_decision per model
  3  l3_op_svm_sigmoid_train: libsvm's sigmoid_train for many pairs at once, against the loop restatement tests/svm_ref.py within
     the restatement's own sensitivity to the order of its float64 sums
  4  fit_grid against SVC.fit per cost
  5  train_svm_search against train_param_search over train_svm; train_svm_fold's files

Measured on an MI355X (profiles/r17_svm_grid.txt): the yardstick m of part 3 is 8.42e-09 (host fits among themselves, noisy
l = 4097; the draw of the labels matters: with the constant jobs' labels drawn from another stream the same three host fits are
1.5e-07 apart at constant l = 65), the device's largest distance to the forward loop 8.42e-09 (noisy l = 4097, 7.48e-09 at constant
l = 4097), 9 of the 48 jobs further than 1e-12 from it (seven constant, noisy and wide 4097).  Part 4: the device's sigmoid fit
within 9.4e-15 of the host's on the grid's own cross-validation decisions."""
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
LOG = logging.getLogger(__name__)
CS = (0.1, 1, 10, 100, 1000)


def _say(msg):
    LOG.info(msg)
    print(msg)


# ---- 1. one cost per problem -----------------------------------------------------------------------------------------------------
COST_SIZES = (2, 37, 300)
COSTS = (0.1, 1, 1000)


def _cost_set(D):
    r = np.random.RandomState(D)
    n = sum(COST_SIZES)
    y = np.arange(n) % 2
    centres = r.randn(2, D) * 0.3
    X = (centres[y] + r.randn(n, D) / np.sqrt(D) * 2.5).astype(np.float32)
    problems, o = [], 0
    for s in COST_SIZES:
        rows = np.arange(o, o + s, dtype=np.int32)
        problems.append((rows, np.where(y[rows] == 0, 1, -1).astype(np.int8)))
        o += s
    return X, problems


@pytest.mark.parametrize('kind', ['rbf', 'linear'])
@pytest.mark.parametrize('D', [21, 32])
def test_costs_per_problem_equal_one_fit_per_cost(gpu_required, D, kind):
    X, problems = _cost_set(D)
    kp = _lib.svm_kernel(kind, 1.0 / D)
    h = _lib.SVM()
    h.set_data(X)
    costs = np.repeat(COSTS, len(problems))
    together = h.fit(kp, problems * len(COSTS), cost=costs)
    at = 0
    for c in COSTS:
        alone = h.fit(kp, problems, cost=c)
        for p in range(len(problems)):
            assert np.array_equal(together[0][at + p], alone[0][p]), (c, p)
            assert np.all(together[0][at + p] <= c) and np.all(together[0][at + p] >= 0)
        for k in range(1, 5):           # rho, updates, outer iterations, gaps
            assert np.array_equal(together[k][at:at + len(problems)], alone[k]), (c, k)
        at += len(problems)
    # the bounds are the problems' own: the smallest cost binds where the largest does not
    n = len(problems)
    assert any(not np.array_equal(together[0][p], together[0][-n + p]) for p in range(n))
    h.close()


@pytest.mark.parametrize('bad', [0.0, -1.0, np.nan, np.inf])
def test_costs_must_be_finite_and_positive(gpu_required, bad):
    X, problems = _cost_set(21)
    h = _lib.SVM()
    h.set_data(X)
    with pytest.raises(_lib.L3Error, match=r'error -1: .*need C > 0'):
        h.fit(_lib.svm_kernel('rbf', 0.05), problems, cost=[1.0, bad, 1.0])
    with pytest.raises(ValueError, match='one value per problem'):
        h.fit(_lib.svm_kernel('rbf', 0.05), problems, cost=[1.0, 1.0])
    h.close()


# ---- 2. held-out decision values of many models in one launch ----------------------------------------------------------------------
HELD = (0, 1, 31, 32, 33, 70)
SV_COUNTS = ((0, 5), (5, 0), (0, 0), (32, 32), (33, 1), (100, 67))


def _cv_jobs(D, seed):
    """every held-out count against every support-vector count: 36 jobs over one pool of rows"""
    r = np.random.RandomState(seed)
    n_pool = 300
    Z = (r.randn(n_pool, D) / np.sqrt(D) * 3).astype(np.float32)
    jobs = []
    for nh in HELD:
        for npos, nneg in SV_COUNTS:
            held = r.randint(0, n_pool, nh).astype(np.int32)
            sv = r.randint(0, n_pool, npos + nneg).astype(np.int32)
            coef = np.concatenate((r.rand(npos) + 0.01, -r.rand(nneg) - 0.01))
            jobs.append((held, sv, npos, coef, float(r.randn())))
    return Z, jobs


@pytest.mark.parametrize('kind', ref.KINDS)
@pytest.mark.parametrize('D', [5, 8, 36])
def test_cv_decision_equals_decision_per_job(gpu_required, D, kind):
    Z, jobs = _cv_jobs(D, 100 + D)
    kp = _lib.svm_kernel(kind, 4.0 / D, 0.5, 3)
    h = _lib.SVM()
    h.set_data(Z)
    got = h.cv_decision(kp, jobs)
    back = h.cv_decision(kp, jobs[::-1])[::-1]
    assert len(got) == len(jobs)
    for j, (held, sv, npos, coef, rho) in enumerate(jobs):
        cs = np.array([0, npos, sv.size], np.int64)
        want = h.decision(kp, cs, coef[None, :], [rho], x_idx=held, sv_idx=sv)[:, 0]
        assert got[j].shape == (held.size,)
        assert np.array_equal(got[j], want), j
        assert np.array_equal(back[j], want), j
        if sv.size == 0:
            assert np.array_equal(got[j], np.full(held.size, -rho))
    h.close()


def test_cv_decision_refuses_bad_rows_and_offsets(gpu_required):
    import ctypes as C
    Z, jobs = _cv_jobs(8, 3)
    kp = _lib.svm_kernel('rbf', 0.5)
    h = _lib.SVM()
    h.set_data(Z)
    held, sv, npos, coef, rho = jobs[-1]
    for bad in (-1, len(Z)):
        wrong = held.copy()
        wrong[3] = bad
        with pytest.raises(_lib.L3Error, match=r'error -1: .*held_rows\[3\]'):
            h.cv_decision(kp, [(wrong, sv, npos, coef, rho)])
        wrong = sv.copy()
        wrong[5] = bad
        with pytest.raises(_lib.L3Error, match=r'error -1: .*sv_rows\[5\]'):
            h.cv_decision(kp, [(held, wrong, npos, coef, rho)])
    with pytest.raises(_lib.L3Error, match=r'error -1: .*sv_neg'):
        h.cv_decision(kp, [(held, sv, sv.size + 1, coef, rho)])
    out = np.empty(held.size)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    hoff, soff, neg = np.array([0, held.size], np.int64), np.array([0, sv.size], np.int64), np.array([npos], np.int64)
    for h_off, s_off in ((np.array([0, -1], np.int64), soff), (hoff, np.array([0, -2], np.int64))):
        rc = h.lib.l3_svm_cv_decision(h.h, C.byref(kp), 1, ptr(h_off), ptr(held), ptr(s_off), ptr(neg), ptr(sv), ptr(coef),
                                      ptr(np.array([rho])), ptr(out))
        assert rc == -1
    h.close()


# ---- 3. sigmoid_train for every pair at once --------------------------------------------------------------------------------------
SIG_L = (2, 3, 63, 64, 65, 257, 1000, 4097)
_sig_cache = {}


def _sign(v):
    return np.where(v > 0, 1, -1).astype(np.int8)


def _sig_jobs():
    """per l one stream RandomState(1000 + l): the decisions, the label noise, then the labels that do not depend on the decisions"""
    jobs = []
    for l in SIG_L:
        r = np.random.RandomState(1000 + l)
        dec, noise = 2 * r.randn(l), r.randn(l)
        free = _sign(r.randn(l))
        jobs.append(('noisy', l, dec, _sign(dec + noise)))
        jobs.append(('wide', l, dec * 50, _sign(dec * 50 + 60 * noise)))
        jobs.append(('separable', l, dec, _sign(dec)))
        jobs.append(('one label', l, dec, np.ones(l, np.int8)))
        jobs.append(('constant', l, np.full(l, 0.75), free))
        jobs.append(('tiny', l, dec * 1e-6, free))
    return jobs


def _distance(dec, ab1, ab2):
    return float(np.abs(svm.sigmoid_predict(dec, *ab1) - svm.sigmoid_predict(dec, *ab2)).max())


def sigmoid_yardstick():
    """-> (jobs, the forward-loop fits, m): m is the largest distance in fitted probabilities, over all jobs, between three float64
    fits on the host that differ in the order of their sums only: the loop restatement forward, the same on reversed rows, and
    svm.sigmoid_train (NumPy's pairwise sums).  Computed once."""
    if 'm' not in _sig_cache:
        jobs = _sig_jobs()
        fwd, m, worst = [], 0.0, None
        for kind, l, dec, lab in jobs:
            a = ref.sigmoid_train(list(dec), list(lab))
            b = ref.sigmoid_train(list(dec[::-1]), list(lab[::-1]))
            c = svm.sigmoid_train(dec, lab)
            d = max(_distance(dec, a, b), _distance(dec, a, c), _distance(dec, b, c))
            if d > m:
                m, worst = d, (kind, l)
            fwd.append(a)
        _say('3 yardstick: m = %.3g at %s' % (m, worst))
        _sig_cache.update(jobs=jobs, fwd=fwd, m=m)
    return _sig_cache['jobs'], _sig_cache['fwd'], _sig_cache['m']


def test_sigmoid_train_matches_the_loop_restatement(gpu_required):
    jobs, fwd, m = sigmoid_yardstick()
    assert len(jobs) == 48
    assert m < 5e-8, m
    A, B, iters = _lib.svm_sigmoid_train(0, [j[2] for j in jobs], [j[3] for j in jobs])
    dist = np.array([_distance(j[2], (A[k], B[k]), fwd[k]) for k, j in enumerate(jobs)])
    for k, (kind, l, _, _) in enumerate(jobs):
        _say('3 %-9s l=%4d: iters %3d, distance to the forward loop %.3g' % (kind, l, iters[k], dist[k]))
    far = int((dist > 1e-12).sum())
    _say('3 device: largest distance %.3g (bound 8 m = %.3g), %d of %d jobs beyond 1e-12' % (dist.max(), 8 * m, far, len(jobs)))
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(B))
    assert np.all((iters >= 0) & (iters <= 100))
    assert dist.max() <= 8 * m, (float(dist.max()), m)
    assert far <= len(jobs) // 3, far


def test_sigmoid_train_job_does_not_depend_on_its_batch(gpu_required):
    jobs = _sig_jobs()
    A, B, iters = _lib.svm_sigmoid_train(0, [j[2] for j in jobs], [j[3] for j in jobs])
    for k, (kind, l, dec, lab) in enumerate(jobs):
        a, b, it = _lib.svm_sigmoid_train(0, [dec], [lab])
        assert (a[0], b[0], it[0]) == (A[k], B[k], iters[k]), (kind, l)


def test_sigmoid_train_refuses_bad_jobs(gpu_required):
    with pytest.raises(_lib.L3Error, match='error -1'):
        _lib.svm_sigmoid_train(0, [np.zeros(0)], [np.zeros(0, np.int8)])
    with pytest.raises(_lib.L3Error, match='error -1: .*signs'):
        _lib.svm_sigmoid_train(0, [np.ones(3)], [np.array([1, 0, -1], np.int8)])
    with pytest.raises(ValueError, match='one label per decision value'):
        _lib.svm_sigmoid_train(0, [np.ones(3)], [np.ones(2, np.int8)])


# ---- 4. fit_grid against SVC.fit per cost -------------------------------------------------------------------------------------------
# class sizes (n = 240, one class of 4 rows) at which, with random_state 7, some cross-validation fold of some pair trains on one
# class only (libsvm's fixed decision values): found by enumeration, asserted below
GRID_SIZES = {3: (29, 207, 4), 12: (18, 23, 24, 19, 27, 13, 21, 22, 29, 22, 4, 18)}
GRID_D = 16
SOLVER_ATTRS = ('classes_', 'support_', 'support_vectors_', 'n_support_', 'dual_coef_', 'intercept_', '_dual_coef_', '_intercept_',
                '_sv_start', 'n_iter_', 'n_outer_')
_grid_cache = {}


def _grid_data(nc):
    sizes = GRID_SIZES[nc]
    r = np.random.RandomState(nc)
    y = np.repeat(np.arange(nc) * 3 + 1, sizes)          # labels that are not their own indices
    r.shuffle(y)
    centres = r.randn(nc, GRID_D) * 0.6
    X = (centres[(y - 1) // 3] + r.randn(y.size, GRID_D)).astype(np.float32)
    return X, y


def _separate_fits(nc):
    """SVC(C=c, probability=True, random_state=7).fit per cost, and fit_grid's two Platt modes from NumPy rows: fitted once"""
    if nc not in _grid_cache:
        X, y = _grid_data(nc)
        alone = [SVC(C=c, probability=True, random_state=7).fit(X, y) for c in CS]
        host = svm.fit_grid(X, y, CS, platt='host', probability=True, random_state=7, keep_cv_decisions=True)
        dev = svm.fit_grid(X, y, CS, platt='device', probability=True, random_state=7)
        _grid_cache[nc] = (X, y, alone, host, dev)
    return _grid_cache[nc]


def _assert_solver_equal(models, alone):
    assert len(models) == len(alone)
    for m, a in zip(models, alone):
        assert m.C == a.C
        for name in SOLVER_ATTRS:
            assert np.array_equal(getattr(m, name), getattr(a, name)), (m.C, name)


def _assert_platt_equal(models, alone):
    for m, a in zip(models, alone):
        assert np.array_equal(m.probA_, a.probA_) and np.array_equal(m.probB_, a.probB_), m.C


def _assert_platt_close(models, host, what):
    """Platt's sigmoids fitted on the device against the host path's, as probabilities on the cross-validation decision values
    they were fitted on, within 8 m (sigmoid_yardstick)"""
    m = sigmoid_yardstick()[2]
    worst = 0.0
    for got, want in zip(models, host):
        assert got.probA_.shape == want.probA_.shape and got.probA_.dtype == np.float64
        for p, dec in enumerate(want.cv_decisions_):
            worst = max(worst, _distance(dec, (got.probA_[p], got.probB_[p]), (want.probA_[p], want.probB_[p])))
    _say('4 %s: pair probabilities of the device sigmoid fit within %.3g of the host fit (bound %.3g)' % (what, worst, 8 * m))
    assert worst <= 8 * m, (worst, m)


@pytest.mark.parametrize('nc', [3, 12])
def test_fit_grid_equals_separate_fits(gpu_required, nc):
    X, y, alone, host, dev = _separate_fits(nc)
    _, yenc = np.unique(y, return_inverse=True)
    cv, _ = svm.cv_problems(svm.pair_problems(yenc, nc)[2], 7)
    assert any(isinstance(job, float) for _, _, job in cv), 'no fold with one class: the fixed decision values are not covered'
    _assert_solver_equal(host, alone)
    _assert_platt_equal(host, alone)
    _assert_solver_equal(dev, alone)
    _assert_platt_close(dev, host, '%d classes' % nc)
    assert max(m.n_iter_.max() for m in alone) > 0 and len({m.support_.size for m in alone}) > 1


@pytest.mark.parametrize('nc', [3, 12])
def test_fit_grid_from_device_features(gpu_required, nc):
    X, y, alone, host, _ = _separate_fits(nc)
    feats = DeviceFeatures(X)
    got = svm.fit_grid(feats, y, CS, platt='host', probability=True, random_state=7)
    _assert_solver_equal(got, alone)
    _assert_platt_equal(got, alone)
    got = svm.fit_grid(feats, y, CS, platt='device', probability=True, random_state=7)
    _assert_solver_equal(got, alone)
    _assert_platt_close(got, host, '%d classes, DeviceFeatures' % nc)
    feats.close()


@pytest.mark.parametrize('nc', [3, 12])
def test_fit_grid_does_not_depend_on_the_entry_budget(gpu_required, nc, monkeypatch):
    X, y, alone, host, dev = _separate_fits(nc)
    calls = []
    fit = _lib.SVM.fit
    monkeypatch.setattr(_lib.SVM, 'fit', lambda self, kp, problems, **kw: calls.append(len(problems)) or fit(self, kp, problems, **kw))
    _, yenc = np.unique(y, return_inverse=True)
    problems = svm.pair_problems(yenc, nc)[2]
    per_cost = problems + svm.cv_problems(problems, 7)[1]
    entries = sum(rows.size for rows, _ in per_cost)
    got = svm.fit_grid(X, y, CS, platt='host', max_entries=2 * entries, probability=True, random_state=7)
    assert calls == [2 * len(per_cost), 2 * len(per_cost), len(per_cost)]
    _assert_solver_equal(got, alone)
    _assert_platt_equal(got, alone)
    got = svm.fit_grid(X, y, CS, platt='device', max_entries=2 * entries, probability=True, random_state=7)
    _assert_solver_equal(got, alone)
    for g, d in zip(got, dev):      # the sigmoid fit of a pair does not depend on its batch either
        assert np.array_equal(g.probA_, d.probA_) and np.array_equal(g.probB_, d.probB_)


def test_grid_models_share_a_handle_and_evaluate_interleaved(gpu_required):
    X, y, alone, host, _ = _separate_fits(12)
    r = np.random.RandomState(5)
    Xt = (X[r.randint(0, len(X), 50)] + 0.3 * r.randn(50, GRID_D)).astype(np.float32)
    yt = y[r.randint(0, len(y), 50)]
    outputs = ('predict', 'decision_function', 'hinge_loss', 'predict_proba', 'file_predict')
    kw = dict(y=yt, file_idxs=[(0, 20), (20, 50)], outputs=outputs)
    a, b = host[1], host[4]
    assert a._h is b._h
    want_a, want_b = alone[1].evaluate(Xt, **kw), alone[4].evaluate(Xt, **kw)
    assert not np.array_equal(want_a['decision_function'], want_b['decision_function'])
    for model, want in ((a, want_a), (b, want_b), (a, want_a), (a, want_a), (b, want_b)):
        got = model.evaluate(Xt, **kw)
        for k in outputs:
            assert np.array_equal(got[k], want[k]), k
    again = pickle.loads(pickle.dumps(b))
    assert again._h is None and np.array_equal(again.evaluate(Xt, **kw)['predict_proba'], want_b['predict_proba'])


def test_fit_grid_without_probability(gpu_required):
    X, y = _grid_data(3)
    got = svm.fit_grid(X, y, (0.5, 2), gamma=0.1)
    for m in got:
        a = SVC(C=m.C, gamma=0.1).fit(X, y)
        _assert_solver_equal([m], [a])
        assert m.probA_.size == 0 and not m.probability


# ---- 5. the search over C and the fold driver ---------------------------------------------------------------------------------------
def _search_splits(seed=0, nc=4, D=12):
    r = np.random.RandomState(seed)
    centres = r.randn(nc, D) * 0.9

    def split(n, files=None):
        y = np.arange(n) % nc
        X = (centres[y] + r.randn(n, D)).astype(np.float32)
        return {'features': X, 'labels': y}

    train, valid = split(160), split(60)
    # the test split: 8 files of 6 frames, one label per file
    yf = np.arange(8) % nc
    Xf = (centres[np.repeat(yf, 6)] + r.randn(48, D)).astype(np.float32)
    test = {'features': Xf, 'labels': yf, 'file_idxs': [(6 * f, 6 * f + 6) for f in range(8)]}
    return train, valid, test


@pytest.mark.parametrize('train_with_valid', [False, True])
def test_train_svm_search_equals_the_search_over_train_svm(gpu_required, tmp_path, train_with_valid):
    train, valid, test = _search_splits()
    d1, d2 = str(tmp_path / 'a'), str(tmp_path / 'b')
    os.makedirs(d1), os.makedirs(d2)
    np.random.seed(11)
    want = classifier.train_param_search(train, valid, test, d1, train_func=classifier.train_svm, search_space={'C': list(CS)},
                                         train_with_valid=train_with_valid, evaluate_on_device=True, num_classes=4, random_state=3)
    np.random.seed(11)
    got = classifier.train_svm_search(train, valid, test, d2, Cs=CS, train_with_valid=train_with_valid, platt='host',
                                      num_classes=4, random_state=3)
    assert got[0].C == want[0].C
    assert got[1]['search_params_best_values'] == want[1]['search_params_best_values']
    for k in range(1, 4):
        np.testing.assert_equal(got[k], want[k])         # dictionaries, lists and NaN (a class without examples) alike
    assert set(got[2]['search']) == {(c,) for c in CS} and got[1]['search_params'] == ['C']
    for name in SOLVER_ATTRS + ('probA_', 'probB_'):
        assert np.array_equal(getattr(got[0], name), getattr(want[0], name)), name
    with open(os.path.join(d2, 'model.pkl'), 'rb') as fh:
        saved = pickle.load(fh)
    assert saved.C == got[0].C and np.array_equal(saved.support_, got[0].support_)
    # the device's sigmoid fit chooses the same cost on this data and reports the same accuracies
    np.random.seed(11)
    dev = classifier.train_svm_search(train, valid, test, d2, Cs=CS, train_with_valid=train_with_valid, num_classes=4, random_state=3)
    assert dev[0].C == want[0].C and dev[2]['accuracy'] == want[2]['accuracy'] and dev[1]['loss'] == want[1]['loss']


def _write_fold_dir(root, dataset='esc50', folds=5, D=12, C=3, files=3, frames=5, seed=0):
    """features/<dataset>/l3/synthetic/fold1..foldN/*.npz as usc_generate writes them (X frames, y the class)"""
    r = np.random.RandomState(seed)
    centres = r.randn(C, D) * 1.5
    fdir = os.path.join(root, 'features', dataset, 'l3', 'synthetic')
    for f in range(folds):
        d = os.path.join(fdir, 'fold%d' % (f + 1))
        os.makedirs(d)
        for c in range(C):
            for k in range(files):
                np.savez(os.path.join(d, '%d-%d-%d.npz' % (f, c, k)), X=(centres[c] + r.randn(frames, D)).astype(np.float32),
                         y=np.array(c))
    return fdir


@pytest.mark.parametrize('fold_num,search,device', [(1, False, None), (2, True, 0)])
def test_train_svm_fold_writes_the_fold(gpu_required, tmp_path, fold_num, search, device):
    """two folds of the smallest layout that leaves a training fold beside the validation and the test fold (esc50's five)"""
    fdir = _write_fold_dir(str(tmp_path))
    out = str(tmp_path / 'out')
    mdir = classifier.train_svm_fold(fdir, out, fold_num, parameter_search=search, preprocess_device=device, C=2.0)
    assert os.path.relpath(mdir, out).split(os.sep)[:8] == ['classifier', 'esc50', 'l3', 'synthetic', 'framewise', 'overlap',
                                                             'no-min-max', 'svm']
    assert sorted(os.listdir(mdir)) == ['config.json', 'min_max_scaler.pkl', 'model.pkl', 'results.pkl', 'stdizer.pkl']
    with open(os.path.join(mdir, 'model.pkl'), 'rb') as fh:
        model = pickle.load(fh)
    with open(os.path.join(mdir, 'results.pkl'), 'rb') as fh:
        results = pickle.load(fh)
    assert sorted(results) == ['test', 'train', 'valid'] and len(results['test']['class_accuracy']) == 50
    assert results['train']['accuracy'] > 0.8 and results['test']['accuracy'] > 0.5
    assert ('search' in results['valid']) == search
    assert model.probability and model.classes_.size == 3 and (search or model.C == 2.0)
    r = np.random.RandomState(1)
    assert model.predict(r.randn(4, 12).astype(np.float32)).shape == (4,)
