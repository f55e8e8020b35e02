"""The reference's SVM sound classifier (classifier/train.py:79-166): sklearn.svm.SVC of scikit-learn 0.19.0, i.e. libsvm's C-SVC,
trained and evaluated on the GPU through the l3_svm handle of libl3hip (csrc/svm.hip).

Here are the multiclass shell and probability estimates of libsvm's svm_train / svm_predict_probability (svm.cpp): one-vs-one
pairs, support vectors grouped by class with the (C - 1, n_SV) coefficient matrix, the vote, Platt scaling fitted on 5-fold
cross-validation decision values, and pairwise coupling.  Every binary problem (the pairs and their cross-validation
sub-problems) goes through the GPU solver in one batched call; the sigmoid fit stays on the host in NumPy.  fit_grid fits the
models of a grid over C in one pass: one solver call with a cost per problem, one launch for the held-out decision values of
every cross-validation sub-problem, one for the sigmoid fits of every pair and cost (csrc/svm_eval.hip).  predict,
decision_function and predict_proba of NumPy rows vote and couple on the host in NumPy; SVC.evaluate scores a split in one pass on
the GPU (csrc/svm_eval.hip: vote, ovr values, hinge loss, Platt probabilities, coupling, per-file means) and takes
usc.DeviceFeatures as it is, as fit does.

Deviations from sklearn 0.19 / libsvm, all deliberate:
  * the cross-validation fold permutation of probability estimates is drawn from np.random.RandomState(random_state) (libsvm
    uses the C library's rand()), as the MLP's epoch shuffle is;
  * the solver is decomposition with working sets of q variables (libsvm's WSS3 inside each), without libsvm's shrinking heuristic
    or kernel cache; kernel values are fp32 (libsvm also stores them as float), alpha and the gradient float64.  The solution meets
    the same stopping test m(alpha) - M(alpha) < tol, so it agrees with libsvm's to the accuracy tol allows, not bit for bit;
  * max_iter caps the local SMO updates per problem (the closest analogue of libsvm's iteration count);
  * class_weight, sample weights, shrinking and cache_size are not built.
"""
import logging

import numpy as np

from . import _lib
from .usc import DeviceFeatures

LOGGER = logging.getLogger('classifier')

NR_FOLD = 5
MIN_PROB = 1e-7
EVALUATE_OUTPUTS = ('predict', 'decision_function', 'hinge_loss', 'predict_proba', 'file_proba', 'file_predict')


# ---- libsvm's probability estimates (svm.cpp), float64 on the host -----------------------------------------------------------
def _sigmoid_loss(dec, t, A, B):
    f = dec * A + B
    pos = f >= 0
    out = np.empty_like(f)
    out[pos] = t[pos] * f[pos] + np.log(1 + np.exp(-f[pos]))
    out[~pos] = (t[~pos] - 1) * f[~pos] + np.log(1 + np.exp(f[~pos]))
    return out.sum()


def sigmoid_train(dec, labels):
    """svm.cpp sigmoid_train: Platt's sigmoid fitted with the Newton method and backtracking of Lin, Lin and Weng. -> (A, B)"""
    dec = np.asarray(dec, np.float64)
    labels = np.asarray(labels)
    prior1 = float((labels > 0).sum())
    prior0 = float(labels.size - prior1)
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    t = np.where(labels > 0, (prior1 + 1.0) / (prior1 + 2.0), 1 / (prior0 + 2.0))
    A, B = 0.0, np.log((prior0 + 1.0) / (prior1 + 1.0))
    fval = _sigmoid_loss(dec, t, A, B)
    for _ in range(max_iter):
        f = dec * A + B
        e = np.exp(-np.abs(f))
        # p = 1 / (1 + exp(f)), q = 1 - p, in the branch that keeps exp's argument <= 0
        p = np.where(f >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
        q = np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        d2 = p * q
        h11 = sigma + (dec * dec * d2).sum()
        h22 = sigma + d2.sum()
        h21 = (dec * d2).sum()
        d1 = t - p
        g1, g2 = (dec * d1).sum(), d1.sum()
        if abs(g1) < eps and abs(g2) < eps:
            break
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= min_step:
            nA, nB = A + step * dA, B + step * dB
            nf = _sigmoid_loss(dec, t, nA, nB)
            if nf < fval + 0.0001 * step * gd:
                A, B, fval = nA, nB, nf
                break
            step /= 2.0
        if step < min_step:
            LOGGER.info('Line search fails in two-class probability estimates')
            break
    return A, B


def sigmoid_predict(dec, A, B):
    """svm.cpp sigmoid_predict, elementwise"""
    f = np.asarray(dec, np.float64) * A + B
    e = np.exp(-np.abs(f))
    return np.where(f >= 0, e / (1.0 + e), 1.0 / (1.0 + e))


def multiclass_probability(r):
    """svm.cpp multiclass_probability (method 2 of Wu, Lin and Weng), for every row at once: r (n, k, k) pairwise probabilities
    r[i, j] = P(i | i or j) -> (n, k).  Each row iterates until its own stopping test, as libsvm does per row."""
    r = np.asarray(r, np.float64)
    n, k = r.shape[:2]
    Q = np.empty((n, k, k))
    for t in range(k):
        others = [j for j in range(k) if j != t]
        Q[:, t, t] = (r[:, others, t] ** 2).sum(axis=1) if others else 0.0
        for j in others:
            Q[:, t, j] = -r[:, j, t] * r[:, t, j]
    p = np.full((n, k), 1.0 / k)
    eps = 0.005 / k
    live = np.arange(n)
    for _ in range(max(100, k)):
        if live.size == 0:
            break
        Ql, pl = Q[live], p[live]
        Qp = np.einsum('ntj,nj->nt', Ql, pl)
        pQp = (pl * Qp).sum(axis=1)
        go = np.abs(Qp - pQp[:, None]).max(axis=1) >= eps
        live, Ql, pl, Qp, pQp = live[go], Ql[go], pl[go], Qp[go], pQp[go]
        for t in range(k):
            diff = (-Qp[:, t] + pQp) / Ql[:, t, t]
            pl[:, t] += diff
            pQp = (pQp + diff * (diff * Ql[:, t, t] + 2 * Qp[:, t])) / (1 + diff) / (1 + diff)
            Qp = (Qp + diff[:, None] * Ql[:, t, :]) / (1 + diff)[:, None]
            pl /= (1 + diff)[:, None]
        p[live] = pl
    return p


def ovr_decision_function(predictions, confidences, n_classes):
    """sklearn 0.19 sklearn.utils.multiclass._ovr_decision_function: votes + sum of confidences / (3 (|sum| + 1))"""
    n = predictions.shape[0]
    votes = np.zeros((n, n_classes))
    conf = np.zeros((n, n_classes))
    k = 0
    for i in range(n_classes):
        for j in range(i + 1, n_classes):
            conf[:, i] -= confidences[:, k]
            conf[:, j] += confidences[:, k]
            votes[predictions[:, k] == 0, i] += 1
            votes[predictions[:, k] == 1, j] += 1
            k += 1
    return votes + conf / (3 * (np.abs(conf) + 1))


def hinge_loss(y_true, pred_decision, labels=None):
    """sklearn 0.19 sklearn.metrics.hinge_loss: the multiclass margin is the true class's decision value minus the largest other
    one (Crammer-Singer); with two classes, y in {-1, +1} (the larger label +1) times the one decision value."""
    y_true = np.asarray(y_true).reshape(-1)
    pred = np.asarray(pred_decision, np.float64)
    present = np.unique(y_true)
    if present.size > 2:
        if labels is None and pred.ndim > 1 and present.size != pred.shape[1]:
            raise ValueError('Please include all labels in y_true or pass labels as third argument')
        lab = np.unique(present if labels is None else np.asarray(labels))
        if not np.all(np.isin(y_true, lab)):
            raise ValueError('y_true contains labels not in labels')
        yi = np.searchsorted(lab, y_true)
        rows = np.arange(y_true.size)
        margin = pred[rows, yi].copy()
        others = pred.copy()
        others[rows, yi] = -np.inf
        margin -= others.max(axis=1)
    else:
        pred = pred.reshape(-1)
        if pred.size != y_true.size:
            raise ValueError('pred_decision should hold one value per sample')
        y = np.where(y_true == present[-1], 1.0, -1.0) if present.size == 2 else -np.ones(y_true.size)
        margin = y * pred
    losses = 1 - margin
    losses[losses <= 0] = 0
    return float(np.mean(losses))


# ---- the problems of a fit: what SVC.fit and fit_grid assemble alike ---------------------------------------------------------------
def _check_rows(X, y):
    """-> (X as fit takes it, y flat, whether X is a usc.DeviceFeatures)"""
    on_device = isinstance(X, DeviceFeatures)
    if not on_device:
        X = np.ascontiguousarray(X, np.float32)
    y = np.asarray(y).reshape(-1)
    if len(X.shape) != 2 or X.shape[0] != y.size:
        raise ValueError('X must be (n_samples, n_features) with one label per row')
    return X, y, on_device


def _encode_classes(y):
    classes, yenc = np.unique(y, return_inverse=True)
    if classes.size < 2:
        raise ValueError('The number of classes has to be greater than one; got %d' % classes.size)
    if classes.size > _lib.SVM_MAX_CLASSES:
        raise ValueError('at most %d classes are built' % _lib.SVM_MAX_CLASSES)
    return classes, yenc


def pair_problems(yenc, nc):
    """libsvm's one-vs-one problems -> (groups: the rows of each class, pairs (i, j), problems: (rows, signs) per pair with class i
    first and +1)"""
    groups = [np.flatnonzero(yenc == c).astype(np.int32) for c in range(nc)]
    pairs = [(i, j) for i in range(nc) for j in range(i + 1, nc)]
    problems = [(np.concatenate((groups[i], groups[j])),
                 np.concatenate((np.ones(groups[i].size, np.int8), -np.ones(groups[j].size, np.int8)))) for i, j in pairs]
    return groups, pairs, problems


def cv_problems(problems, random_state):
    """svm_binary_svc_probability's 5 folds of every pair, the permutations drawn from np.random.RandomState(random_state) pair after
    pair -> (cv, sub): cv lists (pair, held-out positions in the pair's rows, job), job being a sub-problem as its number in
    problems + sub, or libsvm's fixed decision value (a float) for a fold whose training part holds one class or none; sub lists
    the sub-problems (rows, signs)"""
    cv, sub = [], []
    rs = np.random.RandomState(random_state)
    for p, (rows, signs) in enumerate(problems):
        l = rows.size
        perm = rs.permutation(l)
        for f in range(NR_FOLD):
            begin, end = f * l // NR_FOLD, (f + 1) * l // NR_FOLD
            train_pos = np.concatenate((perm[:begin], perm[end:]))
            npos = int((signs[train_pos] > 0).sum())
            nneg = train_pos.size - npos
            if npos == 0 or nneg == 0:      # libsvm's fixed decision values for a fold with one class (or none)
                cv.append((p, perm[begin:end], 0.0 if npos == nneg else (1.0 if npos else -1.0)))
            else:
                cv.append((p, perm[begin:end], len(problems) + len(sub)))
                sub.append((rows[train_pos], signs[train_pos]))
    return cv, sub


def _binary_model(rows, signs, a):
    """a solved binary problem as the decision launches take it -> (support-vector rows, positives first; their count of positives;
    the coefficients y alpha)"""
    nz = a > 0
    pos, neg = nz & (signs > 0), nz & (signs < 0)
    return np.concatenate((rows[pos], rows[neg])), int(pos.sum()), np.concatenate((a[pos], -a[neg]))


# ---- SVC -------------------------------------------------------------------------------------------------------------------------
class SVC(object):
    """sklearn 0.19.0's sklearn.svm.SVC (C-SVC) on the GPU: fit / predict / decision_function / predict_proba and sklearn's
    fitted attributes (classes_, support_, support_vectors_, n_support_, dual_coef_, intercept_, probA_, probB_).  The fitted
    model pickles without its device handle and predicts again after unpickling."""

    def __init__(self, C=1.0, kernel='rbf', degree=3, gamma='auto', coef0=0.0, tol=1e-3, max_iter=-1, probability=False,
                 random_state=None, verbose=False, decision_function_shape='ovr', device=0, ws_size=0):
        self.C, self.kernel, self.degree, self.gamma, self.coef0 = C, kernel, degree, gamma, coef0
        self.tol, self.max_iter, self.probability, self.random_state = tol, max_iter, probability, random_state
        self.verbose, self.decision_function_shape, self.device, self.ws_size = verbose, decision_function_shape, device, ws_size
        self._h = None

    # pickling: everything but the device handle
    def __getstate__(self):
        state = dict(self.__dict__)
        state['_h'] = state['_key'] = None
        state['_model_set'] = state['_resident'] = False
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    def _handle(self):
        if self._h is None:
            self._h = _lib.SVM(self.device)
        return self._h

    def _kernel(self):
        return _lib.svm_kernel(self.kernel, self._gamma, self.coef0, self.degree)

    def fit(self, X, y):
        """X: NumPy rows, or a usc.DeviceFeatures, which is copied on the device (no download; the solver sees the same bits)"""
        X, y, on_device = _check_rows(X, y)
        if not self.C > 0:
            raise ValueError('C <= 0')
        if self.kernel not in _lib.SVM_KERNELS:
            raise ValueError('kernel must be one of %s' % sorted(_lib.SVM_KERNELS))
        self.classes_, yenc = _encode_classes(y)
        nc = self.classes_.size
        self.shape_fit_ = tuple(X.shape)
        self._gamma = 1.0 / X.shape[1] if self.gamma == 'auto' else float(self.gamma)
        self._model_set = self._resident = False
        h = self._handle()
        if on_device:
            h.set_data_dev(X.handle)
        else:
            h.set_data(X)
        kp = self._kernel()
        groups, pairs, problems = pair_problems(yenc, nc)
        # cv: (pair, held-out positions in the pair's rows, sub-problem number or a fixed value)
        cv, sub = cv_problems(problems, self.random_state) if self.probability else ([], [])
        alphas, rho, updates, outer, gaps = h.fit(kp, problems + sub, cost=self.C, tol=self.tol, max_iter=self.max_iter,
                                                  q=self.ws_size)
        self._solved(updates, outer, len(problems))
        self._build_model(h.get_rows if on_device else X.__getitem__, y.size, groups, pairs, problems, alphas, rho)
        if self.probability:
            self.probA_, self.probB_ = self._platt(h, kp, problems, sub, cv, alphas, rho)
        else:
            self.probA_ = self.probB_ = np.empty(0)
        self._resident = True          # the support vectors are rows support_ of this handle's matrix
        return self

    def _solved(self, updates, outer, n_pairs):
        """the solver's counts of this model's problems (the pairs first)"""
        self.n_iter_ = updates[:n_pairs].copy()
        self.n_outer_ = outer[:n_pairs].copy()
        if self.max_iter is not None and self.max_iter > 0 and np.any(updates >= self.max_iter):
            LOGGER.warning('Solver terminated early (max_iter=%d).  Consider pre-processing your data with StandardScaler or '
                           'MinMaxScaler.', self.max_iter)

    def _build_model(self, rows_of, n_rows, groups, pairs, problems, alphas, rho):
        """svm.cpp svm_train's multiclass model: support vectors grouped by class, sv_coef (C - 1, n_SV), rho per pair"""
        nc = len(groups)
        nonzero = np.zeros(n_rows, bool)
        for (rows, _), a in zip(problems, alphas):
            nonzero[rows[a > 0]] = True
        sv_of = [g[nonzero[g]] for g in groups]
        self.n_support_ = np.array([s.size for s in sv_of], np.int32)
        self.support_ = np.concatenate(sv_of).astype(np.int32)
        self.support_vectors_ = rows_of(self.support_)
        start = np.concatenate(([0], np.cumsum(self.n_support_)))
        pos = np.full(n_rows, -1, np.int64)
        pos[self.support_] = np.arange(self.support_.size)
        coef = np.zeros((nc - 1, self.support_.size))
        for (i, j), (rows, signs), a in zip(pairs, problems, alphas):
            ya = signs * a
            nz = a > 0
            ri, rj = rows[:groups[i].size], rows[groups[i].size:]
            mi, mj = nz[:groups[i].size], nz[groups[i].size:]
            coef[j - 1, pos[ri[mi]]] = ya[:groups[i].size][mi]
            coef[i, pos[rj[mj]]] = ya[groups[i].size:][mj]
        self._sv_start = start.astype(np.int64)
        self._dual_coef_ = coef
        self._intercept_ = -np.asarray(rho[:len(pairs)], np.float64)
        self.dual_coef_, self.intercept_ = coef.copy(), self._intercept_.copy()
        if nc == 2:                 # sklearn flips the binary model so that positive means classes_[1]
            self.dual_coef_, self.intercept_ = -self.dual_coef_, -self.intercept_

    def _platt(self, h, kp, problems, sub, cv, alphas, rho):
        """svm_binary_svc_probability for every pair: decision values of the held-out folds (GPU), then sigmoid_train"""
        allp = problems + sub
        decs = [np.empty(rows.size) for rows, _ in problems]
        for p, held, job in cv:
            if isinstance(job, float):
                decs[p][held] = job
                continue
            sv, npos, coef = _binary_model(allp[job][0], allp[job][1], alphas[job])
            cs = np.array([0, npos, sv.size], np.int64)
            decs[p][held] = h.decision(kp, cs, coef[None, :], [rho[job]], x_idx=problems[p][0][held], sv_idx=sv)[:, 0]
        A, B = np.empty(len(problems)), np.empty(len(problems))
        for p, (rows, signs) in enumerate(problems):
            A[p], B[p] = sigmoid_train(decs[p], signs)
        return A, B

    def _check_fitted(self):
        if not hasattr(self, 'support_'):
            raise ValueError('This SVC instance is not fitted yet')

    def _ovo(self, X):
        """libsvm's pairwise decision values (n, P): positive for the first class of the pair"""
        self._check_fitted()
        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2 or X.shape[1] != self.shape_fit_[1]:
            raise ValueError('X has %s features per sample; expecting %d' % (X.shape[1:], self.shape_fit_[1]))
        return self._handle().decision(self._kernel(), self._sv_start, self._dual_coef_, -self._intercept_, X=X,
                                       SV=self.support_vectors_)

    def _ensure_model(self):
        """the resident model of evaluate: set once per fitted model, and again after unpickling"""
        h = self._handle()
        # models fitted together (fit_grid) share one handle, which holds one model at a time: the handle names its owner
        if not getattr(self, '_model_set', False) or getattr(h, 'model_owner', None) is not self._owner_key():
            prob = dict(probA=self.probA_, probB=self.probB_) if self.probability else {}
            sv = dict(sv_idx=self.support_) if getattr(self, '_resident', False) else dict(SV=self.support_vectors_)
            h.set_model(self._kernel(), self._sv_start, self._dual_coef_, -self._intercept_, **dict(sv, **prob))
            self._model_set = True
            h.model_owner = self._owner_key()
        return h

    def _owner_key(self):
        """what a shared handle remembers of the object whose model it holds (not the object: no reference cycle)"""
        if self.__dict__.get('_key') is None:
            self._key = object()
        return self._key

    def evaluate(self, X, y=None, file_idxs=None, outputs=('predict',)):
        """One scoring pass on the GPU over X (NumPy rows or a usc.DeviceFeatures) -> dict of what `outputs` names, and nothing
        else is computed or downloaded: 'predict' (n) as classes_, 'decision_function' (n, C) sklearn's ovr values ((n) for two
        classes), 'hinge_loss' (sklearn's, of y against those values), 'predict_proba' (n, C), 'file_proba' (n_files, C) the mean
        of the rows [s, e) of each file_idxs entry and 'file_predict' its argmax as classes_."""
        self._check_fitted()
        outputs = tuple(outputs)
        unknown = set(outputs) - set(EVALUATE_OUTPUTS)
        if unknown:
            raise ValueError('unknown outputs %s; choose from %s' % (sorted(unknown), list(EVALUATE_OUTPUTS)))
        if 'hinge_loss' in outputs and y is None:
            raise ValueError("'hinge_loss' needs the labels y")
        files = None
        if 'file_proba' in outputs or 'file_predict' in outputs:
            if file_idxs is None:
                raise ValueError("'file_proba' and 'file_predict' need file_idxs")
            files = np.asarray(file_idxs, np.int64).reshape(-1, 2)
        if not self.probability and set(outputs) & {'predict_proba', 'file_proba', 'file_predict'}:
            raise ValueError('probability outputs are not available when probability=False')
        nc = self.classes_.size
        if 'decision_function' in outputs and nc > 2 and self.decision_function_shape != 'ovr':
            raise ValueError("evaluate gives sklearn's ovr decision values only; the pair decisions stay on the device")
        on_device = isinstance(X, DeviceFeatures)
        if not on_device:
            X = np.ascontiguousarray(X, np.float32)
        if len(X.shape) != 2 or X.shape[1] != self.shape_fit_[1]:
            raise ValueError('X has %s features per sample; expecting %d' % (tuple(X.shape[1:]), self.shape_fit_[1]))
        n = X.shape[0]
        labels = None
        if 'hinge_loss' in outputs:
            y = np.asarray(y).reshape(-1)
            if y.size != n:
                raise ValueError('one label per row is needed')
            labels = np.clip(np.searchsorted(self.classes_, y), 0, nc - 1)
            if not np.array_equal(self.classes_[labels], y):
                raise ValueError('y contains labels not in classes_')
        if files is not None and (files.size == 0 or files.min() < 0 or files.max() > n or np.any(files[:, 0] >= files[:, 1])):
            raise ValueError('file_idxs must be non-empty row ranges inside [0, n)')
        names = {'predict': 'pred', 'decision_function': 'ovr', 'hinge_loss': 'hinge_sum', 'predict_proba': 'proba',
                 'file_proba': 'file_proba', 'file_predict': 'file_pred'}
        if n == 0:
            raise ValueError('no rows to evaluate')
        h = self._ensure_model()
        got = h.score(labels=labels, files=files, outputs=tuple(names[k] for k in outputs),
                      **(dict(feat=X.handle) if on_device else dict(X=X)))
        out = {k: got[names[k]] for k in outputs}
        if 'predict' in out:
            out['predict'] = self.classes_[out['predict']]
        if 'file_predict' in out:
            out['file_predict'] = self.classes_[out['file_predict']]
        if 'hinge_loss' in out:
            out['hinge_loss'] = out['hinge_loss'] / n
        return out

    def decision_function(self, X):
        if isinstance(X, DeviceFeatures):
            return self.evaluate(X, outputs=('decision_function',))['decision_function']
        dec = self._ovo(X)
        nc = self.classes_.size
        if nc == 2:
            return -dec.ravel()
        if self.decision_function_shape == 'ovr':
            return ovr_decision_function(dec < 0, -dec, nc)
        return dec

    def predict(self, X):
        """libsvm's one-vs-one vote, ties to the lower class"""
        if isinstance(X, DeviceFeatures):
            return self.evaluate(X, outputs=('predict',))['predict']
        dec = self._ovo(X)
        nc = self.classes_.size
        votes = np.zeros((dec.shape[0], nc), np.int64)
        k = 0
        for i in range(nc):
            for j in range(i + 1, nc):
                win = dec[:, k] > 0
                votes[win, i] += 1
                votes[~win, j] += 1
                k += 1
        return self.classes_[votes.argmax(axis=1)]

    def predict_proba(self, X):
        """svm_predict_probability: sigmoid_predict of each pair's decision value, clipped to [1e-7, 1 - 1e-7], then coupled"""
        if not self.probability:
            raise AttributeError('predict_proba is not available when probability=False')
        if isinstance(X, DeviceFeatures):
            return self.evaluate(X, outputs=('predict_proba',))['predict_proba']
        return pairwise_coupling(self._ovo(X), self.probA_, self.probB_, self.classes_.size)


def pairwise_coupling(dec, probA, probB, n_classes):
    """libsvm's svm_predict_probability from the pairwise decision values (n, P) and Platt's (A, B) per pair -> (n, C)"""
    dec = np.asarray(dec, np.float64).reshape(-1, n_classes * (n_classes - 1) // 2)
    n = dec.shape[0]
    r = np.zeros((n, n_classes, n_classes))
    k = 0
    for i in range(n_classes):
        for j in range(i + 1, n_classes):
            pij = np.clip(sigmoid_predict(dec[:, k], probA[k], probB[k]), MIN_PROB, 1 - MIN_PROB)
            r[:, i, j], r[:, j, i] = pij, 1 - pij
            k += 1
    return multiclass_probability(r)


# ---- the grid over C in one pass -----------------------------------------------------------------------------------------------
PLATT_MODES = ('device', 'host')


def grid_problems(yenc, nc, Cs, probability, random_state):
    """what fit_grid solves: per cost, the problems SVC(C=c, random_state=random_state).fit assembles (pair_problems, cv_problems)
    -> (groups, pairs, problems, folds): folds holds one (cv, sub) per cost.  A fixed random_state gives every cost the same folds,
    as separate fits would draw them; None draws anew for every cost, as separate fits would."""
    groups, pairs, problems = pair_problems(yenc, nc)
    folds = []
    for _ in Cs:
        if not probability:
            folds.append(([], []))
        elif folds and random_state is not None and not isinstance(random_state, np.random.RandomState):
            folds.append(folds[0])
        else:
            folds.append(cv_problems(problems, random_state))
    return groups, pairs, problems, folds


def _cost_batches(entries, budget):
    """consecutive costs per solver call: as many as keep the call's entries (rows over all its problems) within the budget, one
    at least -> list of index lists"""
    batches, used = [], 0
    for g, e in enumerate(entries):
        if not batches or (budget is not None and used + e > budget):
            batches.append([])
            used = 0
        batches[-1].append(g)
        used += e
    return batches


def fit_grid(X, y, Cs, platt='device', max_entries=None, keep_cv_decisions=False, **svc_params):
    """SVC(C=c, **svc_params).fit(X, y) for every c of Cs in one pass -> the fitted models, in the order of Cs.

    X (NumPy rows or a usc.DeviceFeatures) becomes resident once.  The pair problems and the cross-validation sub-problems of every
    cost are solved side by side in one solver call (_lib.SVM.fit with one cost per problem), the held-out decision values of every
    sub-problem come from one launch (_lib.SVM.cv_decision), and Platt's sigmoids of every pair and cost are fitted in one more
    (_lib.svm_sigmoid_train; platt='device').  platt='host' fits them with sigmoid_train in NumPy instead, pair by pair, as SVC.fit
    does.  The solver attributes (support_, dual_coef_, intercept_, n_iter_, ...) are those of the separate fits bit for bit, since
    a problem's solution does not depend on its batch; so are probA_ / probB_ with platt='host'; with platt='device' they differ
    by the order of the float64 sums of the sigmoid fit.  One exception, which SVC.fit shares across its own problems: with
    max_iter=-1 the update cap is max(10^7, 100 x the largest problem), the same for every cost here.

    max_entries: a budget on the rows over all problems of one solver call (its kernel-row scratch is 4 q bytes per entry); the
    costs then go through several calls, a whole cost at a time, and the models do not depend on the split.

    keep_cv_decisions: each model keeps the cross-validation decision values its sigmoids were fitted on as cv_decisions_ (one
    array per pair, in the order of the pair's rows).

    The models share one device handle (and its resident matrix); the handle holds the model evaluate() last used."""
    Cs = [float(c) for c in Cs]
    if not Cs:
        raise ValueError('Cs is empty')
    if any(not c > 0 or not np.isfinite(c) for c in Cs):
        raise ValueError('C <= 0')
    if platt not in PLATT_MODES:
        raise ValueError('platt must be one of %s, not %r' % (list(PLATT_MODES), platt))
    if 'C' in svc_params:
        raise ValueError('the costs come as Cs, not as C')
    models = [SVC(C=c, **svc_params) for c in Cs]
    m0 = models[0]
    X, y, on_device = _check_rows(X, y)
    if m0.kernel not in _lib.SVM_KERNELS:
        raise ValueError('kernel must be one of %s' % sorted(_lib.SVM_KERNELS))
    classes, yenc = _encode_classes(y)
    nc = classes.size
    h = _lib.SVM(m0.device)
    if on_device:
        h.set_data_dev(X.handle)
    else:
        h.set_data(X)
    for m in models:
        m.classes_, m.shape_fit_ = classes, tuple(X.shape)
        m._gamma = 1.0 / X.shape[1] if m.gamma == 'auto' else float(m.gamma)
        m._model_set = m._resident = False
        m._h = h
    kp = m0._kernel()
    groups, pairs, problems, folds = grid_problems(yenc, nc, Cs, m0.probability, m0.random_state)
    n_pairs = len(problems)
    per_cost = [problems + sub for _, sub in folds]
    entries = [sum(rows.size for rows, _ in allp) for allp in per_cost]
    solved = [None] * len(Cs)                   # per cost: (alphas, rho) over problems + sub
    for batch in _cost_batches(entries, max_entries):
        probs = [pr for g in batch for pr in per_cost[g]]
        costs = np.concatenate([np.full(len(per_cost[g]), Cs[g]) for g in batch])
        alphas, rho, updates, outer, _ = h.fit(kp, probs, cost=costs, tol=m0.tol, max_iter=m0.max_iter, q=m0.ws_size)
        at = 0
        for g in batch:
            n = len(per_cost[g])
            solved[g] = (alphas[at:at + n], rho[at:at + n])
            models[g]._solved(updates[at:at + n], outer[at:at + n], n_pairs)
            at += n
    rows_of = h.get_rows if on_device else X.__getitem__
    for m, (alphas, rho) in zip(models, solved):
        m._build_model(rows_of, y.size, groups, pairs, problems, alphas, rho)
        m.probA_ = m.probB_ = np.empty(0)
        m._resident = True
    if m0.probability:
        # every sub-problem of every cost scored on its held-out rows in one launch
        jobs, where = [], []
        decs = [[np.empty(rows.size) for rows, _ in problems] for _ in Cs]
        for g, ((cv, _), (alphas, rho)) in enumerate(zip(folds, solved)):
            for p, held, job in cv:
                if isinstance(job, float):
                    decs[g][p][held] = job
                    continue
                sv, npos, coef = _binary_model(per_cost[g][job][0], per_cost[g][job][1], alphas[job])
                jobs.append((problems[p][0][held], sv, npos, coef, rho[job]))
                where.append((g, p, held))
        for (g, p, held), dec in zip(where, h.cv_decision(kp, jobs)):
            decs[g][p][held] = dec
        if keep_cv_decisions:
            for g, m in enumerate(models):
                m.cv_decisions_ = decs[g]
        if platt == 'device':
            A, B, _ = _lib.svm_sigmoid_train(m0.device, [d for dg in decs for d in dg], [signs for _ in Cs for _, signs in problems])
            for g, m in enumerate(models):
                m.probA_, m.probB_ = A[g * n_pairs:(g + 1) * n_pairs].copy(), B[g * n_pairs:(g + 1) * n_pairs].copy()
        else:
            for g, m in enumerate(models):
                fitted = [sigmoid_train(decs[g][p], signs) for p, (_, signs) in enumerate(problems)]
                m.probA_, m.probB_ = np.array([a for a, _ in fitted], np.float64), np.array([b for _, b in fitted], np.float64)
    return models
