"""The reference's random-forest sound classifier (classifier/train.py:169-227): sklearn.ensemble.RandomForestClassifier of
scikit-learn 0.19 with the arguments train_rf gives it (n_estimators, random_state; everything else at its default: Gini, bootstrap,
max_features sqrt(D), trees grown until the leaves are pure), trained and evaluated on the GPU through the l3_forest handle of
libl3hip (csrc/forest.hip).

The forest is grown level by level from histograms: per feature at most 255 float32 cuts from a sample of
bin_sample rows, a uint8 bin code per value, all trees advancing one level per group of launches, integer class counts and one float64
formula for a split's worth.  Here are the draws a fit needs from NumPy (the tree seeds, each tree's bootstrap multiplicities, the
rows of the cut sample) and sklearn's shell: fit / predict / predict_proba, classes_, estimators_ and pickling.

Beyond sklearn's interface, for the parameter search over n_estimators (classifier.train_rf_search): a forest
of n trees is the first n trees of a larger one fitted with the same random_state (the cuts depend on the data and random_state
alone, a tree on the cuts, its seed and its bootstrap, and RandomState(random_state).randint(2^31 - 1, size=n) is a prefix of the
same call with a larger size).  evaluate() scores rows by several such prefixes in one pass on the GPU (l3_forest_score: predictions,
hits, probabilities, per-file means, each tree walked once per row, bit for bit what predict_proba gives for each prefix), and
prefix(n) is the fitted classifier of the first n trees.

Out-of-bag scores: with oob_score=True fit also sets oob_score_ and oob_decision_function_ by sklearn 0.19's
_set_oob_score rule, and oob_evaluate() gives the out-of-bag predictions, hits, sums and decisions of the training rows at several
forest sizes in one pass on the GPU (l3_forest_oob: each row scored by the trees whose bootstrap missed it, the masks built on the
device from the multiplicities the fit drew).  A prefix's out-of-bag values are those of a separate fit of its size, bit for bit.

Deviations from sklearn 0.19, all deliberate:
  * a split is searched among at most 255 cuts per feature (sklearn tries every midpoint of the node's own values), so the trees are
    not sklearn's; they are judged against sklearn's seed-to-seed spread (tests/golden/make_forest_golden.py) and are equal, node for
    node, to the NumPy restatement of this algorithm in tests/forest_ref.py;
  * the bootstrap of tree t is np.bincount(RandomState(seed_t).randint(0, n, n)) with seed_t from RandomState(random_state) as
    sklearn draws them, but a node's max_features features come from Floyd's subset sampling driven by a counter-based mixer of
    (seed_t, node, draw) on the device (sklearn walks its private rand_r stream through a Fisher-Yates shuffle);
  * sklearn keeps drawing past max_features until it has found one feature that is not constant in the node; here a node draws exactly
    max_features features, and one that finds no valid split among them becomes a leaf;
  * among equally good splits the earlier draw wins, then the lower cut (sklearn: the first it meets in its own order);
  * estimators_ holds the trees as flat arrays (_lib.FOREST_TREE_ARRAYS), not DecisionTreeClassifier objects;
  * oob_score_ and oob_decision_function_ are not pickled and a prefix does not carry the larger forest's: they belong to the rows
    of the fit, and oob_evaluate(X=those rows) gives them again (sklearn pickles both);
  * class_weight, sample weights, min_weight_fraction_leaf, max_leaf_nodes, min_impurity_decrease, warm_start and criteria
    other than Gini are not built; at most _lib.FOREST_MAX_CLASSES classes.
"""
import warnings

import numpy as np

from . import _lib
from .usc import DeviceFeatures


# evaluate()'s X for "the rows this forest was fitted on": they are still on the GPU, in the handle the fit left them in
FITTED_ROWS = object()
EVALUATE_OUTPUTS = ('predict', 'correct', 'proba', 'file_mean', 'file_predict')
_SCORE_NAMES = {'predict': 'pred', 'correct': 'correct', 'proba': 'proba', 'file_mean': 'file_mean', 'file_predict': 'file_pred'}
OOB_OUTPUTS = ('predict', 'correct', 'sums', 'n_oob', 'decision')
_OOB_NAMES = {'predict': 'pred', 'correct': 'correct', 'sums': 'sums', 'n_oob': 'n_oob', 'decision': 'sums'}
_OOB_ATTRIBUTES = ('oob_score_', 'oob_decision_function_')          # of one fit's rows: neither pickled nor handed to a prefix


def tree_seeds(random_state, n_estimators):
    """sklearn's per-tree seeds (ensemble/base.py _set_random_states: randint(MAX_INT) per estimator)"""
    return np.random.RandomState(random_state).randint(np.iinfo(np.int32).max, size=n_estimators).astype(np.int64)


def bootstrap_counts(seeds, n):
    """(n_trees, n) uint16: how often each row occurs in each tree's bootstrap sample (sklearn's _generate_sample_indices)"""
    boot = np.empty((len(seeds), n), np.uint16)
    for t, seed in enumerate(seeds):
        counts = np.bincount(np.random.RandomState(int(seed)).randint(0, n, n), minlength=n)
        if counts.max() > np.iinfo(np.uint16).max:
            raise ValueError('a row occurs %d times in a bootstrap sample; at most 65535 are built' % counts.max())
        boot[t] = counts
    return boot


def bin_sample_rows(random_state, n, bin_sample):
    """the rows the cuts are taken from: None for all of them, else bin_sample of them drawn without replacement, ascending"""
    if n <= bin_sample:
        return None
    return np.sort(np.random.RandomState(random_state).choice(n, bin_sample, replace=False)).astype(np.int32)


def resolve_max_features(max_features, D):
    """sklearn 0.19's reading of max_features for a classifier -> the number of features drawn per node"""
    if max_features is None:
        return D
    if isinstance(max_features, str):
        if max_features in ('sqrt', 'auto'):
            return max(1, int(np.sqrt(D)))
        if max_features == 'log2':
            return max(1, int(np.log2(D)))
        raise ValueError("max_features must be 'sqrt', 'auto', 'log2', None, an int or a float, not %r" % (max_features,))
    if isinstance(max_features, (int, np.integer)):
        k = int(max_features)
    else:
        k = max(1, int(float(max_features) * D)) if max_features > 0 else 0
    if not 1 <= k <= D:
        raise ValueError('max_features must be in (0, n_features]')
    return k


def oob_decision(sums):
    """sklearn 0.19's _set_oob_score normalisation of one forest's out-of-bag sums (n, C): each row over its own total, NaN where no
    tree left the row out (then the warning sklearn gives)"""
    if (sums.sum(axis=1) == 0).any():
        warnings.warn('Some inputs do not have OOB scores. This probably means too few trees were used to compute any reliable oob '
                      'estimates.')
    with np.errstate(invalid='ignore', divide='ignore'):
        return sums / sums.sum(axis=1)[:, None]


class RandomForestClassifier(object):
    """sklearn 0.19's RandomForestClassifier(n_estimators, random_state, oob_score) on the GPU: fit / predict / predict_proba,
    classes_, estimators_ (the trees as the flat arrays of _lib.FOREST_TREE_ARRAYS), and with oob_score=True oob_score_ and
    oob_decision_function_.  The fitted model pickles without its device handle and uploads its trees again on first use.
    wide_min_rows: the node size from which the search takes a workgroup per (node, feature) instead of a wave per node (0: the
    library's default); the trees do not depend on it."""

    def __init__(self, n_estimators=100, random_state=None, max_depth=None, min_samples_split=2, min_samples_leaf=1,
                 max_features='sqrt', bin_sample=4096, device=0, wide_min_rows=0, oob_score=False):
        self.n_estimators, self.random_state, self.max_depth = n_estimators, random_state, max_depth
        self.min_samples_split, self.min_samples_leaf, self.max_features = min_samples_split, min_samples_leaf, max_features
        self.bin_sample, self.device, self.wide_min_rows, self.oob_score = bin_sample, device, wide_min_rows, oob_score
        self._h = None
        self._resident = False
        self._fitted_rows = 0          # rows of the fit's matrix while this model's handle still holds it (evaluate(FITTED_ROWS))

    # pickling: everything but the device handle
    def __getstate__(self):
        state = dict(self.__dict__)
        state['_h'] = None
        state['_resident'] = False
        state['_fitted_rows'] = 0
        for k in _OOB_ATTRIBUTES:
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault('_fitted_rows', 0)          # a model pickled before evaluate() existed
        self.__dict__.setdefault('oob_score', False)         # or before oob_score did

    def _handle(self):
        if self._h is None:
            self._h = _lib.Forest(self.device)
            self._resident = False
            self._fitted_rows = 0
        return self._h

    def fit(self, X, y):
        """X: NumPy rows, or a usc.DeviceFeatures, which is copied on the device (no download; the fit sees the same bits)"""
        on_device = isinstance(X, DeviceFeatures)
        if not on_device:
            X = np.ascontiguousarray(X, np.float32)
        y = np.asarray(y).reshape(-1)
        if len(X.shape) != 2 or X.shape[0] != y.size or y.size == 0:
            raise ValueError('X must be (n_samples, n_features) with one label per row')
        n, D = int(X.shape[0]), int(X.shape[1])
        if int(self.n_estimators) < 1:
            raise ValueError('n_estimators must be at least 1')
        if self.max_depth is not None and int(self.max_depth) < 1:
            raise ValueError('max_depth must be at least 1, or None')
        if int(self.min_samples_split) < 2 or int(self.min_samples_leaf) < 1:
            raise ValueError('min_samples_split must be at least 2 and min_samples_leaf at least 1 (row counts)')
        if not 1 <= int(self.bin_sample) <= _lib.FOREST_MAX_BIN_SAMPLE:
            raise ValueError('bin_sample must be in [1, %d]' % _lib.FOREST_MAX_BIN_SAMPLE)
        classes, yenc = np.unique(y, return_inverse=True)
        if classes.size > _lib.FOREST_MAX_CLASSES:
            raise ValueError('at most %d classes are built' % _lib.FOREST_MAX_CLASSES)
        k = resolve_max_features(self.max_features, D)
        if k > _lib.FOREST_MAX_DRAWS:
            raise ValueError('max_features gives %d features per node; at most %d are built' % (k, _lib.FOREST_MAX_DRAWS))
        seeds = tree_seeds(self.random_state, int(self.n_estimators))
        boot = bootstrap_counts(seeds, n)
        rows = bin_sample_rows(self.random_state, n, int(self.bin_sample))
        h = self._handle()
        self._resident = False
        self._fitted_rows = 0
        if on_device:
            h.set_data_dev(X.handle)
        else:
            h.set_data(X)
        h.fit(yenc, boot, seeds, classes.size, k, max_depth=self.max_depth or 0, min_samples_split=self.min_samples_split,
              min_samples_leaf=self.min_samples_leaf, bin_rows=rows, wide_min_rows=self.wide_min_rows)
        self.classes_, self.n_classes_, self.n_features_, self.max_features_ = classes, classes.size, D, k
        self.estimators_ = h.trees()
        self.level_stats_ = h.level_stats()
        self._resident = True
        self._fitted_rows = n
        for k in _OOB_ATTRIBUTES:
            self.__dict__.pop(k, None)
        if self.oob_score:          # sklearn 0.19's _set_oob_score, on the rows and the multiplicities of this fit
            got = h.oob(boot, outputs=('pred', 'sums'))
            self.oob_decision_function_ = oob_decision(got['sums'][0])
            self.oob_score_ = np.mean(yenc == got['pred'][0])
        return self

    def _check_fitted(self):
        if not hasattr(self, 'estimators_'):
            raise ValueError('This RandomForestClassifier instance is not fitted yet')

    def _ensure_model(self):
        """the handle with this model's trees resident: as the fit left them, or uploaded again after unpickling"""
        h = self._handle()
        if not self._resident:
            h.set_trees(self.estimators_, self.n_features_)
            self._resident = True
        return h

    def _class_indices(self, y, n):
        """the n labels y (classes_ values, every one of them known to the forest) as indices into classes_"""
        y = np.asarray(y).reshape(-1)
        if y.size != n:
            raise ValueError('one label per row')
        labels = np.searchsorted(self.classes_, y).clip(max=self.classes_.size - 1)
        if not np.array_equal(self.classes_[labels], y):
            raise ValueError('y holds a label the forest was not fitted on')
        return labels

    def predict_proba(self, X):
        """(n, n_classes) float64: the mean over the trees of the class fractions of the leaf each row falls into"""
        self._check_fitted()
        on_device = isinstance(X, DeviceFeatures)
        if not on_device:
            X = np.ascontiguousarray(X, np.float32)
        if len(X.shape) != 2 or X.shape[1] != self.n_features_:
            raise ValueError('X has %s features per sample; expecting %d' % (tuple(X.shape[1:]), self.n_features_))
        if X.shape[0] == 0:
            raise ValueError('no rows to predict')
        h = self._ensure_model()
        return h.predict_proba_dev(X.handle) if on_device else h.predict_proba(X)

    def predict(self, X):
        proba = self.predict_proba(X)
        return self.classes_[np.argmax(proba, axis=1)]

    def evaluate(self, X, y=None, file_idxs=None, prefixes=None, outputs=('predict',), chunk_rows=0, stage_bytes=0):
        """One scoring pass on the GPU over X by the forests of the first prefixes[g] trees, every tree walked once per row -> dict
        of what `outputs` names (EVALUATE_OUTPUTS), each with the leading axis G = len(prefixes); without prefixes the whole forest,
        G = 1.  X: NumPy rows, a usc.DeviceFeatures, or FITTED_ROWS (the rows of the last fit, as long as this model's handle still
        holds them: not after pickling).  prefixes: distinct forest sizes in [1, n_estimators], ascending.
        'predict' (G, n): classes_ values; 'correct' (G): the rows predicted as y (classes_ values, every one of them known to the
        forest); 'proba' (G, n, C): predict_proba of each prefix, bit for bit; 'file_mean' (G, F, C): the mean of the probabilities of
        the rows [s, e) of each file_idxs entry, added in row order as NumPy's mean(axis=0) adds them, and 'file_predict' (G, F) its
        arg-max as classes_ values.  chunk_rows, stage_bytes: _lib.Forest.score's, for tests; they change no bit."""
        self._check_fitted()
        outputs = tuple(outputs)
        unknown = set(outputs) - set(EVALUATE_OUTPUTS)
        if unknown:
            raise ValueError('unknown outputs %s; choose from %s' % (sorted(unknown), list(EVALUATE_OUTPUTS)))
        by_file = 'file_mean' in outputs or 'file_predict' in outputs
        if by_file and file_idxs is None:
            raise ValueError("'file_mean' and 'file_predict' need file_idxs")
        if 'correct' in outputs and y is None:
            raise ValueError("'correct' needs y")
        if X is FITTED_ROWS:
            if not self._fitted_rows or self._h is None:
                raise ValueError('the rows of the fit are no longer on the GPU: pass them to evaluate')
            rows, n = dict(resident=True), self._fitted_rows
        else:
            on_device = isinstance(X, DeviceFeatures)
            if not on_device:
                X = np.ascontiguousarray(X, np.float32)
            if len(X.shape) != 2 or X.shape[1] != self.n_features_:
                raise ValueError('X has %s features per sample; expecting %d' % (tuple(X.shape[1:]), self.n_features_))
            if X.shape[0] == 0:
                raise ValueError('no rows to score')
            rows, n = (dict(feat=X.handle) if on_device else dict(X=X)), int(X.shape[0])
        labels = self._class_indices(y, n) if 'correct' in outputs else None
        h = self._ensure_model()
        got = h.score(prefixes=prefixes, labels=labels, files=file_idxs if by_file else None,
                      outputs=tuple(_SCORE_NAMES[k] for k in outputs), chunk_rows=chunk_rows, stage_bytes=stage_bytes, **rows)
        out = {k: got[_SCORE_NAMES[k]] for k in outputs}
        for k in ('predict', 'file_predict'):
            if k in out:
                out[k] = self.classes_[out[k]]
        return out

    def oob_evaluate(self, y=None, prefixes=None, outputs=('correct',), X=FITTED_ROWS, chunk_rows=0, stage_bytes=0):
        """One out-of-bag pass on the GPU over the rows of the fit by the forests of the first prefixes[g] trees: every row is scored
        by the trees whose bootstrap sample missed it, each of them walked once -> dict of what `outputs` names (OOB_OUTPUTS), each
        with the leading axis G = len(prefixes); without prefixes the whole forest, G = 1.  X: FITTED_ROWS (the rows where the fit
        left them, as in evaluate), or the same rows again as NumPy rows or a usc.DeviceFeatures (after unpickling; they replace the
        handle's matrix, so FITTED_ROWS is no longer served afterwards).  The multiplicities are drawn again from random_state, an int.
        'sums' (G, n, C): the leaves' class fractions added in tree order over the row's out-of-bag trees; 'n_oob' (G, n): their
        number; 'predict' (G, n): classes_[argmax(sums)], classes_[0] for a row without such a tree; 'correct' (G): the rows
        predicted as y; 'decision' (G, n, C): oob_decision of the sums, what a fit of prefixes[g] trees with oob_score=True leaves in
        oob_decision_function_ (NaN rows and the warning included), bit for bit.  chunk_rows, stage_bytes: evaluate's."""
        self._check_fitted()
        outputs = tuple(outputs)
        unknown = set(outputs) - set(OOB_OUTPUTS)
        if unknown:
            raise ValueError('unknown outputs %s; choose from %s' % (sorted(unknown), list(OOB_OUTPUTS)))
        if 'correct' in outputs and y is None:
            raise ValueError("'correct' needs y")
        if isinstance(self.random_state, bool) or not isinstance(self.random_state, (int, np.integer)):
            raise ValueError('the bootstrap samples can be drawn again only from an int random_state, not %r' % (self.random_state,))
        if X is FITTED_ROWS:
            if not self._fitted_rows or self._h is None:
                raise ValueError('the rows of the fit are no longer on the GPU: pass them to oob_evaluate')
            h, n = self._ensure_model(), self._fitted_rows
        else:
            on_device = isinstance(X, DeviceFeatures)
            if not on_device:
                X = np.ascontiguousarray(X, np.float32)
            if len(X.shape) != 2 or X.shape[1] != self.n_features_:
                raise ValueError('X has %s features per sample; expecting %d' % (tuple(X.shape[1:]), self.n_features_))
            if X.shape[0] == 0:
                raise ValueError('no rows to score')
            h, n = self._ensure_model(), int(X.shape[0])
            self._fitted_rows = 0
            if on_device:
                h.set_data_dev(X.handle)
            else:
                h.set_data(X)
        labels = None
        if 'correct' in outputs:
            labels = self._class_indices(y, n)
        boot = bootstrap_counts(tree_seeds(self.random_state, int(self.n_estimators)), n)
        got = h.oob(boot, prefixes=prefixes, labels=labels, outputs=tuple(sorted({_OOB_NAMES[k] for k in outputs})),
                    chunk_rows=chunk_rows, stage_bytes=stage_bytes)
        out = {k: got[_OOB_NAMES[k]] for k in outputs}
        if 'predict' in out:
            out['predict'] = self.classes_[out['predict']]
        if 'decision' in out:
            out['decision'] = np.stack([oob_decision(s) for s in got['sums']])
        return out

    def prefix(self, n):
        """the fitted classifier of this forest's first n trees, n_estimators = n: what fit gives with n_estimators=n and everything
        else equal (but for oob_score_ and oob_decision_function_: this forest's are not the prefix's, oob_evaluate gives those).
        Its estimators_ are views of this forest's arrays; it has no handle and uploads its trees on first use."""
        self._check_fitted()
        n = int(n)
        if not 1 <= n <= int(self.n_estimators):
            raise ValueError('a prefix holds between 1 and n_estimators = %d trees' % self.n_estimators)
        part = type(self).__new__(type(self))
        part.__dict__.update(self.__getstate__(), n_estimators=n)
        part.__dict__.pop('level_stats_', None)          # the course of the larger fit
        nodes = int(self.estimators_['tree_off'][n])
        part.estimators_ = {k: v[:n + 1] if k == 'tree_off' else v[:nodes] for k, v in self.estimators_.items()}
        return part
