"""Nearest neighbours in embedding space on the GPU: query by example and a training-free classifier.

`NearestNeighbors` answers "which stored rows lie closest to this one" under the squared Euclidean or the cosine distance and
`KNeighborsClassifier` lets the neighbours' labels vote: the usual first look at a frozen self-supervised embedding, with no
optimiser, no seed and no learning rate.  The rows stay on the device (csrc/knn.hip): dot products on the fp32 matrix cores feed the
top-k lists directly and the N x N matrix is never stored.  The order of a list is strict -- the smaller distance first, the smaller
index first among equal distances, a NaN distance never listed -- so every result is a function of the inputs alone.  Rows are
float32 NumPy arrays or `usc.DeviceFeatures`; there is no silent conversion and no CPU fallback.
"""
import numpy as np

from . import _lib
from .usc import DeviceFeatures

METRICS = tuple(sorted(_lib.KNN_METRICS))
EVALUATE_OUTPUTS = ('predict', 'counts', 'file_predict', 'file_counts')


def _rows(X, what):
    """X as what the binding takes: a _lib.Features (of a DeviceFeatures) or a C-contiguous float32 (n, D) array"""
    if isinstance(X, DeviceFeatures):
        return X.handle
    if isinstance(X, _lib.Features):
        return X
    if X is None:
        raise ValueError('%s must not be None' % what)
    X = np.asarray(X)
    if X.dtype != np.float32:
        raise ValueError('%s must be float32 rows, not %s (there is no silent conversion: cast them)' % (what, X.dtype))
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('%s must have shape (n >= 1, D >= 1), not %s' % (what, X.shape))
    return np.ascontiguousarray(X)


class NearestNeighbors(object):
    """Query by example among fitted rows.  fit(X) copies the rows to the device (a DeviceFeatures is copied there, device to
    device -- pca.PCA.transform(X, to_device=True) gives one of reduced or whitened rows); kneighbors gives every query's nearest
    fitted rows."""

    def __init__(self, n_neighbors=5, metric='sqeuclidean', device=0):
        self.n_neighbors = _lib.knn_check_k(n_neighbors)
        if metric not in _lib.KNN_METRICS:
            raise ValueError('metric must be one of %s, not %r' % (list(METRICS), metric))
        self.metric, self.device = metric, int(device)
        self._X = self._labels = None
        self._h = None

    # ---- the fitted rows and the device handle ----
    def _set_fit(self, X, labels=None):
        rows = _rows(X, 'X')
        self.close()
        self.shape_fit_ = tuple(rows.shape)
        self._labels = labels
        if isinstance(X, DeviceFeatures):
            # the handle copies the rows device to device now, and the model keeps a host copy: it outlives the caller's matrix
            # (a search closes the parts of its cut) and is pickled with its rows
            self._X = rows
            self._handle()
            self._X = X.to_host()
        else:
            self._X = rows
        return self

    def with_neighbors(self, n_neighbors):
        """the same fitted rows with another default list size: a copy that shares the host rows and uploads them on first use"""
        other = self.__class__.__new__(self.__class__)
        other.__dict__.update(self.__dict__)
        other._h = None
        other.n_neighbors = _lib.knn_check_k(n_neighbors)
        return other

    def fit(self, X):
        """X: (n, D) float32 rows or a usc.DeviceFeatures"""
        return self._set_fit(X)

    def _check_fitted(self):
        if self._X is None:
            raise ValueError('fit comes first')

    def _handle(self):
        """the l3_knn handle with the fitted rows (and labels) resident; rebuilt on first use after unpickling or close()"""
        self._check_fitted()
        if self._h is None:
            h = _lib.KNN(self.shape_fit_[1], self.metric, device=self.device)
            h.set_database(_rows(self._X, 'X'), self._labels)
            self._h = h
        return self._h

    def close(self):
        """frees the device copy; the next query uploads the fitted rows again"""
        if getattr(self, '_h', None) is not None:
            self._h.close()
            self._h = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_h'] = None          # a model is pickled with its rows (and labels), not with device memory
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    def _k(self, n_neighbors):
        return self.n_neighbors if n_neighbors is None else _lib.knn_check_k(n_neighbors)

    def _set_queries(self, Q, groups_q, groups_fit):
        """the query side of the handle -> (handle, groups of the queries, groups of the fitted rows).  Q None: the fitted rows
        query themselves, each excluded from its own list (its index is its group) unless groups are given."""
        h = self._handle()
        if (groups_q is None) != (groups_fit is None) and not (Q is None and groups_q is None):
            raise ValueError('groups_q and groups_fit are given together or both left None (Q None: groups_fit alone serves both)')
        if Q is None:
            h.query_self()
            if groups_fit is None:
                groups_fit = np.arange(self.shape_fit_[0], dtype=np.int32)
            if groups_q is None:
                groups_q = groups_fit
        else:
            rows = _rows(Q, 'Q')
            if rows.shape[1] != self.shape_fit_[1]:
                raise ValueError('Q has %d features per row; expecting %d' % (rows.shape[1], self.shape_fit_[1]))
            h.set_queries(rows)
        return h, groups_q, groups_fit

    def kneighbors(self, Q=None, n_neighbors=None, groups_q=None, groups_fit=None):
        """-> (dist (n, k) float32, idx (n, k) int32): every query's k nearest fitted rows, nearest first; among equal distances
        the smaller index first.  A fitted row whose group equals the query's is not a candidate (file or clip ids: the frames of
        one file are near-duplicates); a list with fewer than k candidates ends in index -1 and distance +inf.  Q None: the fitted
        rows are the queries and a row is never its own neighbour, even where a twin row ties at distance 0."""
        k = self._k(n_neighbors)
        h, gq, gc = self._set_queries(Q, groups_q, groups_fit)
        idx, dist = h.topk(k, gq, gc)
        return dist, idx

    def distances(self, Q=None, rows=None, cols=None):
        """the distances of the listed pairs (query rows[p], fitted row cols[p]), with the bits they have in a list; rows and cols
        None: the whole (n_queries, n_fit) matrix (small jobs).  Q None: the fitted rows."""
        h, _, _ = self._set_queries(Q, None, None)
        if (rows is None) != (cols is None):
            raise ValueError('rows and cols are given together or both left None')
        return h.matrix() if rows is None else h.list(rows, cols)


def _class_labels(y, n, num_classes):
    """y as n int32 class indices in [0, num_classes) (num_classes None: max + 1) -> (labels, number of classes)"""
    y = np.asarray(y).reshape(-1)
    if y.size != n or y.dtype.kind not in 'iu':
        raise ValueError('y must hold %d integer class indices, one per row' % n)
    if y.min() < 0:
        raise ValueError('y must hold class indices >= 0; found %d' % int(y.min()))
    C = int(y.max()) + 1 if num_classes is None else int(num_classes)
    if not 1 <= C <= _lib.KNN_MAX_CLASSES:
        raise ValueError('num_classes must be in [1, %d], not %d' % (_lib.KNN_MAX_CLASSES, C))
    if y.max() >= C:
        raise ValueError('y holds the label %d, outside [0, %d)' % (int(y.max()), C))
    return np.ascontiguousarray(y, np.int32), C


class KNeighborsClassifier(NearestNeighbors):
    """k-nearest-neighbour classifier on frozen features: every neighbour has one vote, the class of the most votes wins and the
    lowest class among equals; a query without neighbours is class -1.  Labels are class indices in [0, num_classes)."""

    def __init__(self, n_neighbors=5, metric='sqeuclidean', num_classes=None, device=0):
        super(KNeighborsClassifier, self).__init__(n_neighbors=n_neighbors, metric=metric, device=device)
        if num_classes is not None and not 1 <= int(num_classes) <= _lib.KNN_MAX_CLASSES:
            raise ValueError('num_classes must be in [1, %d], not %r' % (_lib.KNN_MAX_CLASSES, num_classes))
        self.num_classes = None if num_classes is None else int(num_classes)
        self._groups = None

    def fit(self, X, y, groups=None):
        """X: (n, D) float32 rows or a usc.DeviceFeatures; y: n class indices; groups: n integers (file or clip ids) that
        evaluate(X=None) and evaluate(..., groups=...) exclude by, or None"""
        n = _rows(X, 'X').shape[0]
        labels, C = _class_labels(y, n, self.num_classes)
        self._groups = None if groups is None else _lib._group32(groups, 'groups', n, 'fitted row')
        self.classes_ = np.arange(C)
        return self._set_fit(X, labels)

    def evaluate(self, X=None, y=None, file_idxs=None, ks=None, groups=None, outputs=('predict',)):
        """One query at max(ks) on the GPU over X (NumPy rows or a usc.DeviceFeatures) -> dict of what `outputs` names, nothing
        else being downloaded: 'predict' (n) classes, 'counts' (n, C) int32 votes per class, and for the row ranges [s, e) of
        file_idxs 'file_counts' (F, C), the sum of the frames' votes, and 'file_predict' (F), its class of the most votes.  That
        sum equals the mean of the frames' vote fractions (predict_proba) times its constant number of votes per frame whenever
        every list is full, so both choose the same class; integers keep the choice exact and free of an order of additions.
        ks (ascending list sizes <= 64, at most 8): every output gets a leading axis over ks -- the first k' entries of a sorted
        k-list are the k'-list, so one query serves every size; ks None: n_neighbors.
        X None: the fitted rows, each row leaving itself out (leave-one-out), or its whole group when fit had groups.  groups: the
        queries' groups, excluded against fit's.  y is accepted for the shape of SVC.evaluate and not used."""
        outputs = tuple(outputs)
        unknown = set(outputs) - set(EVALUATE_OUTPUTS)
        if unknown or not outputs:
            raise ValueError('unknown outputs %s; choose from %s' % (sorted(unknown), list(EVALUATE_OUTPUTS)))
        self._check_fitted()
        sizes = [self.n_neighbors] if ks is None else list(ks)
        k = _lib.knn_check_k(max(sizes) if sizes and all(isinstance(s, (int, np.integer)) for s in sizes) else 0)
        sizes = _lib.knn_check_sizes(sizes, k)
        if groups is not None and (X is None or self._groups is None):
            raise ValueError('groups go with rows X and a fit that had groups')
        if X is not None and groups is None and self._groups is not None:
            groups_fit = None          # queries from elsewhere without groups: nothing is excluded
        else:
            groups_fit = self._groups
        h, gq, gc = self._set_queries(X, groups, groups_fit)
        names = {'predict': 'pred', 'counts': 'counts', 'file_predict': 'file_pred', 'file_counts': 'file_counts'}
        got = h.vote(k, sizes, len(self.classes_), gq, gc, file_idxs=file_idxs, outputs=[names[o] for o in outputs])
        out = {}
        for o in outputs:
            a = np.moveaxis(got[names[o]], 1, 0)          # (n, S, ...) -> (S, n, ...)
            out[o] = np.ascontiguousarray(a if ks is not None else a[0])
        return out

    def predict(self, X):
        return self.evaluate(X)['predict']

    def predict_proba(self, X):
        """(n, C) float64 vote fractions: the counts divided by the list's length (a query without neighbours: zeros)"""
        counts = self.evaluate(X, outputs=('counts',))['counts'].astype(np.float64)
        return counts / np.maximum(counts.sum(axis=1, keepdims=True), 1.0)
