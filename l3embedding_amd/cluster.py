"""Clustering a frozen embedding on the GPU: k-means, agreement with class labels, and bag-of-words file histograms.

`KMeans` clusters float32 rows with Lloyd's iterations on the device (csrc/kmeans.hip): the distances are those of the
nearest-neighbour kernels bit for bit, a row goes to the centroid of the smallest (distance, index), and every float64 sum has one
fixed order, so a fit is a function of its inputs and its seed alone -- two runs give the same bits.  `contingency` counts the rows
of every (cluster, class) pair; `nmi`, `purity` and `adjusted_rand` score such a table on the host in float64.  `file_histograms`
turns each file's frames into counts of "audio words", rows that `classifier` can take as features.  Rows are float32 NumPy arrays or
`usc.DeviceFeatures` (those of `pca.PCA.transform(X, to_device=True)` as they are); there is no silent conversion and no CPU fallback.

Only the squared Euclidean distance is offered.  Seeding is random rows, given centroids, or plain k-means++ with one candidate per
step (scikit-learn's greedy variant, which tries several candidates per step, is out of scope: restarts take its place).  An empty
cluster keeps its previous centroid and is counted in `history_['empty']`; relocating empty clusters is out of scope.
"""
import numpy as np

from . import _lib
from .knn import _rows

INITS = ('k-means++', 'random')
HISTORY_DTYPE = np.dtype([('inertia', np.float64), ('changed', np.int64), ('empty', np.int64)])
TRANSFORM_BLOCK = 65536          # rows of one block of transform()


# ---- scores of a contingency table (host, float64) -------------------------------------------------------------------------------------
def _table(table):
    t = np.asarray(table)
    if t.ndim != 2 or t.dtype.kind not in 'iu' or t.size == 0 or (t.dtype.kind == 'i' and t.min() < 0) or t.sum() < 1:
        raise ValueError('a contingency table is a non-empty 2-d array of counts >= 0 with at least one row counted')
    return t.astype(np.int64)


def _entropy(counts, total):
    c = counts[counts > 0].astype(np.float64)
    return float(-np.sum(c / total * (np.log(c) - np.log(total))))


def nmi(table):
    """normalised mutual information of the two partitions a contingency table counts: MI / mean(H(clusters), H(classes)), the
    arithmetic-mean normalisation (scikit-learn's default); 1.0 when neither partition splits the rows"""
    t = _table(table)
    rows, cols, total = t.sum(axis=1), t.sum(axis=0), float(t.sum())
    if np.count_nonzero(rows) <= 1 and np.count_nonzero(cols) <= 1:
        return 1.0
    i, j = np.nonzero(t)
    cell = t[i, j].astype(np.float64)
    log_outer = np.log(rows[i].astype(np.float64)) + np.log(cols[j].astype(np.float64)) - 2.0 * np.log(total)
    mi = max(0.0, float(np.sum(cell / total * (np.log(cell) - np.log(total) - log_outer))))
    return mi / max(0.5 * (_entropy(rows, total) + _entropy(cols, total)), np.finfo(np.float64).eps)


def purity(table):
    """the share of rows that belong to their cluster's most frequent class"""
    t = _table(table)
    return float(t.max(axis=1).sum()) / float(t.sum())


def adjusted_rand(table):
    """the adjusted Rand index from the table's pair counts (exact integers until the last division)"""
    t = _table(table)
    n = int(t.sum())
    rows, cols = [int(v) for v in t.sum(axis=1)], [int(v) for v in t.sum(axis=0)]
    cells = [(int(v), rows[i], cols[j]) for (i, j), v in np.ndenumerate(t) if v]
    squares = sum(v * v for v, _, _ in cells)
    same_both = squares - n                                    # ordered pairs together in both partitions
    only_class = sum(v * c for v, _, c in cells) - squares     # together in the classes alone
    only_cluster = sum(v * r for v, r, _ in cells) - squares   # together in the clusters alone
    neither = n * n - only_class - only_cluster - squares
    if only_class == 0 and only_cluster == 0:
        return 1.0
    return 2.0 * (same_both * neither - only_cluster * only_class) / (
        (same_both + only_cluster) * (only_cluster + neither) + (same_both + only_class) * (only_class + neither))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _check_seed(random_state):
    if isinstance(random_state, bool) or not isinstance(random_state, (int, np.integer)) or not 0 <= random_state < 2 ** 32:
        raise ValueError('random_state must be an integer seed in [0, 2^32), not %r' % (random_state,))
    return int(random_state)


class KMeans(object):
    """k-means on the GPU.  init: 'k-means++' (plain, one candidate per step), 'random' (rows of a seeded permutation) or a float32
    array (K, D) of centroids.  The two random inits need random_state: nothing here draws from an unseeded generator.  n_init
    restarts run with the seeds RandomState(random_state).randint(2**31 - 1, size=n_init); the lowest final inertia wins, the first
    among equals.  An empty cluster keeps its previous centroid (it is not relocated) and is counted in history_['empty']."""

    def __init__(self, n_clusters, init='k-means++', n_init=8, max_iter=300, random_state=None, device=0):
        self.n_clusters = _lib.kmeans_check_k(n_clusters)
        if isinstance(init, str):
            if init not in INITS:
                raise ValueError('init must be one of %s or a float32 array of centroids, not %r' % (list(INITS), init))
            if random_state is None:
                raise ValueError("init=%r draws rows at random: give random_state (there is no unseeded default)" % init)
            self.init = init
        else:
            c = np.asarray(init)
            if c.dtype != np.float32 or c.ndim != 2 or c.shape[0] != self.n_clusters or c.shape[1] < 1:
                raise ValueError('init centroids must be float32 of shape (%d, D), not %s %s' % (self.n_clusters, c.dtype, c.shape))
            self.init = np.ascontiguousarray(c)
        self.random_state = None if random_state is None else _check_seed(random_state)
        for name, value in (('n_init', n_init), ('max_iter', max_iter)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value < 2 ** 31:
                raise ValueError('%s must be an integer >= 1, not %r' % (name, value))
        self.n_init, self.max_iter, self.device = int(n_init), int(max_iter), int(device)
        self.cluster_centers_ = None
        self._h = None
        self._rows_resident = False

    @classmethod
    def from_centroids(cls, centroids, device=0):
        """a fitted model of given centroids (a codebook read from a file): predict, transform and file_histograms work"""
        self = cls(len(centroids), init=np.asarray(centroids), n_init=1, device=device)
        self.cluster_centers_ = self.init.copy()
        return self

    # ---- the device handle ----
    def close(self):
        """frees the device copy of the rows and centroids; the next call uploads the centroids again"""
        if getattr(self, '_h', None) is not None:
            self._h.close()
            self._h = None
        self._rows_resident = False

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_h'], state['_rows_resident'] = None, False          # a model is pickled with its centroids, not with device memory
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    def _check_fitted(self):
        if self.cluster_centers_ is None:
            raise ValueError('fit comes first')

    def _handle(self):
        """the l3_kmeans handle with the centroids resident; rebuilt on first use after unpickling or close()"""
        self._check_fitted()
        if self._h is None:
            h = _lib.KMeans(self.cluster_centers_.shape[1], self.n_clusters, device=self.device)
            h.set_centroids(self.cluster_centers_)
            self._h = h
        return self._h

    def _seeds(self):
        if not isinstance(self.init, str):
            return [None]
        return [int(s) for s in np.random.RandomState(self.random_state).randint(2 ** 31 - 1, size=self.n_init)]

    def _seed(self, h, seed, n):
        """the centroids of one restart -> the seed rows, or None for given centroids"""
        if not isinstance(self.init, str):
            h.set_centroids(self.init)
            return None
        rng = np.random.RandomState(seed)
        if self.init == 'random':
            chosen = rng.permutation(n)[:self.n_clusters].astype(np.int64)
            h.seed_rows(chosen)
            return chosen
        return h.seed_pp(rng.random_sample(self.n_clusters))

    def fit(self, X):
        """X: (n >= n_clusters, D) float32 rows or a usc.DeviceFeatures.  The rows stay on the device until close()."""
        rows = _rows(X, 'X')
        n, D = rows.shape
        _lib.kmeans_check_k(self.n_clusters, n)
        if not isinstance(self.init, str) and self.init.shape[1] != D:
            raise ValueError('X has %d features per row; the init centroids %d' % (D, self.init.shape[1]))
        self.close()
        h = _lib.KMeans(D, self.n_clusters, device=self.device)
        try:
            h.set_rows(rows)
            best = None
            for r, seed in enumerate(self._seeds()):
                chosen = self._seed(h, seed, n)
                history = h.fit(self.max_iter)
                inertia = h.labels(outputs=())['inertia']
                if best is None or inertia < best['inertia']:
                    best = dict(run=r, inertia=inertia, history=history, chosen=chosen, centroids=h.centroids())
            if best['run'] != r:          # the labels on the device are a later restart's: those of the winner again
                h.set_centroids(best['centroids'])
                h.assign(outputs=())
            got = h.labels()
        except Exception:
            h.close()
            raise
        self._h, self._rows_resident = h, True
        self.cluster_centers_, self.labels_, self.distances_, self.inertia_ = best['centroids'], got['labels'], got['dist'], got['inertia']
        self.n_iter_, self.chosen_, self.best_run_ = len(best['history']), best['chosen'], best['run']
        self.history_ = np.zeros(len(best['history']), HISTORY_DTYPE)
        self.history_['inertia'] = best['history'][:, 0]
        self.history_['changed'] = best['history'][:, 1].astype(np.int64)
        self.history_['empty'] = best['history'][:, 2].astype(np.int64)
        self.shape_fit_ = (n, D)
        return self

    def fit_predict(self, X):
        return self.fit(X).labels_

    def _other(self, X, what):
        rows = _rows(X, what)
        if rows.shape[1] != self.cluster_centers_.shape[1]:
            raise ValueError('%s has %d features per row; expecting %d' % (what, rows.shape[1], self.cluster_centers_.shape[1]))
        return rows

    def predict(self, X):
        """the nearest centroid of every row of X (n) int32; -1 for a row whose distances are all NaN"""
        h = self._handle()
        return h.predict(self._other(X, 'X'), outputs=('labels',))['labels']

    def transform(self, X):
        """(n, n_clusters) float32 squared distances to the centroids, through the nearest-neighbour matrix kernel in blocks of rows"""
        self._check_fitted()
        rows = self._other(X, 'X')
        knn = _lib.KNN(self.cluster_centers_.shape[1], 'sqeuclidean', device=self.device)
        try:
            knn.set_database(self.cluster_centers_)
            if isinstance(rows, _lib.Features):
                knn.set_queries(rows)
                return knn.matrix()
            out = np.empty((rows.shape[0], self.n_clusters), np.float32)
            for lo in range(0, rows.shape[0], TRANSFORM_BLOCK):
                knn.set_queries(rows[lo:lo + TRANSFORM_BLOCK])
                out[lo:lo + TRANSFORM_BLOCK] = knn.matrix()
            return out
        finally:
            knn.close()

    def _labelled(self, X, what):
        """the handle holding the labels that `what` is about -> (handle, predicted?, number of rows)"""
        h = self._handle()
        if X is not None:
            h.predict(self._other(X, 'X'), outputs=())
            return h, True, h.n_predicted
        if not (self._rows_resident and h.assigned):
            raise ValueError('the fitted rows are not on the device (after close() or unpickling): pass X to %s' % what)
        return h, False, h.n

    def contingency(self, y, X=None, num_classes=None):
        """(n_clusters, C) int64: how many rows of each cluster carry each class.  y: a class index in [0, C) per row, C <= 256
        (num_classes None: max + 1).  X None: the fitted rows; else the rows X, assigned to their nearest centroids."""
        y = np.asarray(y).reshape(-1)
        if y.dtype.kind not in 'iu' or y.size < 1 or y.min() < 0:
            raise ValueError('y must hold integer class indices >= 0, one per row')
        C = int(y.max()) + 1 if num_classes is None else int(num_classes)
        if not 1 <= C <= _lib.KMEANS_MAX_CLASSES:
            raise ValueError('at most %d classes, not %d' % (_lib.KMEANS_MAX_CLASSES, C))
        if y.max() >= C:
            raise ValueError('y holds the class %d, outside [0, %d)' % (int(y.max()), C))
        self._check_fitted()
        h, predicted, n = self._labelled(X, 'contingency')
        if y.size != n:
            raise ValueError('y must hold %d class indices, one per row, not %d' % (n, y.size))
        return h.contingency(y, C, predicted=predicted)

    def file_histograms(self, file_idxs, X=None, normalize=False):
        """(F, n_clusters): for the row range [s, e) of every file the number of its rows in each cluster (int32), or with
        normalize their share (float64; a file whose rows all lack a label: zeros).  X None: the fitted rows."""
        self._check_fitted()
        h, predicted, n = self._labelled(X, 'file_histograms')
        hist = h.file_hist(file_idxs, predicted=predicted)
        if not normalize:
            return hist
        hist = hist.astype(np.float64)
        return hist / np.maximum(hist.sum(axis=1, keepdims=True), 1.0)

    def scores(self, y, X=None, num_classes=None):
        """dict of nmi, purity, adjusted_rand and the table they come from"""
        table = self.contingency(y, X=X, num_classes=num_classes)
        return dict(nmi=nmi(table), purity=purity(table), adjusted_rand=adjusted_rand(table), table=table)
