"""Two-dimensional maps of a frozen embedding on the GPU: t-SNE over the nearest-neighbour lists.

`TSNE` lays n embedding rows out in the plane so that rows that are neighbours in the embedding stay neighbours in the map (van der
Maaten and Hinton's t-SNE, the plot *Look, Listen and Learn* shows of its audio features).  The neighbours come from the k-NN handle
(csrc/knn.hip), the conditional probabilities are calibrated on the device to the perplexity, they are symmetrised once on the host,
and the gradient loop runs on the device (csrc/tsne.hip) with no read-back but a KL record every `kl_every` iterations.  The
repulsive term is the exact sum over all pairs -- no tree, no grid and no approximation parameter -- in one fixed order, so a fit is a
function of its inputs and its seed alone: two runs give the same bits.  Rows are float32 NumPy arrays or `usc.DeviceFeatures`; there
is no silent conversion and no CPU fallback.

The map is 2-D only.  The neighbour lists hold at most 64 entries, so the perplexity is at most 21 (scikit-learn's rule asks for
floor(3 perplexity + 1) neighbours).  PCA initialisation is out of scope: `init` is 'random' (seeded) or an array.
"""
import numpy as np

from . import _lib
from .knn import _rows

HISTORY_DTYPE = np.dtype([('iteration', np.int64), ('kl', np.float64), ('z', np.float64)])
MAX_PERPLEXITY = (_lib.KNN_TOPK_MAX - 1) / 3.0          # 21: floor(3 * 21 + 1) = 64


def n_neighbors_for(perplexity, n):
    """scikit-learn's rule: min(n - 1, floor(3 perplexity + 1)) neighbours; ValueError when they do not fit a neighbour list or the
    perplexity does not fit them"""
    if isinstance(perplexity, bool) or not isinstance(perplexity, (int, float, np.integer, np.floating)) or not perplexity > 1:
        raise ValueError('perplexity must be a number > 1, not %r' % (perplexity,))
    want = int(3.0 * perplexity + 1.0)
    if want > _lib.KNN_TOPK_MAX:
        raise ValueError('perplexity %g asks for %d neighbours per row, but a neighbour list holds at most %d: the perplexity is at most %g'
                         % (perplexity, want, _lib.KNN_TOPK_MAX, MAX_PERPLEXITY))
    k = min(int(n) - 1, want)
    if k < 2 or not perplexity < k:
        raise ValueError('perplexity %g needs more than %d rows: it must lie below the %d neighbours of a row' % (perplexity, n, max(k, 0)))
    return k


def joint_affinities(idx, p):
    """The symmetric P of t-SNE from neighbour lists: idx (n, k) integer (a row's neighbours: distinct, not itself, in [0, n)), p (n, k)
    conditional probabilities p_{j|i}.  P_ij = (p_{j|i} + p_{i|j}) / 2n in float64 (a missing direction counts 0) -> CSR (indptr int64,
    cols int32, vals float32) sorted by (row, column).  NumPy only; once per fit."""
    idx, p = np.asarray(idx), np.asarray(p, np.float64)
    if idx.ndim != 2 or idx.dtype.kind not in 'iu' or p.shape != idx.shape or idx.shape[0] < 1:
        raise ValueError('idx and p must be two (n, k) arrays, neighbour indices and probabilities')
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = idx.reshape(-1).astype(np.int64)
    if k and (cols.min() < 0 or cols.max() >= n):
        raise ValueError('a neighbour index lies outside the %d rows' % n)
    if np.any(cols == rows):
        raise ValueError('a row lists itself as a neighbour')
    key = np.concatenate([rows * n + cols, cols * n + rows])          # each entry once as (i, j) and once as (j, i)
    val = np.concatenate([p.reshape(-1), p.reshape(-1)])
    order = np.argsort(key, kind='stable')
    key, val = key[order], val[order]
    first = np.r_[True, key[1:] != key[:-1]] if len(key) else np.zeros(0, bool)
    starts = np.flatnonzero(first)
    counts = np.diff(np.r_[starts, len(key)])
    if np.any(counts > 2):
        raise ValueError('a row lists the same neighbour twice')
    total = val[starts].copy()
    two = counts == 2
    total[two] = total[two] + val[starts[two] + 1]
    ukey = key[starts]
    vals = (total / (2.0 * n)).astype(np.float32)
    r = ukey // n
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=indptr[1:])
    return indptr, (ukey - r * n).astype(np.int32), vals


def _check_seed(random_state):
    if isinstance(random_state, bool) or not isinstance(random_state, (int, np.integer)) or not 0 <= random_state < 2 ** 32:
        raise ValueError('random_state must be an integer seed in [0, 2^32), not %r' % (random_state,))
    return int(random_state)


class TSNE(object):
    """t-SNE on the GPU.  perplexity in (1, 21]; n_iter iterations of which the first exaggeration_iter multiply P by
    early_exaggeration and use momentum[0], the others momentum[1]; learning_rate a number or 'auto' (scikit-learn's max(n /
    early_exaggeration / 4, 50)); init 'random' (1e-4 * RandomState(random_state).standard_normal((n, 2)), narrowed to float32; it
    needs random_state: nothing is drawn unseeded) or a float32 (n, 2) array.  After fit: embedding_ (n, 2) float32, kl_divergence_
    (the last record's), history_ (iteration, kl, z records) and n_neighbors_."""

    def __init__(self, perplexity=20.0, n_iter=1000, early_exaggeration=12.0, exaggeration_iter=250, learning_rate='auto', momentum=(0.5, 0.8),
                 metric='sqeuclidean', init='random', random_state=None, kl_every=50, device=0):
        n_neighbors_for(perplexity, _lib.KNN_TOPK_MAX + 1)          # the range of the perplexity alone
        self.perplexity = float(perplexity)
        for name, value, low in (('n_iter', n_iter, 1), ('exaggeration_iter', exaggeration_iter, 0), ('kl_every', kl_every, 1)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not low <= value < 2 ** 31:
                raise ValueError('%s must be an integer >= %d, not %r' % (name, low, value))
        if exaggeration_iter > n_iter:
            raise ValueError('exaggeration_iter = %d exceeds n_iter = %d' % (exaggeration_iter, n_iter))
        self.n_iter, self.exaggeration_iter, self.kl_every = int(n_iter), int(exaggeration_iter), int(kl_every)
        if not (isinstance(early_exaggeration, (int, float, np.integer, np.floating)) and np.isfinite(early_exaggeration) and early_exaggeration >= 1):
            raise ValueError('early_exaggeration must be a number >= 1, not %r' % (early_exaggeration,))
        self.early_exaggeration = float(early_exaggeration)
        if isinstance(learning_rate, str):
            if learning_rate != 'auto':
                raise ValueError("learning_rate must be a number > 0 or 'auto', not %r" % (learning_rate,))
        elif not (isinstance(learning_rate, (int, float, np.integer, np.floating)) and np.isfinite(learning_rate) and learning_rate > 0):
            raise ValueError("learning_rate must be a number > 0 or 'auto', not %r" % (learning_rate,))
        self.learning_rate = learning_rate
        momentum = tuple(momentum) if np.ndim(momentum) == 1 else ()
        if len(momentum) != 2 or not all(0 <= float(m) < 1 for m in momentum):
            raise ValueError('momentum must be two numbers in [0, 1): the exaggerated and the plain phase')
        self.momentum = (float(momentum[0]), float(momentum[1]))
        if metric not in _lib.KNN_METRICS:
            raise ValueError('metric must be one of %s, not %r' % (sorted(_lib.KNN_METRICS), metric))
        self.metric = metric
        if isinstance(init, str):
            if init != 'random':
                raise ValueError("init must be 'random' or a float32 (n, 2) array, not %r (PCA initialisation is out of scope: pass its array)" % (init,))
            if random_state is None:
                raise ValueError("init='random' draws the map at random: give random_state (there is no unseeded default)")
            self.init = init
        else:
            y = np.asarray(init)
            if y.dtype != np.float32 or y.ndim != 2 or y.shape[1] != 2:
                raise ValueError('an init array must be float32 of shape (n, 2), not %s %s' % (y.dtype, y.shape))
            self.init = np.ascontiguousarray(y)
        self.random_state = None if random_state is None else _check_seed(random_state)
        self.device = int(device)
        self.embedding_ = None
        self._h = None

    # ---- the device handle ----
    def close(self):
        """frees the device copy of the map and of P"""
        if getattr(self, '_h', None) is not None:
            self._h.close()
            self._h = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_h'] = None          # a model is pickled with its map, not with device memory
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    # ---- the pieces of a fit ----
    def learning_rate_for(self, n):
        if self.learning_rate == 'auto':
            return max(n / self.early_exaggeration / 4.0, 50.0)
        return float(self.learning_rate)

    def initial_map(self, n):
        if isinstance(self.init, str):
            return (1e-4 * np.random.RandomState(self.random_state).standard_normal((n, 2))).astype(np.float32)
        if self.init.shape[0] != n:
            raise ValueError('the init array holds %d points, the data %d rows' % (self.init.shape[0], n))
        return self.init

    def neighbors(self, X):
        """(idx (n, k) int32, dist (n, k) float32): every row's k = n_neighbors_for(perplexity, n) nearest other rows, from the k-NN
        handle: a self query with every row its own group"""
        rows = _rows(X, 'X')
        n, D = rows.shape
        k = n_neighbors_for(self.perplexity, n)
        knn = _lib.KNN(D, self.metric, device=self.device)
        try:
            knn.set_database(rows)
            knn.query_self()
            own = np.arange(n, dtype=np.int32)
            return knn.topk(k, group_q=own, group_c=own)
        finally:
            knn.close()

    def fit(self, X):
        """X: (n, D) float32 rows or a usc.DeviceFeatures (the usual 50-dimensional input: pca.PCA(50).fit_transform(X, to_device=True))"""
        idx, dist = self.neighbors(X)
        return self.fit_neighbors(idx, dist)

    def fit_neighbors(self, idx, dist):
        """neighbour lists from anywhere: idx (n, k) integer, dist (n, k) float32 (squared distances for the usual Gaussian), 2 <= k <=
        64, perplexity < k"""
        idx, dist = np.asarray(idx), np.asarray(dist)
        if idx.ndim != 2 or idx.dtype.kind not in 'iu' or dist.shape != idx.shape:
            raise ValueError('idx and dist must be two (n, k) arrays, neighbour indices and distances')
        if dist.dtype != np.float32:
            raise ValueError('dist must be float32, not %s (there is no silent conversion)' % dist.dtype)
        n, k = idx.shape
        _lib.tsne_check_n(n)
        _lib.tsne_check_perplexity(self.perplexity, k)
        y0 = self.initial_map(n)
        lr = self.learning_rate_for(n)
        p, beta, bad = _lib.op_tsne_conditional(dist, self.perplexity, device=self.device)
        if bad:
            raise ValueError('%d rows have a neighbour distance that is NaN or infinite (rows with NaN features?)' % bad)
        indptr, cols, vals = joint_affinities(idx, p)
        self.close()
        h = _lib.TSNE(n, device=self.device)
        try:
            h.set_affinities(indptr, cols, vals)
            h.set_embedding(y0)
            records = []
            if self.exaggeration_iter:
                records.append(h.run(self.exaggeration_iter, self.early_exaggeration, self.momentum[0], lr, self.kl_every))
            if self.n_iter > self.exaggeration_iter:
                if records:
                    # scikit-learn's schedule: each phase starts from a zero update and unit gains.  Carrying the early phase's
                    # gains over costs about 0.02 of final KL on 300 points; the handle itself keeps them across runs.
                    h.set_embedding(h.embedding())
                plain = h.run(self.n_iter - self.exaggeration_iter, 1.0, self.momentum[1], lr, self.kl_every)
                plain[:, 0] += self.exaggeration_iter if records else 0
                records.append(plain)
            self.embedding_ = h.embedding()
        except Exception:
            h.close()
            raise
        self._h = h
        records = np.concatenate(records)
        self.history_ = np.zeros(len(records), HISTORY_DTYPE)
        self.history_['iteration'], self.history_['kl'], self.history_['z'] = records[:, 0].astype(np.int64), records[:, 1], records[:, 2]
        self.kl_divergence_ = float(records[-1, 1])
        self.n_neighbors_, self.learning_rate_, self.beta_ = k, lr, beta
        return self

    def fit_transform(self, X):
        return self.fit(X).embedding_


def neighbor_preservation(idx_high, Y, k, device=0):
    """(n) float64: the share of each row's first k high-dimensional neighbours idx_high[:, :k] found among its k nearest points of
    the map Y (n, 2) float32; the map's lists come from the k-NN handle at D = 2"""
    idx_high, Y = np.asarray(idx_high), _rows(Y, 'Y')
    k = _lib.knn_check_k(k)
    if Y.shape[1] != 2 or idx_high.ndim != 2 or idx_high.shape[0] != Y.shape[0] or idx_high.shape[1] < k or Y.shape[0] <= k:
        raise ValueError('need Y (n > k, 2) and idx_high (n, >= k)')
    n = Y.shape[0]
    knn = _lib.KNN(2, 'sqeuclidean', device=device)
    try:
        knn.set_database(Y)
        knn.query_self()
        own = np.arange(n, dtype=np.int32)
        idx_map, _ = knn.topk(k, group_q=own, group_c=own)
    finally:
        knn.close()
    hits = (idx_high[:, :k, None] == idx_map[:, None, :]).any(axis=2).sum(axis=1)
    return hits / float(k)
