"""NumPy oracle of l3embedding_amd/csrc/kmeans.hip (include/l3hip.h, "K-means"): the assignment's strict order, the run order of every
float64 sum, the update, the inertia, k-means++ with its edge rules, the fit loop and the label scores.  No GPU, no library.

The run order is written with explicit loops or np.cumsum (a sequential prefix); np.sum adds pairwise and is not the contract.
fit_ref and pp_ref take a `distances(rows, centroids)` callable -> (n, K): float64 on the CPU (distances_f64), or on the GPU the
library's own l3_knn_matrix, whose bits the k-means kernels are held to."""
import numpy as np

RUN = 256          # L3_KMEANS_RUN


def distances_f64(rows, centroids):
    """(n, K) float64 squared Euclidean distances, every operation in float64 (integer rows: exact in int64)"""
    rows, centroids = np.asarray(rows), np.asarray(centroids)
    if rows.dtype.kind in 'iu' and centroids.dtype.kind in 'iu':
        a, b = rows.astype(np.int64), centroids.astype(np.int64)
        return (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2 * (a @ b.T)
    a, b = rows.astype(np.float64), centroids.astype(np.float64)
    return np.maximum(0.0, (a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :] - 2.0 * (a @ b.T))


# ---- the assignment ------------------------------------------------------------------------------------------------------------------
def assign_ref(M):
    """(labels (n) int32, dist (n) of M's float dtype) of a distance matrix M (n, K): the smallest distance, the smaller index among
    equal distances; a NaN never wins; a row of NaNs alone has label -1 and distance NaN"""
    M = np.asarray(M)
    F = M if M.dtype.kind == 'f' else M.astype(np.float64)
    nan = np.isnan(F)
    masked = np.where(nan, np.inf, F)
    labels = np.argmin(masked, axis=1).astype(np.int32)          # the first minimum: the smaller index among equals
    for i in np.flatnonzero(np.isinf(masked.min(axis=1)) & nan.any(axis=1)):          # +inf beside NaNs: the first that is no NaN
        ok = np.flatnonzero(~nan[i])
        labels[i] = ok[0] if len(ok) else -1
    dist = np.where(labels >= 0, F[np.arange(len(F)), np.maximum(labels, 0)], np.nan).astype(F.dtype)
    return labels, dist


def assign_bruteforce(M):
    """assign_ref by a double loop: the oracle's own check"""
    M = np.asarray(M)
    labels, dist = np.full(len(M), -1, np.int32), np.full(len(M), np.nan, np.float64)
    for i in range(M.shape[0]):
        best = None
        for j in range(M.shape[1]):
            d = float(M[i, j])
            if d != d:
                continue
            if best is None or d < best[0]:          # (j ascends: an equal distance later never replaces)
                best = (d, j)
        if best is not None:
            dist[i], labels[i] = best
    return labels, dist


# ---- the order of a float64 sum --------------------------------------------------------------------------------------------------------
def run_sum(terms):
    """the members' terms (m,) or (m, D), in member order -> their float64 sum in the library's order: runs of RUN members, each
    summed sequentially from 0.0, the run sums added sequentially in ascending order"""
    terms = np.asarray(terms, np.float64)
    total = np.zeros(terms.shape[1:], np.float64)
    for r in range(0, len(terms), RUN):
        run = np.zeros(terms.shape[1:], np.float64)
        for v in terms[r:r + RUN]:
            run = run + v
        total = total + run
    return total


def run_sum_fast(terms):
    """run_sum with np.cumsum for the sequential part (the same additions in the same order)"""
    terms = np.asarray(terms, np.float64)
    zero = np.zeros((1,) + terms.shape[1:], np.float64)
    runs = [np.cumsum(np.concatenate([zero, terms[r:r + RUN]]), axis=0)[-1] for r in range(0, len(terms), RUN)]
    return np.cumsum(np.concatenate([zero] + [t[None] for t in runs]), axis=0)[-1]


def cumulative_ref(v):
    """(cum (n) float64, total) of the seeding: rows in runs of RUN, within a run the sequential prefix from 0.0, a run's offset the
    sequential sum of the earlier runs' totals, cum = offset + prefix"""
    v = np.asarray(v, np.float64)
    cum, off = np.empty(len(v), np.float64), 0.0
    for r in range(0, len(v), RUN):
        pre = np.cumsum(np.concatenate([[0.0], v[r:r + RUN]]))[1:]
        cum[r:r + RUN] = off + pre
        off = off + pre[-1]
    return cum, off


def update_ref(X, labels, centroids):
    """-> (new centroids (K, D) float32, counts (K) int64): C[c] = (float)(S_c / n_c); an empty cluster keeps its centroid"""
    X, labels = np.asarray(X), np.asarray(labels)
    new = np.array(centroids, np.float32, copy=True)
    counts = np.zeros(len(new), np.int64)
    for c in range(len(new)):
        members = np.flatnonzero(labels == c)
        counts[c] = len(members)
        if len(members):
            new[c] = (run_sum_fast(X[members]) / np.float64(len(members))).astype(np.float32)
    return new, counts


def inertia_ref(dist, labels):
    """the float64 sum, in the run order, of the float32 distances of the rows with a label"""
    dist, labels = np.asarray(dist), np.asarray(labels)
    return float(run_sum_fast(dist[labels >= 0].astype(np.float64)))


# ---- seeding -------------------------------------------------------------------------------------------------------------------------
def uniform_pick(u, n):
    return min(n - 1, int(np.floor(np.float64(u) * np.float64(n))))


def pp_ref(X, u, distances):
    """plain k-means++ from the draws u (K,) -> the chosen rows (K) int64; include/l3hip.h has the rule and its edges"""
    X = np.asarray(X)
    n = len(X)
    chosen = [uniform_pick(u[0], n)]
    mind = np.asarray(distances(X, X[chosen[0]:chosen[0] + 1]))[:, 0]
    for t in range(1, len(u)):
        with np.errstate(invalid='ignore'):
            v = np.where(np.isnan(mind), 0.0, mind).astype(np.float64)
        cum, total = cumulative_ref(v)
        if total == 0.0:
            pick = uniform_pick(u[t], n)
        else:
            hit = np.flatnonzero(cum > np.float64(u[t]) * total)
            positive = np.flatnonzero(v > 0.0)
            pick = int(hit[0]) if len(hit) else int(positive[-1]) if len(positive) else uniform_pick(u[t], n)
        chosen.append(pick)
        d = np.asarray(distances(X, X[pick:pick + 1]))[:, 0]
        with np.errstate(invalid='ignore'):
            mind = np.where(d < mind, d, mind)
    return np.array(chosen, np.int64)


# ---- the fit loop ----------------------------------------------------------------------------------------------------------------------
def fit_ref(X, centroids, max_iter, distances):
    """the loop of l3_kmeans_fit -> dict(centroids, labels, dist, inertia, history (n_iter, 3), n_iter)"""
    X = np.asarray(X)
    C = np.array(centroids, np.float32, copy=True)
    prev = np.full(len(X), -2, np.int64)
    history, settled = [], False
    for it in range(max_iter):
        labels, dist = assign_ref(distances(X, C))
        inertia = inertia_ref(dist, labels)
        changed = int(np.sum(labels != prev))
        counts = np.bincount(labels[labels >= 0], minlength=len(C))
        history.append((inertia, float(changed), float(np.sum(counts == 0))))
        prev = labels
        if changed == 0:
            settled = True
            break
        C, _ = update_ref(X, labels, C)
    if not settled:
        labels, dist = assign_ref(distances(X, C))
        inertia = inertia_ref(dist, labels)
    return dict(centroids=C, labels=labels, dist=dist, inertia=inertia, history=np.array(history, np.float64).reshape(-1, 3),
                n_iter=len(history))


def seeds_ref(random_state, n_init):
    return np.random.RandomState(random_state).randint(2 ** 31 - 1, size=n_init)


def best_of_ref(X, K, random_state, n_init, max_iter, distances):
    """n_init restarts of k-means++ and the fit -> the result of the lowest final inertia, the first among equals"""
    best = None
    for seed in seeds_ref(random_state, n_init):
        chosen = pp_ref(X, np.random.RandomState(seed).random_sample(K), distances)
        got = fit_ref(X, np.asarray(X)[chosen], max_iter, distances)
        got['chosen'] = chosen
        if best is None or got['inertia'] < best['inertia']:
            best = got
    return best


# ---- label statistics ------------------------------------------------------------------------------------------------------------------
def contingency_ref(labels, classes, K, C):
    table = np.zeros((K, C), np.int64)
    labels, classes = np.asarray(labels), np.asarray(classes)
    keep = labels >= 0
    np.add.at(table, (labels[keep], classes[keep]), 1)
    return table


def _entropy(counts):
    p = counts[counts > 0].astype(np.float64)
    total = p.sum()
    return float(-np.sum((p / total) * (np.log(p) - np.log(total))))


def nmi_ref(table):
    """mutual information over the arithmetic mean of the two entropies (natural logarithms); 1.0 when both partitions are trivial"""
    t = np.asarray(table, np.float64)
    a, b, N = t.sum(axis=1), t.sum(axis=0), t.sum()
    if np.count_nonzero(a) <= 1 and np.count_nonzero(b) <= 1:
        return 1.0
    i, j = np.nonzero(t)
    mi = float(np.sum(t[i, j] / N * (np.log(t[i, j]) - np.log(N) - (np.log(a[i]) + np.log(b[j]) - 2.0 * np.log(N)))))
    mi = max(mi, 0.0)
    return mi / max(0.5 * (_entropy(a) + _entropy(b)), np.finfo(np.float64).eps)


def purity_ref(table):
    t = np.asarray(table, np.int64)
    return float(t.max(axis=1).sum()) / float(t.sum())


def adjusted_rand_ref(table):
    """from the pair counts, in exact integers until the last division"""
    t = [[int(v) for v in row] for row in np.asarray(table)]
    n = sum(sum(row) for row in t)
    a, b = [sum(row) for row in t], [sum(col) for col in zip(*t)]
    squares = sum(v * v for row in t for v in row)
    tp = squares - n
    fp = sum(t[i][j] * b[j] for i in range(len(a)) for j in range(len(b))) - squares
    fn = sum(t[i][j] * a[i] for i in range(len(a)) for j in range(len(b))) - squares
    tn = n * n - fp - fn - squares
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def blobs(K, D, per, spread, seed=5):
    """the blob fixtures of the quality bar: centres 3 randn(K, D), rows centre + spread randn -> (X float32, y)"""
    rng = np.random.RandomState(seed)
    centres = 3.0 * rng.randn(K, D)
    y = np.repeat(np.arange(K), per)
    X = centres[y] + spread * rng.randn(K * per, D)
    return X.astype(np.float32), y
