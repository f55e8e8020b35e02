"""Float64 / int64 NumPy oracle of l3embedding_amd/csrc/knn.hip (include/l3hip.h, "Nearest neighbours"): distances, the strict order
of a neighbour list, groups, empty slots, votes and per-file vote sums.  No GPU, no library: plain loops where the order matters."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def distances_ref(Q, X, metric):
    """(nq, nc) float64 distances of float rows, every operation in float64 (int64 rows: exact under 'sqeuclidean')"""
    Q, X = np.asarray(Q), np.asarray(X)
    if Q.dtype.kind in 'iu' and metric == 'sqeuclidean':
        Q, X = Q.astype(np.int64), X.astype(np.int64)
        dot = Q @ X.T
        return (Q * Q).sum(axis=1)[:, None] + (X * X).sum(axis=1)[None, :] - 2 * dot
    Q, X = Q.astype(np.float64), X.astype(np.float64)
    dot = Q @ X.T
    nq, nx = (Q * Q).sum(axis=1), (X * X).sum(axis=1)
    if metric == 'sqeuclidean':
        return np.maximum(0.0, nq[:, None] + nx[None, :] - 2.0 * dot)
    if metric != 'cosine':
        raise ValueError(metric)
    with np.errstate(divide='ignore', invalid='ignore'):
        rq, rx = np.where(nq > 0, 1.0 / np.sqrt(nq), 0.0), np.where(nx > 0, 1.0 / np.sqrt(nx), 0.0)
    return 1.0 - dot * rq[:, None] * rx[None, :]


def distance_bound(Q, X, metric):
    """|d - d64| <= bound, elementwise (nq, nc).  Each of dot, nn(q), nn(c) is a D-term float32 fma chain, error <= D u sum|terms|,
    and sum|q_i c_i| <= (nn(q) + nn(c)) / 2; the epilogue adds a few roundings: (2 D + 4) u (nn64(q) + nn64(c)) under 'sqeuclidean',
    (2 D + 8) u under 'cosine' (where everything is normalised to 1)."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    D = Q.shape[1]
    if metric == 'cosine':
        return np.full((len(Q), len(X)), (2 * D + 8) * U)
    return (2 * D + 4) * U * ((Q * Q).sum(axis=1)[:, None] + (X * X).sum(axis=1)[None, :])


def topk_ref(M, k, group_q=None, group_c=None):
    """(idx (nq, k) int32, dist (nq, k) of M's dtype) of a distance matrix M: per query the candidates j with group_c[j] !=
    group_q[i] (all without groups) whose distance is not NaN, by (distance, index) ascending; the tail is (-1, +inf)."""
    M = np.asarray(M)
    nq, nc = M.shape
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, M.dtype if M.dtype.kind == 'f' else np.float64)
    for i in range(nq):
        keep = ~np.isnan(M[i].astype(np.float64))
        if group_q is not None:
            keep &= np.asarray(group_c) != group_q[i]
        js = np.flatnonzero(keep)
        order = js[np.lexsort((js, M[i, js]))][:k]          # by distance, then by index
        idx[i, :len(order)] = order
        dist[i, :len(order)] = M[i, order]
    return idx, dist


def topk_bruteforce(M, k, group_q=None, group_c=None):
    """topk_ref by a double loop and a selection of the minimum: the oracle's own check"""
    M = np.asarray(M)
    nq, nc = M.shape
    idx = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float64)
    for i in range(nq):
        taken = set()
        for slot in range(k):
            best = None
            for j in range(nc):
                d = float(M[i, j])
                if j in taken or d != d or (group_q is not None and group_c[j] == group_q[i]):
                    continue
                if best is None or d < best[0] or (d == best[0] and j < best[1]):
                    best = (d, j)
            if best is None:
                break
            taken.add(best[1])
            idx[i, slot], dist[i, slot] = best[1], best[0]
    return idx, dist


def _leader(counts):
    """the class of the most votes, the lowest class among equals, -1 when nobody voted"""
    return int(np.argmax(counts)) if counts.max() > 0 else -1


def vote_ref(idx, labels, ks, n_classes, file_idxs=None):
    """-> counts (n, S, C) int64, pred (n, S), and with file_idxs file_counts (F, S, C), file_pred (F, S): entry l of a list votes
    for its label at every size ks[s] > l; empty slots (-1) do not vote; a file's score is the sum of its rows' votes."""
    idx, labels = np.asarray(idx), np.asarray(labels)
    n, S = len(idx), len(ks)
    counts = np.zeros((n, S, n_classes), np.int64)
    pred = np.zeros((n, S), np.int64)
    for i in range(n):
        for s, k in enumerate(ks):
            for j in idx[i, :k]:
                if j >= 0:
                    counts[i, s, labels[j]] += 1
            pred[i, s] = _leader(counts[i, s])
    if file_idxs is None:
        return counts, pred
    files = np.asarray(file_idxs).reshape(-1, 2)
    file_counts = np.stack([counts[a:b].sum(axis=0) for a, b in files])
    file_pred = np.array([[_leader(file_counts[f, s]) for s in range(S)] for f in range(len(files))], np.int64)
    return counts, pred, file_counts, file_pred


def search_choice_ref(ks, accuracies):
    """the first maximum of the validation accuracy, in the order of ks"""
    best = 0
    for g in range(1, len(ks)):
        if accuracies[g] > accuracies[best]:
            best = g
    return ks[best]
