"""The top-k lists of l3_pairs_topk / l3_op_pair_topk on a matrix of margins, with NumPy, straight from the contract in
include/l3hip.h ("The order of a list"): for query row i the candidates are the columns j with group_c[j] != group_q[i] (every column
without groups) and, with a truth, j = truth[i] whatever its group; the larger margin first, the smaller index first among equal
margins, NaN never listed; a list with fewer than k candidates ends in index -1 and margin -inf.  The other direction is the same
function on the transposed matrix with the groups exchanged."""
import numpy as np


def topk_ref(m, k, truth=None, group_q=None, group_c=None):
    """(idx (nq, k) int32, margin (nq, k) float32) of the rows of m (nq, nc)"""
    m = np.asarray(m, np.float32)
    nq, nc = m.shape
    if (group_q is None) != (group_c is None):
        raise ValueError('group_q and group_c come together')
    idx = np.full((nq, k), -1, np.int32)
    margin = np.full((nq, k), -np.inf, np.float32)
    for i in range(nq):
        cand = np.ones(nc, bool) if group_q is None else np.asarray(group_c) != np.asarray(group_q)[i]
        if truth is not None:
            cand[int(truth[i])] = True
        cand &= ~np.isnan(m[i])
        j = np.flatnonzero(cand)
        j = j[np.lexsort((j, -m[i, j]))][:k]          # the last key is the primary one: -margin ascending, then the index
        idx[i, :len(j)] = j
        margin[i, :len(j)] = m[i, j]
    return idx, margin


def same_lists(got, want):
    """indices equal, margins equal as bits"""
    return (got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == want[0].shape and
            np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))
