"""float64 / NumPy forms of csrc/locmap.hip: the AVC head at every location of one side's last feature map (DESIGN.md 8r;
tests/test_locmap_host.py checks the forms against loops without a GPU, tests/test_locmap_gpu.py checks the kernels against them).

A location is scored like an item (tests/pairs_ref.py): with m (n_items, L, H) the projected location rows and t (n_q, H) the queries,
    margin[i, j, l] = sum_k relu(m[i, l, k] + t[j, k]) wd_k + bd
and the rounding bound of a stored float32 margin is pairs_ref.margins_bound of that (location, query) pair: the chain is the same.

The order of a peak (include/l3hip.h): the larger margin first by float comparison (+0 == -0), among equal margins the smaller
location, a NaN margin never; every margin NaN: peak -inf, arg -1.
"""
import numpy as np

from pairs_ref import margins_bound, margins_ref, project_bound, project_ref, ranks_ref          # noqa: F401 (the oracle's parts)


def maps_ref(m, t, wd, bd, L):
    """(n_items, n_q, L) float64 margins of projected location rows m (n_items L, H) and queries t (n_q, H)"""
    m = np.asarray(m)
    n = m.shape[0] // L
    return margins_ref(m, t, wd, bd).reshape(n, L, len(t)).transpose(0, 2, 1)


def maps_bound(m, t, wd, bd, L, head_rounded=False):
    m = np.asarray(m)
    n = m.shape[0] // L
    return margins_bound(m, t, wd, bd, head_rounded).reshape(n, L, len(t)).transpose(0, 2, 1)


def peaks_ref(maps):
    """(peak, arg) over the last axis of `maps` by the order of a peak; maps of any float type, peak of the same type, arg int32"""
    maps = np.asarray(maps)
    nan = np.isnan(maps)
    filled = np.where(nan, -np.inf, maps)
    peak = filled.max(axis=-1)
    # the first location that is not NaN and equals the peak: np.argmax takes the first of equal values, and +0 == -0
    hit = ~nan & (filled == peak[..., None])
    arg = np.where(hit.any(axis=-1), hit.argmax(axis=-1), -1).astype(np.int32)
    # the peak is that location's margin, bit for bit (of +0 and -0 the one that stands first)
    peak = np.where(arg >= 0, np.take_along_axis(filled, np.maximum(arg, 0)[..., None].astype(np.int64), axis=-1)[..., 0], -np.inf)
    return peak.astype(maps.dtype), arg


def peak_ranks_ref(S, truth_a=None, truth_v=None, group_v=None, group_a=None):
    """l3_pairs_map_ranks: pairs_ref.ranks_ref over S (Nv, Na), the best-location score of every (frame, second) pair"""
    return ranks_ref(S, truth_a, truth_v, group_v, group_a)
