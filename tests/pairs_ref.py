"""float64 forms, derived rounding bounds and the NumPy rank count of csrc/pairs.hip (tests/test_pairs_host.py checks the forms
without a GPU, tests/test_pairs_gpu.py checks the kernels against them).

The head factored over pairs, W1 = [W1v; W1a]:
    u_i = v_i W1v,   t_j = a_j W1a + b1,   margin_ij = sum_k relu(u_ik + t_jk) wd_k + bd,   wd = W2[:, 1] - W2[:, 0],  bd = b2[1] - b2[0]

Bounds.  EPS = 2**-24 is the unit roundoff of one correctly rounded float32 operation; n roundings in a row give a relative error
of at most (1 + EPS)**n - 1 <= (n + 1) EPS for every n used here (n EPS < 2**-11).  No constant below is fitted to a measurement.

  projection   one fma chain over k = 0 .. K-1 started at 0, then (audio side) one addition of the bias: the first product passes K
               roundings of the chain and one of the bias addition, every later one fewer.  |y - y64| <= (K + 2) EPS (|x| |w| + |b|),
               c = 2: one for the bias addition, one for the second-order terms.  The bound holds for any order of the K terms.
  pair         s_k = fl(u_k + t_k): one rounding, |s_k - (u_k + t_k)| <= EPS |u_k + t_k|; max(., 0) is exact, 1-Lipschitz and keeps
               zero at zero, so h_k carries the same relative error.  acc = fma(h_k, wd_k, acc) for k = 0 .. H-1 in that order from
               0: term k passes at most H roundings.  margin = fl(acc + bd): one more.  With A = sum_k relu(u_k + t_k) |wd_k|:
               |m - m64| <= (H + 3) EPS (A + |bd|)   (1 + H + 1 roundings on the longest path, + 1 for the second-order terms).
               When wd and bd are themselves formed in float32 from W2 and b2 (l3_pairs_set_head: one rounding each) and the
               reference uses the exact differences, A and |bd| each carry one more rounding: (H + 4) EPS (A + |bd|).
  probability  p = fl(1 / fl(1 + expf(-m))): expf within 1 ulp = 2 EPS relative (the HIP math API's table), one addition whose
               result is at least the exponential (so the exponential's relative error does not grow), one correctly rounded
               division: 4 roundings' worth, + 1 for the second-order terms, relative to p <= 1.  The sigmoid is 1/4-Lipschitz.
               expf(-m) overflows only for m < -88.7, where the sigmoid is below FLT_MIN: that much is added once.
               |p - sigmoid(m64)| <= 0.25 |m - m64| + 5 EPS sigmoid(m64) + FLT_MIN
"""
import numpy as np

EPS = 2.0 ** -24
FLT_MIN = 2.0 ** -126
F = np.float32
TILE = 64          # L3_PAIRS_TILE: frames and seconds of one workgroup's tile (csrc/pairs.hip)


def f64(a):
    return np.asarray(a, np.float64)


def project_ref(x, w, b=None):
    y = f64(x) @ f64(w)
    return y if b is None else y + f64(b)


def project_bound(x, w, b=None):
    K = np.shape(x)[1]
    mag = np.abs(f64(x)) @ np.abs(f64(w))
    if b is not None:
        mag = mag + np.abs(f64(b))
    return (K + 2) * EPS * mag


def margins_ref(u, t, wd, bd):
    """(Nv, Na) float64 margins of float32 (or float64) projected rows"""
    u, t, wd = f64(u), f64(t), f64(wd)
    out = np.empty((len(u), len(t)))
    for i in range(len(u)):
        out[i] = np.maximum(u[i][None, :] + t, 0.0) @ wd
    return out + float(bd)


def margins_bound(u, t, wd, bd, head_rounded=False):
    u, t, wd = f64(u), f64(t), f64(wd)
    H = u.shape[1]
    A = np.empty((len(u), len(t)))
    for i in range(len(u)):
        A[i] = np.maximum(u[i][None, :] + t, 0.0) @ np.abs(wd)
    return (H + (4 if head_rounded else 3)) * EPS * (A + abs(float(bd)))


def sigmoid_ref(m):
    m = f64(m)
    return np.where(m >= 0, 1.0 / (1.0 + np.exp(-np.abs(m))), np.exp(-np.abs(m)) / (1.0 + np.exp(-np.abs(m))))


def probability_bound(m64, margin_bound):
    return 0.25 * f64(margin_bound) + 5 * EPS * sigmoid_ref(m64) + FLT_MIN


def head_diff(w2, b2, dtype=np.float64):
    """(wd, bd) of dense_2: float64 exact differences, or float32 as l3_pairs_set_head forms them"""
    w2, b2 = np.asarray(w2, dtype), np.asarray(b2, dtype)
    return w2[:, 1] - w2[:, 0], b2[1] - b2[0]


def factored_margins(v, a, w1, b1, w2, b2):
    """float64 margins (Nv, Na) of tower outputs v (Nv, nv), a (Na, na) through the factored head"""
    v, a, w1 = f64(v), f64(a), f64(w1)
    nv = v.shape[1]
    wd, bd = head_diff(w2, b2)
    return margins_ref(v @ w1[:nv], a @ w1[nv:] + f64(b1), wd, bd)


def ranks_ref(m, truth_a=None, truth_v=None, group_v=None, group_a=None):
    """The rank counts of l3_pairs_ranks on a matrix of margins, with NumPy: strictly greater than the truth pair's score, items
    of the query's own group excluded."""
    m = np.asarray(m)
    nv, na = m.shape
    other = np.ones((nv, na), bool) if group_v is None else np.asarray(group_v)[:, None] != np.asarray(group_a)[None, :]
    rv = ra = None
    if truth_a is not None:
        s = m[np.arange(nv), np.asarray(truth_a)]
        rv = np.sum((m > s[:, None]) & other, axis=1).astype(np.int32)
    if truth_v is not None:
        s = m[np.asarray(truth_v), np.arange(na)]
        ra = np.sum((m > s[None, :]) & other, axis=0).astype(np.int32)
    return rv, ra
