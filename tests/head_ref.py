"""float64 restatements, rounding bounds and float32 emulations of the head, loss, L2-sum, Adam and BatchNorm moving-average
kernels of csrc/elementwise.hip (tests/test_head_host.py checks them against each other without a GPU, tests/test_head_gpu.py
checks the kernels against them).

Three things per kernel:
  *_ref    plain NumPy float64 of the operation on the float32 inputs (oracle.l3_oracle where it states the operation);
  *_bound  a rigorous bound on |float32 kernel - float64| from the kernel's summation structure (EPS = 2**-24, the unit
           roundoff of a correctly rounded float32 add / multiply / fma), or, for the loss, Adam and the moving averages, a running
           error propagated through the formula in float64 by `Err` below;
  *_emu    the kernel's own order of operations in NumPy float32: the CPU stand-in that must lie within HALF of the bound (the other
           half covers fma contraction and the device math library, where the emulation may differ in the last bit).

Per-operation errors of `Err`: one ulp (2**-23 relative) per float32 add, subtract, multiply and divide -- twice what IEEE
rounding gives, which also covers a contraction the compiler may or may not make.  expf and logf: 2 ulp, sqrtf: 1 ulp.  The HIP
math API table gives expf 1, logf 1 (2 in some releases) and sqrtf 1 ulp; the larger figure is taken for both transcendental
functions.  fminf / fmaxf / comparisons are exact."""
import numpy as np

from oracle import l3_oracle as o

EPS = 2.0 ** -24
ULP = 2.0 ** -23
ULP_EXP, ULP_LOG, ULP_SQRT = 2, 2, 1
TINY = 2.0 ** -149           # a float32 result may also be off by the smallest denormal
F = np.float32
DENSE_KS = 8
SUMSQ_BLOCKS = 64
SUMSQ_MAX_SEGS = 24


def f64(a):
    return np.asarray(a, np.float64)


def fma32(a, b, c):
    """fl32(a * b + c) for float32 operands: the product is exact in float64, the sum is rounded once more on the way (a double
    rounding that can differ from a true fma in the last bit, rarely)."""
    return (f64(a) * f64(b) + f64(c)).astype(F)


# ---- running-error arithmetic ------------------------------------------------------------------------------------------------
class Err(object):
    """A float64 value v with a bound e on |float32 computation - v|.  Every operation returns the exact float64 result of the
    operands' values and the first-principles bound: the operands' errors carried through the operation (with the operands taken
    at their worst inside their error interval) plus `ulps` ulp of the largest result the float32 computation can have."""

    def __init__(self, v, e=0.0):
        self.v = f64(v)
        self.e = np.broadcast_to(f64(e), self.v.shape).copy() if np.ndim(self.v) else f64(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def _round(self, v, e, ulps=1):
        return Err(v, e + ulps * ULP * (np.abs(v) + e) + TINY)

    def __add__(self, other):
        other = Err.of(other)
        return self._round(self.v + other.v, self.e + other.e)

    def __sub__(self, other):
        other = Err.of(other)
        return self._round(self.v - other.v, self.e + other.e)

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, other):
        other = Err.of(other)
        e = np.abs(self.v) * other.e + np.abs(other.v) * self.e + self.e * other.e
        return self._round(self.v * other.v, e)

    def __truediv__(self, other):
        other = Err.of(other)
        lo = np.abs(other.v) - other.e
        assert np.all(lo > 0), 'divisor not bounded away from zero'
        v = self.v / other.v
        e = (self.e + np.abs(v) * other.e) / lo
        return self._round(v, e)

    def exp(self):
        v = np.exp(self.v)
        return self._round(v, v * np.expm1(self.e), ULP_EXP)

    def log(self):
        lo = self.v - self.e
        assert np.all(lo > 0), 'logarithm of a value not bounded away from zero'
        return self._round(np.log(self.v), np.log(self.v / lo), ULP_LOG)

    def sqrt(self):
        v = np.sqrt(self.v)
        e = np.maximum(np.sqrt(self.v + self.e) - v, v - np.sqrt(np.maximum(self.v - self.e, 0.0)))
        return self._round(v, e, ULP_SQRT)

    def clip(self, lo, hi):      # fminf(fmaxf(x, lo), hi): exact and 1-Lipschitz
        return Err(np.clip(self.v, lo, hi), self.e)

    def where(self, cond, other):
        other = Err.of(other)
        return Err(np.where(cond, self.v, other.v), np.where(cond, self.e, np.broadcast_to(other.e, np.shape(cond))))

    def __getitem__(self, idx):
        return Err(self.v[idx], self.e[idx])


# ---- dense head --------------------------------------------------------------------------------------------------------------
def dense_fwd_ref(x, w, b, relu):
    y = f64(x) @ f64(w) + f64(b)
    return np.maximum(y, 0) if relu else y


def dense_fwd_bound(x, w, b):
    """Each output is 8 fma chains of ceil(K / 8) terms, 7 adds of the partial sums and the bias add: at most ceil(K / 8) + 8
    roundings lie on the path of any product (+ 2 for the second-order terms).  ReLU is exact and 1-Lipschitz."""
    K = x.shape[1]
    return (-(-K // DENSE_KS) + 10) * EPS * (np.abs(f64(x)) @ np.abs(f64(w)) + np.abs(f64(b)))


def dense_fwd_emu(x, w, b, relu):
    x, w, b = F(x), F(w), F(b)
    B, K = x.shape
    N = w.shape[1]
    klen = -(-K // DENSE_KS)
    ps = np.zeros((DENSE_KS, B, N), F)
    for ks in range(DENSE_KS):
        for k in range(ks * klen, min(K, ks * klen + klen)):
            ps[ks] = fma32(x[:, k:k + 1], w[k:k + 1, :], ps[ks])
    acc = ps[0]
    for ks in range(1, DENSE_KS):
        acc = acc + ps[ks]
    acc = acc + b
    return np.maximum(acc, F(0)) if relu else acc


def dense_slice_ends(K):
    """First and last k of every non-empty K slice of dense_fwd_kernel."""
    klen = -(-K // DENSE_KS)
    ks = []
    for s in range(DENSE_KS):
        k0, k1 = s * klen, min(K, s * klen + klen)
        if k1 > k0:
            ks += [k0, k1 - 1]
    return sorted(set(ks))


def dense_bwd_ref(x, w, dy):
    x, w, dy = f64(x), f64(w), f64(dy)
    return x.T @ dy, dy.sum(axis=0), dy @ w.T


def dense_bwd_bound(x, w, dy):
    """dw[k, n] and db[n] are one sequential chain over the B rows, dx[b, k] one over the N columns."""
    ax, aw, ady = np.abs(f64(x)), np.abs(f64(w)), np.abs(f64(dy))
    B, N = dy.shape
    return (B + 2) * EPS * (ax.T @ ady), (B + 2) * EPS * ady.sum(axis=0), (N + 2) * EPS * (ady @ aw.T)


def dense_bwd_emu(x, w, dy):
    x, w, dy = F(x), F(w), F(dy)
    B, K = x.shape
    N = w.shape[1]
    dw, db, dx = np.zeros((K, N), F), np.zeros(N, F), np.zeros((B, K), F)
    for b in range(B):
        dw = fma32(x[b][:, None], dy[b][None, :], dw)
        db = db + dy[b]
    for n in range(N):
        dx = fma32(dy[:, n:n + 1], w[None, :, n], dx)
    return dw, db, dx


# ---- two-class softmax + keras categorical cross-entropy ---------------------------------------------------------------------------
CE_EPS = F(1e-7)              # the kernel's clip constants, in float32 as keras computes them (epsilon, 1 - epsilon)
CE_HI = F(1.0) - CE_EPS


def softmax_ce_ref(z, t, gscale):
    """oracle.loss_and_grads' loss block (softmax, p / sum, clip, -t log, its gradient through clip -> normalise -> softmax) with
    the clip constants at the float32 values the kernel and keras use.  -> dict(probs, q, dlogits, loss (per row), correct)."""
    z, t = f64(z), f64(t)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    s = p.sum(axis=1, keepdims=True)
    q = p / s
    lo, hi = f64(CE_EPS), f64(CE_HI)
    qc = np.clip(q, lo, hi)
    loss = -(t * np.log(qc)).sum(axis=1)
    dqc = -(t / qc) * f64(gscale)
    dq = np.where((q >= lo) & (q <= hi), dqc, 0)
    dp = dq / s - (dq * p).sum(axis=1, keepdims=True) / (s * s)
    dz = p * (dp - (dp * p).sum(axis=1, keepdims=True))
    correct = (p[:, 1] > p[:, 0]).astype(np.int64) == (t[:, 1] > t[:, 0]).astype(np.int64)
    return dict(probs=p, q=q, dlogits=dz, loss=loss, correct=correct)


def softmax_ce_bound(z, t, gscale):
    """The kernel's formula, operation for operation, in `Err` arithmetic (z - max exact up to one rounding, expf, the sum, 1 / sum,
    the products, p0 + p1, the two quotients, the clip, logf, the label products, and the gradient chain), so the bound holds for
    whatever the float32 intermediates round to.  The clip's branch (q inside [1e-7, 1 - 1e-7] or not) is discontinuous: `unsure`
    marks the rows where q lies within its own error of a threshold, where float32 and float64 may take different branches; their
    gradient is not comparable.  The loss sum adds the per-row terms in the kernel's order (a chain of ceil(B / 256) adds per
    thread, then the 8-level tree), every add with its rounding.
    -> dict(probs, dlogits, loss_sum: bounds; unsure: bool per row)."""
    z, t = Err(f64(z)), f64(t)
    g = f64(F(gscale))
    mx = np.maximum(z.v[:, 0], z.v[:, 1])
    e0, e1 = (z[:, 0] - mx).exp(), (z[:, 1] - mx).exp()
    inv = Err(1.0) / (e0 + e1)
    p0, p1 = e0 * inv, e1 * inv
    sm = p0 + p1
    q0, q1 = p0 / sm, p1 / sm
    lo, hi = f64(CE_EPS), f64(CE_HI)
    c0, c1 = q0.clip(lo, hi), q1.clip(lo, hi)
    loss = -(c0.log() * t[:, 0] + c1.log() * t[:, 1])
    unsure = np.zeros(len(t), bool)
    for q in (q0, q1):
        unsure |= (np.abs(q.v - lo) <= q.e) | (np.abs(q.v - hi) <= q.e)
    in0, in1 = (q0.v >= lo) & (q0.v <= hi), (q1.v >= lo) & (q1.v <= hi)
    dq0 = (-(Err(t[:, 0]) / c0) * g).where(in0, 0.0)
    dq1 = (-(Err(t[:, 1]) / c1) * g).where(in1, 0.0)
    dot = (dq0 * p0 + dq1 * p1) / (sm * sm)
    dp0, dp1 = dq0 / sm - dot, dq1 / sm - dot
    pd = dp0 * p0 + dp1 * p1
    dz0, dz1 = p0 * (dp0 - pd), p1 * (dp1 - pd)
    B = len(t)
    pad = (-B) % 256
    lv = np.concatenate([loss.v, np.zeros(pad)]).reshape(-1, 256)
    le = np.concatenate([loss.e, np.zeros(pad)]).reshape(-1, 256)
    acc = Err(np.zeros(256))
    for r in range(lv.shape[0]):
        acc = acc + Err(lv[r], le[r])
    s = 128
    while s > 0:
        acc = acc[:s] + acc[s:2 * s]
        s >>= 1
    return dict(probs=np.stack([p0.e, p1.e], axis=1), dlogits=np.stack([dz0.e, dz1.e], axis=1), loss_sum=float(acc.e[0]),
                unsure=unsure)


def softmax_ce_emu(z, t, gscale):
    z, t, g = F(z), F(t), F(gscale)
    z0, z1, t0, t1 = z[:, 0], z[:, 1], t[:, 0], t[:, 1]
    mx = np.maximum(z0, z1)
    e0, e1 = np.exp(z0 - mx), np.exp(z1 - mx)
    inv = F(1) / (e0 + e1)
    p0, p1 = e0 * inv, e1 * inv
    sm = p0 + p1
    q0, q1 = p0 / sm, p1 / sm
    c0, c1 = np.minimum(np.maximum(q0, CE_EPS), CE_HI), np.minimum(np.maximum(q1, CE_EPS), CE_HI)
    loss = -(t0 * np.log(c0) + t1 * np.log(c1))
    correct = (p1 > p0) == (t1 > t0)
    dq0 = np.where((q0 >= CE_EPS) & (q0 <= CE_HI), -(t0 / c0) * g, F(0))
    dq1 = np.where((q1 >= CE_EPS) & (q1 <= CE_HI), -(t1 / c1) * g, F(0))
    dot = (dq0 * p0 + dq1 * p1) / (sm * sm)
    dp0, dp1 = dq0 / sm - dot, dq1 / sm - dot
    pd = dp0 * p0 + dp1 * p1
    dz = np.stack([p0 * (dp0 - pd), p1 * (dp1 - pd)], axis=1)
    B = len(t0)
    pad = (-B) % 256
    rows = np.concatenate([loss, np.zeros(pad, F)]).reshape(-1, 256)
    acc = np.zeros(256, F)
    for r in rows:
        acc = acc + r
    s = 128
    while s > 0:
        acc = acc[:s] + acc[s:2 * s]
        s >>= 1
    assert loss.dtype == F and dz.dtype == F and acc.dtype == F
    return dict(probs=np.stack([p0, p1], axis=1), dlogits=dz, loss_sum=acc[0], correct=float(correct.sum()))


# ---- sums of squares ---------------------------------------------------------------------------------------------------------
def sumsq_ref(base, off, n):
    return np.array([(f64(base[o_:o_ + n_]) ** 2).sum() for o_, n_ in zip(off, n)])


def _sumsq_geometry(n):
    nb = min(max(-(-n // (256 * 32)), 1), 1024)
    return nb, -(-n // (nb * 256))


def _multi_geometry(off, n):
    head = min(n, (4 - (off & 3)) & 3)          # the base buffer is 16-byte aligned
    n4 = (n - head) >> 2
    return head, n4, n - head - 4 * n4, -(-n4 // (SUMSQ_BLOCKS * 256))


def sumsq_bound(base, off, n, multi):
    """(longest per-thread fma chain + 8 levels of float32 tree + 2) EPS sum x^2.  sumsq_kernel: min(max(ceil(n / 8192), 1),
    1024) blocks of 256 threads in a grid-stride loop, so a thread's chain is ceil(n / (256 blocks)) long; the 256 partials meet in
    an 8-level tree; the blocks' partials are added in double.  sumsq_multi_kernel: 64 x 256 threads take the aligned float4s in
    a grid-stride loop (4 fma each), the first threads of block 0 one head and one tail element more; 6 shuffle levels and 2 adds
    through LDS; the 64 partials are added in double.  The + 2 covers the final rounding to float32 and the second-order terms."""
    out = []
    for o_, n_ in zip(off, n):
        chain = 4 * _multi_geometry(int(o_), int(n_))[3] + 2 if multi else _sumsq_geometry(int(n_))[1]
        out.append((chain + 8 + 2) * EPS * (f64(base[o_:o_ + n_]) ** 2).sum())
    return np.array(out)


def _strided_fma(x, threads):
    """acc[t] over x[t], x[t + threads], ... as fma(v, v, acc); x zero padded (an fma with 0 leaves acc as it is)."""
    rows = np.concatenate([x, np.zeros((-len(x)) % threads, F)]).reshape(-1, threads)
    acc = np.zeros(threads, F)
    for r in rows:
        acc = fma32(r, r, acc)
    return acc


def sumsq_emu(base, off, n, multi):
    base = F(base)
    out = []
    lanes = np.arange(64)
    for o_, n_ in zip(off, n):
        x = base[o_:o_ + n_]
        if not multi:
            nb, _ = _sumsq_geometry(int(n_))
            sm = _strided_fma(x, nb * 256).reshape(nb, 256)
            s = 128
            while s > 0:
                sm = sm[:, :s] + sm[:, s:2 * s]
                s >>= 1
            out.append(F(f64(sm[:, 0]).sum()))
            continue
        head, n4, rest, iters = _multi_geometry(int(o_), int(n_))
        T = SUMSQ_BLOCKS * 256
        x4 = x[head:head + 4 * n4].reshape(n4, 4)
        x4 = np.concatenate([x4, np.zeros(((-n4) % T, 4), F)]).reshape(-1, T, 4)
        acc = np.zeros(T, F)
        for it in x4:
            for e in range(4):
                acc = fma32(it[:, e], it[:, e], acc)
        acc[:head] = fma32(x[:head], x[:head], acc[:head])
        tail = x[head + 4 * n4:]
        acc[:rest] = fma32(tail, tail, acc[:rest])
        a = acc.reshape(SUMSQ_BLOCKS, 4, 64)
        for sh in (32, 16, 8, 4, 2, 1):
            a = a + a[:, :, lanes ^ sh]
        w = a[:, :, 0]
        part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
        assert part.dtype == F
        out.append(F(f64(part).sum()))
    return np.array(out, F)


# ---- Adam --------------------------------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, n_l2, l2x2, lr_t, b1, b2, eps, gscale):
    """keras Adam at a given lr_t on g * gscale + l2x2 * p (the first n_l2 elements), float64 -> (p, m, v)."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    gi = g * f64(gscale) + np.where(np.arange(p.size) < n_l2, f64(l2x2) * p, 0.0)
    m = f64(b1) * m + (1 - f64(b1)) * gi
    v = f64(b2) * v + (1 - f64(b2)) * gi * gi
    return p - f64(lr_t) * m / (np.sqrt(v) + f64(eps)), m, v


def adam_bound(p, g, m, v, n_l2, l2x2, lr_t, b1, b2, eps, gscale, em=0.0, ev=0.0):
    """adam_kernel's formula in `Err` arithmetic: g * gscale; the L2 fma (as a multiply and an add); 1 - b1, b1 m, (1 - b1) gi and
    their sum; the same for v with gi * gi; sqrtf; + eps; lr_t * m; the quotient; the subtraction.  -> bounds on (p, m, v).  v is
    taken as normal (the tests keep |g| gscale >= 1e-15): a denormal v would lose more than the ulp this model charges.  em, ev:
    bounds on how far the float32 moments that go in are from the float64 m, v given (a second step); lr_t may be an `Err`."""
    p0, g, m, v = Err(f64(p)), Err(f64(g)), Err(f64(m), em), Err(f64(v), ev)
    gi = g * f64(gscale)
    gi = (Err(f64(l2x2)) * p0 + gi).where(np.arange(p0.v.size) < n_l2, gi)
    c1, c2 = Err(1.0) - f64(b1), Err(1.0) - f64(b2)
    mi = Err(f64(b1)) * m + c1 * gi
    vi = Err(f64(b2)) * v + c2 * gi * gi
    pn = p0 - Err.of(lr_t) * mi / (vi.sqrt() + f64(eps))
    return pn.e, mi.e, vi.e


def adam_lr_t(lr, t, b1, b2):
    """lr_t as the engine computes it in float32, lr * (sqrtf(1 - powf(b2, t)) / (1 - powf(b1, t))), as an `Err` (powf: 2 ulp)."""
    p1, p2 = f64(b1) ** float(t), f64(b2) ** float(t)
    num = (Err(1.0) - Err(p2, 2 * ULP * p2)).sqrt()
    den = Err(1.0) - Err(p1, 2 * ULP * p1)
    return Err(f64(F(lr))) * (num / den)


def adam_emu(p, g, m, v, n_l2, l2x2, lr_t, b1, b2, eps, gscale):
    p, g, m, v = F(p), F(g), F(m), F(v)
    l2x2, lr_t, b1, b2, eps, gscale = [F(a) for a in (l2x2, lr_t, b1, b2, eps, gscale)]
    gi = g * gscale
    gi = np.where(np.arange(p.size) < n_l2, fma32(l2x2, p, gi), gi)
    mi = b1 * m + (F(1) - b1) * gi
    vi = b2 * v + (F(1) - b2) * gi * gi
    pn = p - lr_t * mi / (np.sqrt(vi) + eps)
    assert pn.dtype == F and mi.dtype == F and vi.dtype == F
    return pn, mi, vi


# ---- BatchNorm moving averages -----------------------------------------------------------------------------------------------
def bn_moving_ref(moving, biased, values, momentum, zero_debias, step):
    """`values` (replicas, C): the updates of one statistic, applied in order; `step` = updates applied once done.  float64
    -> (moving, biased); biased is returned unchanged without zero_debias."""
    mom = f64(momentum)
    if zero_debias:
        b = f64(biased)
        for val in f64(values):
            b = b - (b - val) * (1 - mom)
        return b / (1.0 - mom ** float(step)), b
    mv = f64(moving)
    for val in f64(values):
        mv = mv * mom + val * (1 - mom)
    return mv, f64(biased)


def bn_moving_bound(moving, biased, values, momentum, zero_debias, step, eb=0.0):
    """The same chain in `Err` arithmetic: three float32 operations per replica (and 1 - momentum), then with zero_debias the
    division by the double-precision 1 - momentum^step rounded to float32: 3 replicas + 1 operations at most.
    -> bounds on (moving, biased).  eb: a bound on how far the float32 `biased` that goes in is from the float64 one given."""
    mom = f64(momentum)
    c = Err(1.0) - mom
    if zero_debias:
        b = Err(f64(biased), eb)
        for val in f64(values):
            b = b - (b - val) * c
        return (b / Err(1.0 - mom ** float(step))).e, b.e
    mv = Err(f64(moving))
    for val in f64(values):
        mv = mv * mom + Err(val) * c
    return mv.e, np.zeros_like(mv.e)


def bn_moving_emu(moving, biased, values, momentum, zero_debias, step):
    mom = F(momentum)
    c = F(1) - mom
    if zero_debias:
        b = F(biased)
        for val in F(values):
            b = b - (b - val) * c
        corr = 1.0 - float(mom) ** float(step)
        return (f64(b) / corr).astype(F), b
    mv = F(moving)
    for val in F(values):
        mv = mv * mom + val * c
    return mv, F(biased)


# ---- the input sets of tests/test_head_gpu.py (tests/test_head_host.py runs the emulations over the same ones) -----------------------
DENSE_FWD_CASES = [(3, 1024, 128, 1), (3, 128, 2, 0), (1, 7, 2, 0), (2, 1030, 130, 1), (5, 1, 1, 0), (257, 64, 2, 0)]
DENSE_BWD_CASES = [(B, K, N) for (K, N) in ((1024, 128), (128, 2), (1000, 300)) for B in (1, 7, 8, 9, 64, 257)]
SOFTMAX_B = [1, 2, 255, 256, 257, 600]
ADAM_N = [1, 255, 256, 257, 100003]
ADAM_GSCALE = [1.0, 1.0 / 64, 8.0]
ADAM_CONST = dict(l2x2=F(2e-5), lr_t=F(1e-4) * (np.sqrt(F(1) - F(0.999)) / (F(1) - F(0.9))), b1=F(0.9), b2=F(0.999), eps=F(1e-8))
BN_C = [1, 3, 64, 512, 513]
BN_STEPS = [1, 2, 1000]
BN_MOMENTUM = F(0.99)
SENTINEL = F(-12345.0)


def dense_inputs(B, K, N, seed=0):
    """Post-ReLU-like activations, He-scaled weights, a small bias, a gradient of the size a mean over B rows leaves."""
    rng = np.random.RandomState(1000 + seed + B + 7 * K + 13 * N)
    x = np.maximum(rng.standard_normal((B, K)), 0).astype(F)
    w = (rng.standard_normal((K, N)) * np.sqrt(2.0 / K)).astype(F)
    b = (0.1 * rng.standard_normal(N)).astype(F)
    dy = (rng.standard_normal((B, N)) / B).astype(F)
    return x, w, b, dy


def dense_delta_inputs(K, N):
    """x = e_k for the first and last k of every K slice; w an integer ramp / 8 and b integers / 8 (every sum exact in float32)."""
    ks = dense_slice_ends(K)
    x = np.zeros((len(ks), K), F)
    x[np.arange(len(ks)), ks] = 1
    w = ((np.arange(K * N).reshape(K, N) % 4093) - 2046).astype(F) / F(8)
    b = (np.arange(N) - N // 2).astype(F) / F(8)
    return ks, x, w, b


def softmax_inputs(B, soft=False):
    """-> logits, labels, kinds.  kinds[i]: 'tie', 'far' (a +-40 difference: both classes clipped), 'edge' (q within a few ulp of
    the clip threshold) or '' (logits uniform in [-4, 4], at least 1e-3 apart).  The special rows come first, as many as the
    1 % cap on rows that may be left out of the gradient comparison allows: 'far' and 'edge' rows are such rows ('far' because the
    larger q, 1 to within rounding, lies within its error of 1 - 1e-7)."""
    rng = np.random.RandomState(77 + B + (1000 if soft else 0))
    z = rng.uniform(-4, 4, size=(B, 2)).astype(F)
    close = np.abs(z[:, 0] - z[:, 1]) < 1e-3
    z[close, 1] = z[close, 0] + F(0.5)
    kinds = [''] * B
    special = []
    if B >= 2:
        special.append(('tie', (F(0.75), F(0.75))))
    cap = B // 100
    thr = np.log(f64(CE_EPS) / (1 - f64(CE_EPS)))          # z0 - z1 at which q0 = 1e-7
    far = [('far', (F(-20.0), F(20.0))), ('far', (F(21.5), F(-18.5)))]
    edge = [('edge', (np.nextafter(F(thr), F(0)), F(0.0))), ('edge', (F(0.0), np.nextafter(F(thr), F(-100)))),
            ('edge', (F(thr), F(0.0))), ('edge', (F(0.0), np.nextafter(F(thr), F(0))))]
    mix = [far[0], edge[0], far[1], edge[1], edge[2], edge[3]]
    special += mix[:cap]
    for i, (kind, zz) in enumerate(special):
        z[i] = zz
        kinds[i] = kind
    lab = rng.randint(0, 2, size=B)
    t = np.stack([lab, 1 - lab], axis=1).astype(F)
    if soft:
        t[:] = (F(0.3), F(0.7))
    return z, t, kinds


def sumsq_inputs():
    """One base buffer and 24 ranges: lengths 1-4 at every offset mod 4 (n < head included), 5, 255 (magnitudes 1e-3 .. 1e3),
    1024 (He-normal, and one of exact zeros), 65536 + 3 and 9 * 512 * 512.  -> base, off, n, index of the zero range."""
    rng = np.random.RandomState(5)
    spec = [(n, m) for n in (1, 2, 3, 4) for m in range(4)]
    spec += [(5, 1), (5, 3), (255, 1), (1024, 2), (1024, 3), (65536 + 3, 1), (65536 + 3, 2), (9 * 512 * 512, 0)]
    assert len(spec) == SUMSQ_MAX_SEGS
    off, pos = [], 5
    for n, m in spec:
        pos += (m - pos) % 4
        off.append(pos)
        pos += n + 1
    base = (rng.standard_normal(pos + 3) * np.sqrt(2.0 / (9 * 512))).astype(F)
    i255, izero = spec.index((255, 1)), spec.index((1024, 3))
    base[off[i255]:off[i255] + 255] = (10.0 ** rng.uniform(-3, 3, 255) * rng.choice([-1, 1], 255)).astype(F)
    base[off[izero]:off[izero] + 1024] = 0
    return base, np.array(off, np.int64), np.array([n for n, _ in spec], np.int64), izero


def adam_inputs(n, warm, seed=0):
    """p He-like, g ~ 1e-3 (|g| >= 1e-12), about a tenth of the elements with g = 0 and m = v = 0; warm: m ~ 1e-3, v ~ 1e-6."""
    rng = np.random.RandomState(300 + n + seed + (1 if warm else 0))
    p = 0.05 * rng.standard_normal(n)
    p = (np.sign(p) * np.maximum(np.abs(p), 0.01)).astype(F)      # |p| >= 0.01: the decay of any one element is visible
    g = 1e-3 * rng.standard_normal(n)
    g = (np.sign(g) * np.maximum(np.abs(g), 1e-12)).astype(F)
    still = rng.uniform(size=n) < 0.1
    still[-1] = True
    g[still] = 0
    m = (1e-3 * rng.standard_normal(n)).astype(F) if warm else np.zeros(n, F)
    v = np.maximum(1e-6 * rng.standard_normal(n) ** 2, 1e-12).astype(F) if warm else np.zeros(n, F)
    m[still] = 0
    v[still] = 0
    return p, g, m, v, still


def adam_l2_counts(n):
    return sorted(set([0, 1, n // 2, n]))


def bn_inputs(replicas, seed=0):
    """A table over BN_C: slots of C + 3 floats (sentinels behind each C), moving / biased / batch vectors, and for replicas > 1 a
    gathered buffer of stride packed size + 7 whose replica slots all differ (and differ from the batch vectors).
    -> dict(c, slot_off, n_slots, moving, biased, batch, gathered, stride, packed_off)"""
    rng = np.random.RandomState(900 + replicas + seed)
    c = np.array(BN_C, np.int32)
    slot_off = np.concatenate([[0], np.cumsum(c + 3)[:-1]]).astype(np.int64)
    n_slots = int((c + 3).sum())
    bufs = [np.full(n_slots, SENTINEL, F) for _ in range(3)]
    for i, (C, so) in enumerate(zip(c, slot_off)):
        bufs[0][so:so + C] = (1.0 + 0.5 * rng.standard_normal(C)).astype(F)
        bufs[1][so:so + C] = (0.01 * rng.standard_normal(C)).astype(F)
        bufs[2][so:so + C] = (0.3 * i + rng.standard_normal(C)).astype(F)
    total = int(c.sum())
    packed_off = np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int64)
    gathered, stride = None, 0
    if replicas > 1:
        stride = total + 7
        gathered = np.full((replicas - 1) * stride + total + 2, SENTINEL, F)
        for r in range(replicas):
            gathered[r * stride:r * stride + total] = (10.0 * (r + 1) + rng.standard_normal(total)).astype(F)
    return dict(c=c, slot_off=slot_off, n_slots=n_slots, moving=bufs[0], biased=bufs[1], batch=bufs[2], gathered=gathered,
                stride=stride, packed_off=packed_off, total=total)


def bn_values(d, i, replicas):
    """(replicas, C) updates of entry i as the kernel must read them."""
    C, so, po = int(d['c'][i]), int(d['slot_off'][i]), int(d['packed_off'][i])
    if d['gathered'] is None:
        return d['batch'][so:so + C][None, :]
    return np.stack([d['gathered'][r * d['stride'] + po:r * d['stride'] + po + C] for r in range(replicas)])
