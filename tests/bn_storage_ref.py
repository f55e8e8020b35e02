"""float64 reference, criteria, cases and an fp32 yardstick for the BatchNorm kernels of bn_fused.hip in their storage forms.

The kernels (bn_stats_fast, bn_apply_fast, bn_relu_pool2_fwd, bn_bwd_fast) read x and dy as fp32 or bfloat16 and write y / p / dx
as fp32 or bfloat16.  Here:
  * plain_ref / pooled_ref: the operation in float64 from oracle.l3_oracle's unfused ops.  Inputs flagged bf16 are rounded
    first, the mathematics is float64, outputs come back UNROUNDED (the criteria below know about the store).
  * stored_ok / check: the criteria.  An fp32-stored tensor: max |err| < TOL of the reference's range (test_layer_parity_gpu).  A
    bf16-stored one: test_conv_layer_bf16_stored_output's -- every value a bfloat16 within half a spacing + TOL of the range of
    the float64 value, and at most NOT_NEAREST_CAP of the elements not THE nearest bfloat16.
  * plain_case / pooled_case: deterministic inputs of the layer tests' distributions with planted edges (an exact tie between
    the (0,1) and (1,0) elements of one window; exact 0.0 and -0.0 inputs in mode 2) and an unambiguity margin: no ReLU gate
    closer than MARGIN of the range to zero, no two distinct candidates of a window closer than MARGIN of the range, so that
    fp32 arithmetic cannot legitimately choose another mask or winner than float64 does.
  * plain_f32 / pooled_f32: the kernels' formulas restated in NumPy -- fp32 element arithmetic, float64 column sums -- with
    named mutants.  A yardstick only: the host test shows that it passes every criterion and that each mutant fails the one
    named for it; where a shape legitimately exceeds TOL its error against float64 (times 4) is the bound.

ReLU placement: plain 0 none / 1 BN -> ReLU; pooled 1 pool(relu(bn(x))) / 2 pool(bn(relu(x))) (vision_model.py:137-139).
"""
import functools

import numpy as np

from oracle import l3_oracle as o

TOL = 3e-6                  # test_layer_parity_gpu.TOL
NOT_NEAREST_CAP = 1e-3      # test_conv_layer_bf16_stored_output
MARGIN = 1e-4
EPS32 = np.float32(1e-3)    # what the operators pass to the kernels
F32, F64 = np.float32, np.float64

# ---- the cases of test_bn_storage_gpu.py -------------------------------------------------------------------------------------
# plain (rows, C): 2.6 tiles of the bf16 apply with a partial last tile; C4 = 1; C = 8; C4 = FB (every thread writes partials);
# one row (variance 0)
PLAIN_SHAPES = [(333, 64), (77, 4), (50, 8), (9, 1024), (1, 16)]
# 2.56 M channel quads > FAST_MAX_BLOCKS * FB * 8 = 2 097 152: the capped grids of the statistics and both backward kernels
PLAIN_BIG = (40000, 256)
# pooled (N, H, W, C, same): both sizes odd (clipped last row / column, under one block); the same 'valid' (leftover row and
# column); 9.56 blocks of FB * U windows; every window clipped in one direction (twice); a single window; C4 = FB
POOL_SHAPES = [(3, 9, 7, 16, 1), (3, 9, 7, 16, 0), (2, 17, 33, 64, 1), (2, 1, 5, 8, 1), (2, 5, 1, 8, 1), (1, 2, 2, 4, 0),
               (5, 3, 4, 1024, 1)]
# 4.29 M input quads, 1.06 M window quads (520 blocks of the reduction, 529 of the backward apply: below the cap of 1024)
POOL_BIG = (2, 130, 129, 512, 0)
# 2 129 920 window quads (reduction) and 2 163 200 cells (backward apply) > 2 097 152: the capped pooled grids
POOL_CAPPED = (2, 130, 129, 1024, 0)
# The three big cases have 10 M, 17 M and 34 M elements: their float64 reference covers subset_channels(C), 64 channels, only.
# BatchNorm and the pool are per channel, so those channels' sums run through every block and every pass of the grid-stride
# loops and their elements lie in every tile; the bit-exact tier of the GPU test covers every element.
BIG_CASES = [('plain', PLAIN_BIG, 1), ('pooled', POOL_BIG, 1), ('pooled', POOL_BIG, 2), ('pooled', POOL_CAPPED, 1),
             ('pooled', POOL_CAPPED, 2)]                                # (kind, shape, relu / mode)
ODD_SAME = [s for s in POOL_SHAPES if s[4] and (s[1] % 2 or s[2] % 2)]
PLAIN_CASES = [(s, 1) for s in PLAIN_SHAPES] + [((50, 8), 0)]          # (shape, relu)
POOL_CASES = [(s, m) for s in POOL_SHAPES for m in (1, 2)]             # (shape, mode)
FORMS = [(xb, db) for xb in (False, True) for db in (False, True)]     # (x is bf16, dy is bf16)


def tag(shape):
    return 'x'.join(map(str, shape))


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def _as64(a, bf16):
    a = np.asarray(a, F32)
    return (o.bf16_round(a) if bf16 else a).astype(F64)


def pool_out(h, same):
    return -(-h // 2) if same else (h - 2) // 2 + 1


def windows(a, fill):
    """(N, ceil(H/2), ceil(W/2), 4, C): the 2x2 cells of a in row-major element order, `fill` outside the tensor."""
    n, h, w, c = a.shape
    win = np.full((n, -(-h // 2), -(-w // 2), 4, c), fill, a.dtype)
    for k, (i, j) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        s = a[:, i::2, j::2]
        win[:, :s.shape[1], :s.shape[2], k] = s
    return win


def unwindow(win, h, w):
    """Inverse of windows(): the in-tensor elements of the cells back in (N, H, W, C)."""
    n, _, _, _, c = win.shape
    a = np.empty((n, h, w, c), win.dtype)
    for k, (i, j) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        s = a[:, i::2, j::2]
        s[...] = win[:, :s.shape[1], :s.shape[2], k]
    return a


def _range(a):
    return float(a.max() - a.min())


def _gap_margin(v):
    """v (N, Ho, Wo, 4, C) with -inf outside: the smallest gap between a window's best and its best DISTINCT other candidate, per
    window (inf where there is none)."""
    best = v.max(3, keepdims=True)
    second = np.where(v < best, v, -np.inf).max(3, keepdims=True)
    return (best - second)[:, :, :, 0]


# ---- float64 reference ---------------------------------------------------------------------------------------------------------
def plain_ref(x, gamma, beta, dy, relu, x_bf16=False, dy_bf16=False):
    """BN(+ReLU) over (rows, C), batch statistics, and its backward when dy is given."""
    x64, g64, b64 = _as64(x, x_bf16), np.asarray(gamma, F32).astype(F64), np.asarray(beta, F32).astype(F64)
    c = x64.shape[-1]
    pre, cache = o.bn_fwd(x64, g64, b64, None, None, True)
    out = dict(y=np.maximum(pre, 0) if relu else pre, mean=cache[2], var=cache[3], win_margin=np.inf,
               relu_margin=float(np.abs(pre).min() / max(_range(pre), 1e-300)) if relu else np.inf)
    if dy is not None:
        d = _as64(dy, dy_bf16)
        dz = np.where(pre > 0, d, 0.0) if relu else d
        out['dx'], out['dgamma'], out['dbeta'] = o.bn_bwd(dz, g64, cache, True)
        # the largest term of dx = g rstd (dz - dbeta / n - xhat dgamma / n): the scale of its rounding error where the terms
        # cancel altogether (one row: dx is identically 0)
        out['dx_terms'] = float(np.abs(g64 * cache[1] * dz.reshape(-1, c)).max())
    return out


def pooled_ref(x, gamma, beta, dp, same, mode, x_bf16=False, dy_bf16=False):
    """The Conv -> BN -> ReLU -> MaxPool(2,2) tail (mode 1) / Conv -> ReLU -> BN -> MaxPool (mode 2) behind the convolution, its
    window winners (the input element, rectified in mode 2, whose BatchNorm(-ReLU) is the pooled value: first maximum in row-major
    order) and its backward from the pooled gradient dp; dbias is the column sum of dx."""
    x64, g64, b64 = _as64(x, x_bf16), np.asarray(gamma, F32).astype(F64), np.asarray(beta, F32).astype(F64)
    n, h, w, c = x64.shape
    pad = 'same' if same else 'valid'
    xin = np.maximum(x64, 0) if mode == 2 else x64
    pre, cache = o.bn_fwd(xin, g64, b64, None, None, True)
    cand = np.maximum(pre, 0) if mode == 1 else pre                     # what the pool compares
    p, pc = o.maxpool_fwd(cand, 2, 2, 2, 2, pad)
    ho, wo = p.shape[1:3]
    xwin = np.take_along_axis(windows(xin, 0.0)[:, :ho, :wo], pc[0][:, :, :, None, :].astype(np.int64), 3)[:, :, :, 0]
    rng_c = max(_range(cand), 1e-300)
    out = dict(p=p, xwin=xwin, mean=cache[2], var=cache[3],
               relu_margin=float(np.abs(pre).min() / max(_range(pre), 1e-300)) if mode == 1 else np.inf,
               win_margin=float(_gap_margin(windows(cand, -np.inf)[:, :ho, :wo]).min() / rng_c))
    if dp is not None:
        d = o.maxpool_bwd(_as64(dp, dy_bf16), pc)
        if mode == 1:
            dx, dg, db = o.bn_bwd(np.where(cand > 0, d, 0.0), g64, cache, True)
        else:
            dr, dg, db = o.bn_bwd(d, g64, cache, True)
            dx = np.where(x64 > 0, dr, 0.0)
        out.update(dx=dx, dgamma=dg, dbeta=db, dbias=dx.reshape(-1, c).sum(0))
    return out


# ---- criteria ----------------------------------------------------------------------------------------------------------------
def relerr(got, exact, scale=None):
    got, exact = np.asarray(got, F64), np.asarray(exact, F64)
    s = np.abs(exact).max() if scale is None else scale
    return float(np.abs(got - exact).max() / (s + 1e-300))


def stored_ok(got, exact, tol, scale=None):
    """test_conv_layer_bf16_stored_output's criterion.  Returns (ok, worst (|got - exact| - half a bfloat16 spacing) / range, share of
    the elements that are not the bfloat16 nearest to exact)."""
    got, exact = np.asarray(got, F32).astype(F64), np.asarray(exact, F64)
    s = (np.abs(exact).max() if scale is None else scale) + 1e-300
    with np.errstate(invalid='ignore', over='ignore'):
        is_bf16 = np.array_equal(o.bf16_round(got), got)
        half = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(exact), np.abs(got)) + 1e-300)) - 8)
        excess = float((np.abs(got - exact) - half).max() / s)
    share = float((got != o.bf16_round(exact)).mean())
    return bool(is_bf16 and excess <= tol), excess, share


def check(got, ref, stored=(), tol=None):
    """Every criterion on one call's outputs: {name: (ok, figure)}.  got: the tensors by name (y / p / dx, xwin, mean, var,
    dgamma, dbeta, dbias); stored: which of them were stored as bfloat16; tol: per-name overrides of TOL."""
    tol = tol or {}
    res = {}
    for k, v in got.items():
        t = tol.get(k, TOL)
        # an identically zero reference (dx of a one-row BatchNorm): relative to the largest of the terms that cancel
        scale = ref['dx_terms'] if k == 'dx' and 'dx_terms' in ref and not np.any(ref['dx']) else None
        if k == 'xwin':
            res['xwin'] = (bool(np.array_equal(np.asarray(v, F64), ref['xwin'])), float((np.asarray(v, F64) != ref['xwin']).mean()))
        elif k == 'dbias':
            # test_bn_relu_pool_tail_layer's bound: the column sum of dx (analytically 0 in BN -> ReLU order)
            bound = 1e-4 * np.abs(ref['dx']).sum(axis=(0, 1, 2)).max() + 1e-7
            e = float(np.abs(np.asarray(v, F64) - ref['dbias']).max())
            res['dbias'] = (e < bound, e / bound)
        elif k in stored:
            ok, excess, share = stored_ok(v, ref[k], t, scale)
            res['stored_ok:' + k] = (ok, excess)
            if scale is None:       # around an exact 0 there is no nearest bfloat16 to miss: rounding noise of either sign is all there is
                res['nearest_share:' + k] = (share < NOT_NEAREST_CAP, share)
        else:
            e = relerr(v, ref[k], scale)
            res['relerr:' + k] = (e < t, e)
    return res


def failures(res):
    return sorted(k for k, (ok, _) in res.items() if not ok)


# ---- cases -------------------------------------------------------------------------------------------------------------------
def subset_channels(c):
    """64 channels spread over all of c (a multiple of 64) and over the four lanes of a channel quad."""
    step = c // 64
    return np.array([step * k + k % step for k in range(64)])


def _draw_x(rng, shape, x_bf16):
    x = rng.standard_normal(shape, dtype=F32) * F32(1.5) + F32(0.3)
    return o.bf16_round(x) if x_bf16 else x


def _case(shape, pool, mode, x_bf16, chans):
    """x, gamma, beta of one case and its margins {relu_margin, win_margin}.  Elements that break a margin are drawn again from
    the same stream (a tensor of 10^5 elements and more has some in every draw: |pre-activation| < 1e-4 of the range has
    probability ~6e-4 per element); a case that six rounds do not settle moves to the next seed.  Planted elements are never
    redrawn.  chans: the margins hold (and are repaired) on these channels only -- the ones a float64 reference will cover."""
    c = shape[-1]
    for seed in range(100):
        rng = np.random.default_rng([20180123, sum(shape), mode, int(x_bf16), seed])
        x = _draw_x(rng, shape, x_bf16)
        gamma = (1 + 0.1 * rng.standard_normal(c)).astype(F32)
        beta = (0.1 * rng.standard_normal(c)).astype(F32)
        frozen = np.zeros(shape, bool)
        if pool and shape[1] >= 2 and shape[2] >= 2:
            # an exact tie of the window maximum between elements (0,1) and (1,0): the first in row-major order must win
            n0, i0, j0, c0 = shape[0] - 1, (shape[1] // 2 - 1) * 2, (shape[2] // 2 - 1) * 2, c - 3
            x[n0, i0, j0 + 1, c0] = x[n0, i0 + 1, j0, c0] = 8.0
            frozen[n0, i0, j0 + 1, c0] = frozen[n0, i0 + 1, j0, c0] = True
        if pool and mode == 2:
            # exact zeros of both signs at the ReLU in front of the BatchNorm: `> 0` lets neither pass a gradient
            idx = np.unique(rng.integers(0, x.size, min(8, x.size // 4)))
            idx = idx[~frozen.reshape(-1)[idx]]
            x.reshape(-1)[idx] = np.where(np.arange(idx.size) % 2 == 0, 0.0, -0.0).astype(F32)
            frozen.reshape(-1)[idx] = True
        view = (lambda a: a) if chans is None else (lambda a: a[..., chans])
        g64, b64 = view(gamma).astype(F64), view(beta).astype(F64)
        for _ in range(6):
            xs = view(x)
            xin = np.maximum(xs, 0).astype(F64) if pool and mode == 2 else xs.astype(F64)
            pre = o.bn_fwd(xin, g64, b64, None, None, True)[0]
            m = dict(relu_margin=np.inf, win_margin=np.inf)
            bad = np.zeros(xs.shape, bool)
            if mode == 1:
                m['relu_margin'] = float(np.abs(pre).min() / max(_range(pre), 1e-300))
                bad |= np.abs(pre) < 1.5 * MARGIN * _range(pre)
            if pool:
                cand = np.maximum(pre, 0) if mode == 1 else pre
                ho, wo = pool_out(shape[1], pool[0]), pool_out(shape[2], pool[0])
                gaps = _gap_margin(windows(cand, -np.inf))
                gaps[:, ho:] = np.inf                                    # 'valid' leftover cells are no windows
                gaps[:, :, wo:] = np.inf
                m['win_margin'] = float(gaps.min() / max(_range(cand), 1e-300))
                near = gaps < 1.5 * MARGIN * _range(cand)
                bad |= unwindow(np.broadcast_to(near[:, :, :, None, :], near.shape[:3] + (4, near.shape[3])), *xs.shape[1:3])
            if m['relu_margin'] > MARGIN and m['win_margin'] > MARGIN:
                return x, gamma, beta, m
            bad &= ~view(frozen)
            fresh = _draw_x(rng, (int(bad.sum()),), x_bf16)
            if chans is None:
                x[bad] = fresh
            else:
                sub = x[..., chans]
                sub[bad] = fresh
                x[..., chans] = sub
    raise AssertionError('no seed meets the margins: %r' % (shape,))


@functools.lru_cache(maxsize=None)
def plain_case(shape, relu, x_bf16, big=False):
    """(x, gamma, beta, margins) -- read-only, shared by the tests.  big: margins on subset_channels(C) only."""
    out = _case(tuple(shape), None, relu, x_bf16, subset_channels(shape[-1]) if big else None)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pooled_case(shape, mode, x_bf16, big=False):
    out = _case(tuple(shape[:4]), (shape[4],), mode, x_bf16, subset_channels(shape[3]) if big else None)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def gradient(shape, dy_bf16, salt=0):
    """The incoming gradient dy / dp: 1e-3 N(0,1), bfloat16-valued when it arrives so."""
    rng = np.random.default_rng([7, sum(shape), salt])
    dy = rng.standard_normal(shape, dtype=F32) * F32(1e-3)
    return o.bf16_round(dy) if dy_bf16 else dy


# ---- the kernels' formulas in fp32 NumPy, with mutants ---------------------------------------------------------------------------
MUTANTS = {
    # name: (the criteria that must reject it, what it is)
    'truncate': (('stored_ok', 'nearest_share'), 'the bf16 store truncates instead of rounding to nearest even'),
    'last_max': (('xwin', 'relerr:dx', 'stored_ok:dx'), 'the last maximum of a window wins instead of the first'),
    'clip_col_shift': (('relerr:dx', 'stored_ok:dx'), "the dx of a clipped window's second column is written to the next cell"),
    'valid_leftover_grad': (('relerr:dx', 'stored_ok:dx'), "'valid' leftover cells are given gradient"),
    'gate_ge': (('relerr:dx', 'stored_ok:dx'), 'the mode-2 gate is x >= 0'),
    'relu_after_pool': (('relerr:p', 'stored_ok:p', 'relerr:dx', 'stored_ok:dx'), 'mode 2 rectifies the pooled value as mode 1 does'),
    'dy_as_f32': (('relerr:dx', 'stored_ok:dx'), 'a bfloat16 dy is read as fp32'),
}


def _fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)       # an exact product, one rounding


def _store(v, obf, mutant):
    if not obf:
        return v
    if mutant == 'truncate':
        return (np.ascontiguousarray(v, F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    return o.bf16_round(v)


def _load(a, bf16, mutant=None):
    a = np.ascontiguousarray(a, F32)
    if not bf16:
        return a
    a = o.bf16_round(a)
    if mutant == 'dy_as_f32':           # the 16-bit buffer taken for floats (zeros behind it)
        bits = (a.view(np.uint32) >> np.uint32(16)).astype(np.uint16).reshape(-1)
        return np.concatenate([bits, np.zeros_like(bits)]).view(F32).reshape(a.shape)
    return a


def _stats_f32(xin, gamma, beta):
    """StatFinal over bn_stats_fast_kernel's sums about row 0: mean, var, scale, shift (fp32)."""
    x2 = xin.reshape(-1, xin.shape[-1])
    d = x2 - x2[0]
    s0, s1 = d.sum(0, dtype=F64), (d * d).sum(0, dtype=F64)
    dm = s0 / x2.shape[0]
    v = np.maximum(s1 / x2.shape[0] - dm * dm, 0.0)
    m = x2[0].astype(F64) + dm
    sc = gamma.astype(F64) / np.sqrt(v + F64(EPS32))
    return m.astype(F32), v.astype(F32), sc.astype(F32), (beta.astype(F64) - m * sc).astype(F32)


def _bwd_coeffs(s0, s1, gamma, mean, var, rows):
    """BwdFinal: dgamma, dbeta and dx = A dz + B x + C."""
    rstd = 1.0 / np.sqrt(var.astype(F64) + F64(EPS32))
    gr = gamma.astype(F64) * rstd
    return (s1.astype(F32), s0.astype(F32), gr.astype(F32), (-gr * rstd * s1 / rows).astype(F32),
            (gr * (-s0 / rows + mean.astype(F64) * rstd * s1 / rows)).astype(F32))


def plain_f32(x, gamma, beta, dy, relu, x_bf16=False, dy_bf16=False, out_bf16=False, mutant=None):
    gamma, beta = np.asarray(gamma, F32), np.asarray(beta, F32)
    xv = _load(x, x_bf16)
    mean, var, sc, sh = _stats_f32(xv, gamma, beta)
    pre = _fma(xv, sc, sh)
    out = dict(y=_store(np.maximum(pre, 0) if relu else pre, out_bf16, mutant), mean=mean, var=var)
    if dy is not None:
        with np.errstate(all='ignore'):
            d = _load(dy, dy_bf16, mutant)
            if relu:
                d = np.where(pre > 0, d, F32(0))
            rs = (F32(1) / np.sqrt(var + EPS32)).astype(F32)
            c = xv.shape[-1]
            s0, s1 = d.reshape(-1, c).sum(0, dtype=F64), (d * ((xv - mean) * rs)).reshape(-1, c).sum(0, dtype=F64)
            dg, db, A, B, C = _bwd_coeffs(s0, s1, gamma, mean, var, xv.size // c)
            out.update(dx=_store(_fma(A, d, _fma(B, xv, C)), out_bf16, mutant), dgamma=dg, dbeta=db)
    return out


def pooled_f32(x, gamma, beta, dp, same, mode, x_bf16=False, dy_bf16=False, out_bf16=False, mutant=None):
    gamma, beta = np.asarray(gamma, F32), np.asarray(beta, F32)
    xr = _load(x, x_bf16)
    n, h, w, c = xr.shape
    ho, wo = pool_out(h, same), pool_out(w, same)
    xv = np.maximum(xr, 0) if mode == 2 else xr
    mean, var, sc, sh = _stats_f32(xv, gamma, beta)
    xw = windows(xv, F32(0))                                             # coverage grid (N, Hc, Wc, 4, C)
    inside = windows(np.ones((1, h, w, 1), bool), False)
    cand = _fma(xw, sc, sh)
    if mode == 1:
        cand = np.maximum(cand, 0)
    cand = np.where(inside, cand, F32(-np.inf))
    k = 3 - cand[:, :, :, ::-1].argmax(3) if mutant == 'last_max' else cand.argmax(3)       # argmax4: strict >, so the first
    k = k[:, :, :, None]
    best = np.take_along_axis(cand, k, 3)
    p = best[:, :ho, :wo, 0]
    if mode == 1 or mutant == 'relu_after_pool':
        p = np.maximum(p, 0)
    xk = np.take_along_axis(xw, k, 3)
    out = dict(p=_store(p, out_bf16, mutant), xwin=xk[:, :ho, :wo, 0], mean=mean, var=var)
    if dp is not None:
        with np.errstate(all='ignore'):
            d = _load(dp, dy_bf16, mutant)
            dcell = np.zeros(best.shape, F32)                           # 'valid' leftover cells receive no gradient
            dcell[:, :ho, :wo, 0] = d
            if mutant == 'valid_leftover_grad':
                dcell[:, :, :, 0] = np.pad(d, ((0, 0), (0, best.shape[1] - ho), (0, best.shape[2] - wo), (0, 0)), mode='edge')
            gate = F32(-np.inf) if mode == 2 and mutant != 'relu_after_pool' else F32(0)
            dk = np.where(best > gate, dcell, F32(0))
            live = dk[:, :ho, :wo, 0]
            rs = (F32(1) / np.sqrt(var + EPS32)).astype(F32)
            s0 = live.reshape(-1, c).sum(0, dtype=F64)
            s1 = (live * ((xk[:, :ho, :wo, 0] - mean) * rs)).reshape(-1, c).sum(0, dtype=F64)
            dg, db, A, B, C = _bwd_coeffs(s0, s1, gamma, mean, var, n * h * w)
            dz = np.where(np.arange(4)[None, None, None, :, None] == k, dk, F32(0))
            ow = _fma(A, dz, _fma(B, xw, C))
            if mode == 2:
                rw = windows(xr, F32(0))
                ow = np.where(rw >= 0 if mutant == 'gate_ge' else rw > 0, ow, F32(0))
            dx = unwindow(ow, h, w)
            if mutant == 'clip_col_shift' and w % 2:
                # the (0,1) store of a window clipped in W, not suppressed: the clamped tap's value lands one pixel further on
                stray = _fma(A, F32(0), _fma(B, xv[:, 0::2, w - 1], C))
                if mode == 2:
                    stray = np.where(xr[:, 0::2, w - 1] > 0, stray, F32(0))
                flat = dx.reshape(-1, c)
                pix = (np.arange(n)[:, None] * h + np.arange(0, h, 2)[None, :]) * w + w
                okp = pix < flat.shape[0]
                flat[pix[okp]] = stray[okp]
            out.update(dx=_store(dx, out_bf16, mutant), dgamma=dg, dbeta=db, dbias=dx.reshape(-1, c).sum(0, dtype=F64).astype(F32))
    return out
