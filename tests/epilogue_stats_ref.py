"""The yardstick of the conv-epilogue BatchNorm partials (test_conv_epilogue_stats_gpu.py, test_conv_epilogue_stats_host.py): input
builders, the float64 terms of every sum an epilogue leaves, and the criterion the sums are held to.

A convolution's epilogue leaves, per block of its output, [sum t, sum t^2] of t = y - pivot (stat_mode 1) or relu(y) - pivot
(stat_mode 2) for the BatchNorm behind it -- pivot = bias[c] as the kernels take it: relu(bias[c]) in mode 2, what
bn_stats_from_partials adds back --, and a data gradient's epilogue leaves [sum m dx, sum m dx x_hat] for the BatchNorm in front.
The reference is always float64 NumPy over the tensor the kernel itself returned, so only the epilogue's summation is judged:

    | sum over blocks of the partials - S |  <=  TOL * sum |term|        per channel, TOL = 3e-6

3e-6 is TOL of test_layer_parity_gpu.py, the bound the unfused kernels of the same reductions meet there (against the range of
the result); normalising by the sum of magnitudes is the forward-error measure of a sum and is no tighter.  mean is judged
against mean |t|, var against mean t^2, dgamma / dbeta against the magnitudes of their own terms."""
import numpy as np

from oracle import l3_oracle as o

TOL = 3e-6
TOL_F4 = 3e-5          # y / dx of the F(4x4,3x3) kernel against the oracle (test_layer_parity_gpu.py)
BN_EPS = 1e-3
MASK_MARGIN = 1e-3     # no BatchNorm pre-activation closer to 0: the recomputed ReLU mask is unambiguous

# ---- the cases: (N, H, W, Cin, Cout), all 3x3 'same' ------------------------------------------------------------------------------
F4_SHAPES = [(3, 13, 18, 16, 64), (2, 9, 7, 24, 128), (5, 30, 21, 72, 64), (4, 16, 16, 40, 192)]
# F(4x4,3x3) channel-sliced tail: (shape, L3_W4_NCU or None = the real chip).  Tile blocks = ceil(N ceil(H/4) ceil(W/4) / 32) * Cout / 64
# against a grid of NCU workgroups (conv_wino4.hip launch_wino4): 1 x 1 on >= 8 CUs -- all tail, one block over 16 slices; 2 x 2 = 4
# on 8 -- all tail, two slices each; 5 x 2 = 10 on 8 -- one full round and a tail of 2 blocks over 4 slices each.
F4_TAIL_CASES = [((2, 12, 12, 256, 64), None), ((4, 16, 16, 256, 128), '8'), ((6, 20, 20, 256, 128), '8')]
F2_SHAPES = [(3, 16, 18, 16, 64), (2, 17, 7, 32, 128), (7, 28, 28, 64, 64)]
BX6_SHAPES = [(5, 16, 40, 32, 64), (9, 18, 66, 32, 64)]
FIRST_SHAPES = [(2, 12, 10, 1, 64), (1, 5, 199, 1, 64), (3, 4, 33, 3, 64), (1, 40, 65, 3, 64)]
BF16_SHAPES = [(2, 9, 33, 64, 128), (1, 17, 15, 128, 256), (3, 5, 50, 64, 128), (2, 1, 1, 64, 128), (2, 9, 33, 64, 64)]
BF16_FLAT_SHAPES = [(5, 3, 4, 64, 128), (7, 6, 5, 64, 128), (3, 28, 28, 64, 128)]
BF16_VARIANTS = ['halo_auto', 'halo_pw32', 'halo_pw16', 'halo_2d', 'halo_flat', 'tap_tiles']
# (N, H, W, C, 'same' pooling): the BatchNorm-ReLU-MaxPool(2, 2) tails whose window winners feed the backward partials
POOL_CASES = [(2, 9, 7, 16, 1), (2, 9, 7, 16, 0), (3, 10, 11, 128, 1), (1, 199, 6, 64, 0)]


def bf16_variant_env(variant):
    """The knobs of test_conv_bf16_stored_random_geometries for the forward / data-gradient variants."""
    env = {'L3_BF16_HALO': '0' if variant == 'tap_tiles' else '1', 'L3_WG_TR': '1', 'L3_WG_TR_TS': '1'}
    if variant.startswith('halo_pw'):
        env['L3_HALO_PW'] = variant[-2:]
    if variant in ('halo_flat', 'halo_2d'):
        env['L3_HALO_FLAT'] = '0' if variant == 'halo_2d' else '2'
    return env


def bf16_shapes(variant):
    return BF16_SHAPES + (BF16_FLAT_SHAPES if variant == 'halo_flat' else [])


# ---- input builders (those of the tests the shapes come from) -------------------------------------------------------------------------
def conv_inputs(group, shape):
    """x, w, b as float32.  group: 'wino' (F4 / tail / F2 / bx6 / first layer: randn input, he_normal filter, small bias) or 'bf16'
    (post-ReLU input, bias of order one: test_conv_bf16_stored_random_geometries)."""
    n, h, w, ci, co = shape
    rng = np.random.RandomState((ci * 7 + co + 31 * h + 977 * w + n) % (2 ** 31))
    if group == 'bf16':
        x = np.maximum(rng.randn(n, h, w, ci), 0).astype(np.float32)
        wt = (rng.randn(3, 3, ci, co) / np.sqrt(9 * ci)).astype(np.float32)
        b = rng.randn(co).astype(np.float32)
    else:
        x = rng.randn(n, h, w, ci).astype(np.float32)
        wt = (rng.randn(3, 3, ci, co) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
        b = (0.1 * rng.randn(co)).astype(np.float32)
    return x, wt, b


def scale_shift(gamma, beta, mean, var):
    """bn_scale_shift: float64 from the float32 parameters, stored as float32."""
    g, bt, m, v = (np.asarray(t, np.float32).astype(np.float64) for t in (gamma, beta, mean, var))
    sc = g / np.sqrt(v + np.float64(np.float32(BN_EPS)))
    return sc.astype(np.float32), (bt - m * sc).astype(np.float32)


def near_zero_mask_count(bn_x, gamma, beta, mean, var):
    sc, sh = scale_shift(gamma, beta, mean, var)
    pre = bn_x.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)
    return int((np.abs(pre) < MASK_MARGIN).sum())


def bwd_inputs(dgrad_shape, bf16):
    """The operands of a data gradient whose OWN geometry (a convolution from Cin to Cout channels) is the listed one, i.e. of a
    forward convolution Cout -> Cin, and the BatchNorm(+ReLU) in front of that forward convolution: dy (N, H, W, Cin), the forward
    filter (3, 3, Cout, Cin), bn_x (N, H, W, Cout) with gamma, beta and its batch moments.  No element of bn_x lies within
    MASK_MARGIN of the ReLU threshold (offenders are pushed away from it; bf16: re-rounded and re-checked)."""
    n, h, w, ci, co = dgrad_shape
    rng = np.random.RandomState((ci * 13 + co * 3 + 31 * h + 977 * w + n + (5 if bf16 else 0)) % (2 ** 31))
    dy = rng.randn(n, h, w, ci).astype(np.float32)
    wt = (rng.randn(3, 3, co, ci) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
    bn_x = (rng.randn(n, h, w, co) * 1.5 + 0.3).astype(np.float32)
    gamma = (1 + 0.1 * rng.randn(co)).astype(np.float32)
    beta = (0.1 * rng.randn(co)).astype(np.float32)
    if bf16:
        dy, bn_x = o.bf16_round(dy), o.bf16_round(bn_x)
    mean = bn_x.astype(np.float64).reshape(-1, co).mean(0).astype(np.float32)
    var = bn_x.astype(np.float64).reshape(-1, co).var(0).astype(np.float32)
    bn_x = push_off_threshold(bn_x, gamma, beta, mean, var, bf16)
    return dy, wt, bn_x, gamma, beta, mean, var


def push_off_threshold(bn_x, gamma, beta, mean, var, bf16):
    """bn_x with every element whose pre-activation bn_x * scale + shift lies within MASK_MARGIN of 0 moved away from it (the
    moments are the caller's and stay: the operator takes them as given)."""
    sc, sh = scale_shift(gamma, beta, mean, var)
    sc64, sh64 = sc.astype(np.float64), sh.astype(np.float64)
    bn_x = bn_x.copy()
    for step in range(1, 9):
        pre = bn_x.astype(np.float64) * sc64 + sh64
        bad = np.abs(pre) < MASK_MARGIN
        if not bad.any():
            break
        # to a pre-activation of +-4 margins (bf16: further each time, until the rounded value clears the margin)
        target = np.where(pre >= 0, 1.0, -1.0) * 4 * MASK_MARGIN * step * (8 if bf16 else 1)
        moved = ((target - sh64) / sc64).astype(np.float32)
        moved = np.broadcast_to(moved, bn_x.shape)
        bn_x[bad] = (o.bf16_round(moved) if bf16 else moved)[bad]
    return bn_x


def pool_inputs(case, mode, bf16):
    """x (N, H, W, C), gamma, beta of a BatchNorm-ReLU-pool tail: one 2x2 window of equal values, one channel <= 0 everywhere, and
    (mode 1, where the backward mask is recomputed) no element within MASK_MARGIN of the ReLU threshold under its own batch moments."""
    n, h, w, c, same = case
    rng = np.random.RandomState(h * 7 + w + c + mode + (3 if bf16 else 0))
    x = (rng.randn(n, h, w, c) * 1.5 + 0.3).astype(np.float32)
    x[..., 1] = -np.abs(x[..., 1])
    x[0, 0:2, 0:2, 0] = 1.5
    x[0, 2:4, 0:2, 2] = [[1.5, 1.5], [2.5, 1.5]]          # ties below a winner that is not tied
    gamma = (1 + 0.1 * rng.randn(c)).astype(np.float32)
    beta = (0.1 * rng.randn(c)).astype(np.float32)
    if bf16:
        x = o.bf16_round(x)
    if mode == 1:
        for _ in range(4):          # a nudge moves the moments by ~1e-6 of themselves: settle
            mean = x.astype(np.float64).reshape(-1, c).mean(0).astype(np.float32)
            var = x.astype(np.float64).reshape(-1, c).var(0).astype(np.float32)
            sc, sh = scale_shift(gamma, beta, mean, var)
            pre = x.astype(np.float64) * sc + sh
            if not (np.abs(pre) < 2 * MASK_MARGIN).any():
                break
            tied = np.zeros(x.shape, bool)
            tied[0, 0:2, 0:2, 0] = tied[0, 2:4, 0:2, 2] = True
            keep = x.copy()
            x = push_off_threshold(x, gamma, beta, mean, var, bf16)
            x[tied] = keep[tied]
    return x, gamma, beta


# ---- the terms --------------------------------------------------------------------------------------------------------------------------
def fwd_pivot(bias, mode):
    b = np.asarray(bias, np.float32).astype(np.float64)
    return np.maximum(b, 0) if mode == 2 else b


def fwd_terms(y, bias, mode):
    """(rows, C) float64: t = y - pivot (mode 1) / relu(y) - pivot (mode 2) of the tensor the kernel returned."""
    y = np.asarray(y, np.float64).reshape(-1, np.shape(y)[-1])
    return (np.maximum(y, 0) if mode == 2 else y) - fwd_pivot(bias, mode)


def bwd_terms(dx, bn_x, gamma, beta, mean, var, relu):
    """(rows, C) float64 each: t0 = m dx, t1 = m dx (bn_x - mean) / sqrt(var + eps), m = (bn_x scale + shift > 0) if relu else 1."""
    c = np.shape(dx)[-1]
    dx = np.asarray(dx, np.float64).reshape(-1, c)
    bx = np.asarray(bn_x, np.float64).reshape(-1, c)
    sc, sh = scale_shift(gamma, beta, mean, var)
    m = (bx * sc.astype(np.float64) + sh.astype(np.float64) > 0) if relu else np.ones(bx.shape, bool)
    m64, v64 = np.asarray(mean, np.float32).astype(np.float64), np.asarray(var, np.float32).astype(np.float64)
    t0 = np.where(m, dx, 0.0)
    return t0, t0 * (bx - m64) / np.sqrt(v64 + np.float64(np.float32(BN_EPS)))


# ---- the criterion ----------------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))


def sum_ratio(got, terms):
    """Worst channel of |got - S| / (TOL * sum |term|): got (C,) or the (nblk, C) partials, terms (rows, C) float64.  <= 1 passes."""
    got = np.asarray(got, np.float64)
    if got.ndim == 2:
        got = got.sum(0)
    return _ratio(np.abs(got - terms.sum(0)), TOL * np.abs(terms).sum(0))


def partials_ratio(part, t0, t1):
    """The two rows of the (nblk, 2, C) partials against their terms."""
    part = np.asarray(part)
    assert part.ndim == 3 and part.shape[1] == 2 and np.isfinite(part).all()
    return max(sum_ratio(part[:, 0], t0), sum_ratio(part[:, 1], t1))


def moments_ratio(mean, var, terms, pivot, rows=None):
    """mean against mean |t|, var (biased) against mean t^2; rows: the divisor the reference uses (the tensor's own)."""
    rows = terms.shape[0] if rows is None else rows
    dm = terms.sum(0) / rows
    v = np.maximum((terms * terms).sum(0) / rows - dm * dm, 0)
    r_mean = _ratio(np.abs(np.asarray(mean, np.float64) - (pivot + dm)), TOL * np.abs(terms).sum(0) / rows)
    r_var = _ratio(np.abs(np.asarray(var, np.float64) - v), TOL * (terms * terms).sum(0) / rows)
    return max(r_mean, r_var)


# ---- honest float32 partials, for the host test that the yardstick bites ----------------------------------------------------------------
def f32_partials(t0, t1, block_rows=256):
    """float32 partials of the float32 terms, one block per block_rows rows, each block summed in float32 as a tree (NumPy's
    pairwise sum along a contiguous axis: short chains combined in halves, the shape of the kernels' lane / slot reductions; one
    chain of 256 adds of same-signed terms alone takes 0.6 of the bound)."""
    a0, a1 = np.ascontiguousarray(t0.astype(np.float32).T), np.ascontiguousarray(t1.astype(np.float32).T)
    nblk = (a0.shape[1] + block_rows - 1) // block_rows
    part = np.zeros((nblk, 2, a0.shape[0]), np.float32)
    for b in range(nblk):
        s = slice(b * block_rows, (b + 1) * block_rows)
        part[b, 0] = np.ascontiguousarray(a0[:, s]).sum(1, dtype=np.float32)
        part[b, 1] = np.ascontiguousarray(a1[:, s]).sum(1, dtype=np.float32)
    return part


# ---- the window winners of the pooled BatchNorm -----------------------------------------------------------------------------------------
def pool_windows(x, same):
    """(N, Ho, Wo, 4, C) window elements in row-major order and the (Ho, Wo, 4) mask of those inside the tensor."""
    n, h, w, c = x.shape
    ho, wo = (-(-h // 2), -(-w // 2)) if same else ((h - 2) // 2 + 1, (w - 2) // 2 + 1)
    win = np.zeros((n, ho, wo, 4, c), x.dtype)
    ok = np.zeros((ho, wo, 4), bool)
    for k, (dy, dx) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        ys, xs = 2 * np.arange(ho) + dy, 2 * np.arange(wo) + dx
        oky, okx = ys < h, xs < w
        ok[:, :, k] = oky[:, None] & okx[None, :]
        win[:, :, :, k][np.ix_(np.arange(n), np.nonzero(oky)[0], np.nonzero(okx)[0])] = x[:, ys[oky]][:, :, xs[okx]]
    return win, ok


def bn_of(v, gamma, beta, mean, var):
    g, bt, m, s = (np.asarray(t, np.float32).astype(np.float64) for t in (gamma, beta, mean, var))
    return (np.asarray(v, np.float64) - m) / np.sqrt(s + np.float64(np.float32(BN_EPS))) * g + bt


def pool_reference(x, gamma, beta, mean, var, mode, same):
    """p and the winners in float64 arithmetic: first maximum in row-major order of the values the pool compares (mode 1: the
    post-ReLU BatchNorm outputs; mode 2: the BatchNorm outputs of the rectified inputs, the element kept is the rectified one)."""
    xin = np.maximum(x, 0) if mode == 2 else x
    win, ok = pool_windows(xin.astype(np.float64), same)
    v = bn_of(win, gamma, beta, mean, var)
    if mode == 1:
        v = np.maximum(v, 0)
    v = np.where(ok[None, :, :, :, None], v, -np.inf)
    k = v.argmax(3)
    return v.max(3), np.take_along_axis(win, k[:, :, :, None, :], 3)[:, :, :, 0, :]


def xwin_faults(xwin, p, x, gamma, beta, mean, var, mode, same):
    """The two checks of the winner tensor: (count of elements that are none of their window's in-bounds inputs -- mode 2: the
    rectified ones --, worst |BatchNorm(-ReLU) of the element in float64 - p| / (TOL * range of p))."""
    xin = np.maximum(x, 0) if mode == 2 else x
    win, ok = pool_windows(np.asarray(xin, np.float64), same)
    member = ((win == np.asarray(xwin, np.float64)[:, :, :, None, :]) & ok[None, :, :, :, None]).any(3)
    v = bn_of(xwin, gamma, beta, mean, var)
    if mode == 1:
        v = np.maximum(v, 0)
    p = np.asarray(p, np.float64)
    return int((~member).sum()), float(np.abs(v - p).max() / (TOL * (p.max() - p.min())))
