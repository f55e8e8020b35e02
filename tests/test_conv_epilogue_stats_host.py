"""The yardstick of test_conv_epilogue_stats_gpu.py bites (no GPU): on the same input builders, honest float32 partials of the
oracle's tensors pass the criterion of epilogue_stats_ref.py with room to spare, and every fault the GPU test exists to catch --
a pixel dropped, an out-of-image pixel of a ragged tile let in, a zero row of a flat tile counted, the bias added before the
moments, unrounded instead of bf16-rounded values, the ReLU mask taken from the wrong tensor, the wrong element of a window
recorded as its winner -- fails it, on the smallest and the largest case of every group."""
import functools

import numpy as np
import pytest

import epilogue_stats_ref as R
from oracle import l3_oracle as o

FWD_GROUPS = {
    'f4': ('wino', R.F4_SHAPES), 'f4_tail': ('wino', [c[0] for c in R.F4_TAIL_CASES]), 'f2': ('wino', R.F2_SHAPES),
    'bx6': ('wino', R.BX6_SHAPES), 'first': ('wino', R.FIRST_SHAPES), 'bf16': ('bf16', R.BF16_SHAPES + R.BF16_FLAT_SHAPES)}
BWD_GROUPS = {
    'f4': (False, R.F4_SHAPES[:3]), 'f4_tail': (False, [(2, 12, 12, 256, 64)]), 'f2': (False, R.F2_SHAPES[:2]),
    'bf16': (True, R.BF16_SHAPES + R.BF16_FLAT_SHAPES)}


def _ends(shapes):
    by_rows = sorted(shapes, key=lambda s: s[0] * s[1] * s[2])
    return [by_rows[0]] if len(by_rows) == 1 else [by_rows[0], by_rows[-1]]


FWD_CASES = [(g, s) for g in FWD_GROUPS for s in _ends(FWD_GROUPS[g][1])]
BWD_CASES = [(g, s) for g in BWD_GROUPS for s in _ends(BWD_GROUPS[g][1])]


@functools.lru_cache(maxsize=None)
def _fwd(group, shape):
    """The oracle's y (float64 arithmetic, stored as float32 as a kernel returns it) and the value the convolution takes one pixel
    to the right of image 0's first row: what a ragged tile computes there and must not count."""
    builder = FWD_GROUPS[group][0]
    x, wt, b = R.conv_inputs(builder, shape)
    x64, w64, b64 = (t.astype(np.float64) for t in (x, wt, b))
    with o.mixed_precision('bf16' if builder == 'bf16' else None):
        y = o.conv2d_fwd(x64, w64, b64, 'same')
        outside = o.conv2d_fwd(np.pad(x64[:1], ((0, 0), (0, 0), (0, 1), (0, 0))), w64, b64, 'same')[0, 0, -1]
    return y.astype(np.float32), b, outside.astype(np.float32)


def _moments_from(part, pivot, rows):
    s0, s1 = part[:, 0].astype(np.float64).sum(0), part[:, 1].astype(np.float64).sum(0)
    dm = s0 / rows
    return (pivot + dm).astype(np.float32), np.maximum(s1 / rows - dm * dm, 0).astype(np.float32)


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('group,shape', FWD_CASES, ids=['%s-%s' % (g, 'x'.join(map(str, s))) for g, s in FWD_CASES])
def test_forward_yardstick(group, shape, mode):
    y, b, outside = _fwd(group, shape)
    rounded = group in ('first', 'bf16')           # the kernels that also store bfloat16: then the sums are those of the rounded values
    for stored in ([False, True] if rounded else [False]):
        yk = o.bf16_round(y) if stored else y
        t = R.fwd_terms(yk, b, mode)
        pivot, rows = R.fwd_pivot(b, mode), t.shape[0]
        part = R.f32_partials(t, t * t, block_rows=256 if rows > 256 else 1)
        # (a) honest float32 partials and the moments stage 2 makes of them
        mean, var = _moments_from(part, pivot, rows)
        assert R.partials_ratio(part, t, t * t) < 0.5
        assert R.moments_ratio(mean, var, t, pivot) < 0.5
        # (b) one pixel dropped
        drop = part.copy()
        drop[0, 0] -= t[0].astype(np.float32)
        drop[0, 1] -= (t[0] * t[0]).astype(np.float32)
        assert R.partials_ratio(drop, t, t * t) > 1
        # one out-of-image pixel of a ragged tile added
        to = R.fwd_terms((o.bf16_round(outside) if stored else outside)[None], b, mode)[0]
        add = part.copy()
        add[-1, 0] += to.astype(np.float32)
        add[-1, 1] += (to * to).astype(np.float32)
        assert R.partials_ratio(add, t, t * t) > 1
        # one zero row of a flat tile counted in `rows`: its term is 0 (the accumulator is), the divisor is not
        mean1, var1 = _moments_from(part, pivot, rows + 1)
        assert R.moments_ratio(mean1, var1, t, pivot) > 1
        # the bias added before the moments are taken
        tb = R.fwd_terms(yk.astype(np.float64) + b.astype(np.float64), b, mode)
        assert R.partials_ratio(R.f32_partials(tb, tb * tb), t, t * t) > 1
        # unrounded values where the rounded ones are stored
        if stored:
            tu = R.fwd_terms(y, b, mode)
            assert R.partials_ratio(R.f32_partials(tu, tu * tu), t, t * t) > 1


@pytest.mark.parametrize('group,shape', [(g, s) for g in BWD_GROUPS for s in BWD_GROUPS[g][1]],
                         ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_backward_inputs_leave_the_relu_mask_unambiguous(group, shape):
    bf16 = BWD_GROUPS[group][0]
    dy, wt, bn_x, gamma, beta, mean, var = R.bwd_inputs(shape, bf16)
    assert R.near_zero_mask_count(bn_x, gamma, beta, mean, var) == 0
    if bf16:
        assert np.array_equal(o.bf16_round(bn_x), bn_x) and np.array_equal(o.bf16_round(dy), dy)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('group,shape', BWD_CASES, ids=['%s-%s' % (g, 'x'.join(map(str, s))) for g, s in BWD_CASES])
def test_backward_yardstick(group, shape, relu):
    bf16 = BWD_GROUPS[group][0]
    dy, wt, bn_x, gamma, beta, mean, var = R.bwd_inputs(shape, bf16)
    with o.mixed_precision('bf16' if bf16 else None):
        dx = o.conv2d_bwd(bn_x.astype(np.float64), wt.astype(np.float64), dy.astype(np.float64), 'same')[0].astype(np.float32)
    dxk = o.bf16_round(dx) if bf16 else dx
    t0, t1 = R.bwd_terms(dxk, bn_x, gamma, beta, mean, var, relu)
    part = R.f32_partials(t0, t1, block_rows=256 if t0.shape[0] > 256 else 1)
    assert R.partials_ratio(part, t0, t1) < 0.5
    dbeta, dgamma = (part[:, k].astype(np.float64).sum(0).astype(np.float32) for k in (0, 1))
    assert max(R.sum_ratio(dbeta, t0), R.sum_ratio(dgamma, t1)) < 0.5
    row = int(np.abs(t0).sum(1).argmax())          # a pixel that passes the mask somewhere
    drop = part.copy()
    drop[0, 0] -= t0[row].astype(np.float32)
    drop[0, 1] -= t1[row].astype(np.float32)
    assert R.partials_ratio(drop, t0, t1) > 1
    if relu:        # the mask taken from dx instead of bn_x
        m = dxk.reshape(t0.shape) > 0
        w0 = np.where(m, dxk.reshape(t0.shape).astype(np.float64), 0.0)
        xh = R.bwd_terms(np.ones_like(dxk), bn_x, gamma, beta, mean, var, 0)[1]
        assert R.partials_ratio(R.f32_partials(w0, w0 * xh), t0, t1) > 1
    if bf16:        # the sums of the unrounded gradient
        u0, u1 = R.bwd_terms(dx, bn_x, gamma, beta, mean, var, relu)
        assert R.partials_ratio(R.f32_partials(u0, u1), t0, t1) > 1


@pytest.mark.parametrize('xbf', [False, True], ids=['x_f32', 'x_bf16'])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('case', R.POOL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_window_winner_yardstick(case, mode, xbf):
    n, h, w, c, same = case
    x, gamma, beta = R.pool_inputs(case, mode, xbf)
    xin = np.maximum(x, 0) if mode == 2 else x
    mean = xin.astype(np.float64).reshape(-1, c).mean(0).astype(np.float32)
    var = xin.astype(np.float64).reshape(-1, c).var(0).astype(np.float32)
    p, win = R.pool_reference(x, gamma, beta, mean, var, mode, same)
    p, win = p.astype(np.float32), win.astype(np.float32)
    strangers, rbn = R.xwin_faults(win, p, x, gamma, beta, mean, var, mode, same)
    assert strangers == 0 and rbn < 0.5
    if mode == 1:
        assert R.near_zero_mask_count(win, gamma, beta, mean, var) == 0
    assert np.all(win[..., 1] <= 0) and win[0, 0, 0, 0] == 1.5 and win[0, 1, 0, 2] == 2.5
    # the last element of the window (2 ties of 1.5 around the winner 2.5) recorded instead: still one of the window's inputs, but
    # not the one the pooled output came from
    bad = win.copy()
    bad[0, 1, 0, 2] = 1.5
    strangers, rbn = R.xwin_faults(bad, p, x, gamma, beta, mean, var, mode, same)
    assert strangers == 0 and rbn > 1
    # an element from outside the window
    bad = win.copy()
    bad[0, 0, 0, 3] = np.float32(123.0)
    assert R.xwin_faults(bad, p, x, gamma, beta, mean, var, mode, same)[0] == 1
