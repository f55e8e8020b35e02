"""What the convolution epilogues leave for the BatchNorm beside them, each kernel alone against float64 (epilogue_stats_ref.py).

Forward: the per-block [sum, sum of squares] of y (relu(y)) about the bias, from the main epilogue and the channel-sliced tail of
the F(4x4,3x3) kernel, from F(2x2,3x3) and its split-bf16 experiment, from the first-layer kernel and from the bf16 halo (2-D
patches, flat tiles) and tap-by-tap kernels.  Backward: the data gradient's [sum m dx, sum m dx x_hat] for the BatchNorm in front
(BnBwdFuse), also over the window winners a pooled BatchNorm's forward leaves.  The operators run the engine's own path resolution
and block counts on a partial buffer of exactly that many NaN blocks with a guard behind it, and the reference is float64 NumPy of
the tensor the GPU itself returned, so only the epilogue's summation is judged: every sum within 3e-6 of the sum of its terms'
magnitudes.  Each case prints err / bound (profiles/r27_epilogue_stats_bounds.txt records the worst per kernel)."""
import functools

import numpy as np
import pytest

import epilogue_stats_ref as R
from conftest import need_experiments
from l3embedding_amd import _lib
from oracle import l3_oracle as o

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@functools.lru_cache(maxsize=None)
def _oracle_fwd(group, shape, mixed):
    x, wt, b = R.conv_inputs(group, shape)
    x64, w64, b64 = (t.astype(np.float64) for t in (x, wt, b))
    with o.mixed_precision('bf16' if mixed else None):
        y = o.conv2d_fwd(x64, w64, b64, 'same')
    y.setflags(write=False)
    return y


def _stored_bf16_ok(y, exact):
    """test_conv_layer_bf16_stored_output's criterion: bfloat16 values within half a spacing + the fp32 accumulation error."""
    y = y.astype(np.float64)
    assert np.array_equal(o.bf16_round(y), y)
    half_ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(exact), np.abs(y)) + 1e-300)) - 8)
    return float((np.abs(y - exact) - half_ulp).max()) <= R.TOL * np.abs(exact).max()


def _forward(kernel, group, shape, mode, dtype='f32', y_tol=R.TOL):
    """One forward case: twice (bit-identical partials), y against the oracle, partials and moments against the float64 sums over the
    returned y.  Returns (y, partials, terms)."""
    x, wt, b = R.conv_inputs(group, shape)
    y, part, mean, var = _lib.op_conv2d_fwd_stats(x, wt, b, True, mode, dtype=dtype)
    y2, part2, mean2, var2 = _lib.op_conv2d_fwd_stats(x, wt, b, True, mode, dtype=dtype)
    assert np.array_equal(part, part2) and np.array_equal(y, y2) and np.array_equal(mean, mean2) and np.array_equal(var, var2)
    exact = _oracle_fwd(group, shape, dtype != 'f32')
    if dtype == 'bf16_stored_out':
        assert _stored_bf16_ok(y, exact), (kernel, shape)
    else:
        assert relerr(y, exact) < y_tol, (kernel, shape, relerr(y, exact))
    t = R.fwd_terms(y, b, mode)
    rp = R.partials_ratio(part, t, t * t)
    rm = R.moments_ratio(mean, var, t, R.fwd_pivot(b, mode))
    print('EPISTAT %s fwd %s mode=%d %s nblk=%d partials=%.3f moments=%.3f' % (kernel, 'x'.join(map(str, shape)), mode, dtype, part.shape[0], rp, rm))
    assert rp <= 1 and rm <= 1, (kernel, shape, mode, dtype, rp, rm)
    return y, part, t


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('shape', R.F4_SHAPES)
def test_f4_main_epilogue_moments(gpu_required, shape, mode, monkeypatch):
    """conv_wino4.hip, one-pass epilogue: ragged tile rows / columns, a partial last tile block, 2 to 9 eight-channel stages."""
    monkeypatch.setenv('L3_WINO4', '16')
    monkeypatch.setenv('L3_W4_TAIL', '0')
    _forward('wino4', 'wino', shape, mode, y_tol=R.TOL_F4)


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('case', R.F4_TAIL_CASES, ids=lambda c: 'x'.join(map(str, c[0])))
def test_f4_tail_reduce_moments(gpu_required, case, mode, monkeypatch):
    """wino4_tail_reduce_kernel: the tail tile blocks' channel slices summed, bias added, moments taken -- and the same layer with the
    tail off.  Each one's partials must also fit the OTHER's y (the two differ in summation order only), and the two y must differ in
    some bit: the tail really ran."""
    shape, ncu = case
    if ncu is not None:
        monkeypatch.setenv('L3_W4_NCU', ncu)
    y_t, part_t, t_t = _forward('wino4_tail', 'wino', shape, mode, y_tol=R.TOL_F4)
    monkeypatch.setenv('L3_W4_TAIL', '0')
    y_0, part_0, t_0 = _forward('wino4', 'wino', shape, mode, y_tol=R.TOL_F4)
    assert part_t.shape == part_0.shape
    assert not np.array_equal(y_t, y_0)
    # the sums over the other run's y: the y differ by the kernel's own error (<= TOL_F4 of the range), far above the criterion, in
    # single elements -- but with alternating signs; the sums are held to the criterion all the same
    cross = max(R.partials_ratio(part_t, t_0, t_0 * t_0), R.partials_ratio(part_0, t_t, t_t * t_t))
    print('EPISTAT wino4_tail cross %s mode=%d ratio=%.3f' % ('x'.join(map(str, shape)), mode, cross))
    assert cross <= 1, (shape, mode, cross)


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('shape', R.F2_SHAPES)
def test_f2_epilogue_moments(gpu_required, shape, mode, monkeypatch):
    """conv_wino.hip F(2x2,3x3)."""
    monkeypatch.setenv('L3_WINO4', '0')
    _forward('wino2', 'wino', shape, mode)


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('shape', R.BX6_SHAPES)
def test_bx6_epilogue_moments(gpu_required, shape, mode, monkeypatch):
    """conv_wino_bx6.hip (the experiments build): blocks of flat tile rows that straddle one or two image boundaries."""
    need_experiments()
    monkeypatch.setenv('L3_FP32_CONV', 'f2x2_bf16x6')
    _forward('wino_bx6', 'wino', shape, mode)


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('dtype', ['f32', 'bf16_stored_out'])
@pytest.mark.parametrize('shape', R.FIRST_SHAPES)
def test_first_layer_epilogue_moments(gpu_required, shape, dtype, mode):
    """conv_first.hip, fp32 and bfloat16 output (the moments of the ROUNDED values); mode 2 is the vision tower's order.  The widest
    cases have one block whose waves each sum 288 (1x5x199) or 480 (1x40x65) pixels per channel: the bf16-output form summed them
    in one fp32 chain and came to 1.12 and 1.25 of the bound in mode 2; it now sums per 32-pixel run (0.15).  The fp32-output form
    keeps the chain, at 0.72 / 0.85 (profiles/r27_epilogue_stats_bounds.txt, FINDING 1)."""
    _forward('first', 'wino', shape, mode, dtype=dtype)


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('dtype', ['bf16_stored', 'bf16_stored_out'])
@pytest.mark.parametrize('variant', R.BF16_VARIANTS)
def test_bf16_stored_epilogue_moments(gpu_required, variant, dtype, mode, monkeypatch):
    """conv_bf16_halo.hip (2-D patches 8 x 32 / 16 x 16, flat tiles that start mid-row, span images and hold zero rows) and
    conv_bf16.hip (tap by tap), ragged against every tile shape.  bf16 output: the partials are those of the rounded values -- they
    fit the returned tensor and are FAR from the sums over the unrounded convolution."""
    for k, v in R.bf16_variant_env(variant).items():
        monkeypatch.setenv(k, v)
    far = 0.0
    for shape in R.bf16_shapes(variant):
        y, part, t = _forward('bf16_' + variant, 'bf16', shape, mode, dtype=dtype)
        if dtype == 'bf16_stored_out':
            b = R.conv_inputs('bf16', shape)[2]
            tu = R.fwd_terms(_oracle_fwd('bf16', shape, True), b, mode)
            far = max(far, R.partials_ratio(part, tu, tu * tu))
    if dtype == 'bf16_stored_out':
        print('EPISTAT bf16_%s distance to the unrounded sums / bound = %.1f' % (variant, far))
        assert far > 10, (variant, far)


def _backward(kernel, dgrad_shape, relu, dtype, dx_tol):
    bf = dtype != 'f32'
    dy, wt, bn_x, gamma, beta, mean, var = R.bwd_inputs(dgrad_shape, bf)
    assert R.near_zero_mask_count(bn_x, gamma, beta, mean, var) == 0
    dx, part, dg, db = _lib.op_conv2d_dgrad_bn_bwd(dy, wt, True, bn_x, gamma, beta, mean, var, relu, dtype=dtype)
    dx2, part2, _, _ = _lib.op_conv2d_dgrad_bn_bwd(dy, wt, True, bn_x, gamma, beta, mean, var, relu, dtype=dtype)
    assert np.array_equal(part, part2) and np.array_equal(dx, dx2)
    with o.mixed_precision('bf16' if bf else None):
        exact = o.conv2d_bwd(bn_x.astype(np.float64), wt.astype(np.float64), dy.astype(np.float64), 'same')[0]
    if bf:
        assert _stored_bf16_ok(dx, exact), (kernel, dgrad_shape)
    else:
        assert relerr(dx, exact) < dx_tol, (kernel, dgrad_shape, relerr(dx, exact))
    t0, t1 = R.bwd_terms(dx, bn_x, gamma, beta, mean, var, relu)
    rp = R.partials_ratio(part, t0, t1)
    rf = max(R.sum_ratio(db, t0), R.sum_ratio(dg, t1))
    print('EPISTAT %s bwd %s relu=%d %s nblk=%d partials=%.3f dgamma_dbeta=%.3f' % (kernel, 'x'.join(map(str, dgrad_shape)), relu, dtype, part.shape[0], rp, rf))
    assert rp <= 1 and rf <= 1, (kernel, dgrad_shape, relu, rp, rf)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('shape', R.F4_SHAPES[:3])
def test_f4_dgrad_bn_backward_partials(gpu_required, shape, relu, monkeypatch):
    monkeypatch.setenv('L3_WINO4', '16')
    monkeypatch.setenv('L3_W4_TAIL', '0')
    _backward('wino4', shape, relu, 'f32', R.TOL_F4)


@pytest.mark.parametrize('relu', [0, 1])
def test_f4_tail_dgrad_bn_backward_partials(gpu_required, relu):
    """The forward layer (2, 12, 12, 64 -> 256): its data gradient has 256 input channels and one tile block, all tail."""
    _backward('wino4_tail', (2, 12, 12, 256, 64), relu, 'f32', R.TOL_F4)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('shape', R.F2_SHAPES[:2])
def test_f2_dgrad_bn_backward_partials(gpu_required, shape, relu, monkeypatch):
    monkeypatch.setenv('L3_WINO4', '0')
    _backward('wino2', shape, relu, 'f32', R.TOL)


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('variant', ['halo_auto', 'halo_pw16', 'halo_flat'])
def test_bf16_halo_dgrad_bn_backward_partials(gpu_required, variant, relu, monkeypatch):
    """conv_bf16_halo.hip on bf16-stored dy, bn_x and dx: the sums are those of the STORED gradient."""
    for k, v in R.bf16_variant_env(variant).items():
        monkeypatch.setenv(k, v)
    for shape in R.bf16_shapes(variant):
        _backward('bf16_' + variant, shape, relu, 'bf16_stored_out', R.TOL)


@pytest.mark.parametrize('xbf', [False, True], ids=['x_f32', 'x_bf16'])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('case', R.POOL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_pooled_chain_window_winners_feed_the_backward_partials(gpu_required, case, mode, xbf):
    """bn_relu_pool2_fwd's winner tensor (never read by a test before): each element is one of its window's inputs and the one whose
    BatchNorm(-ReLU) IS the pooled output; then the data gradient at the pooled geometry takes it as the BatchNorm input (relu 1 for
    BN -> ReLU, 0 for ReLU -> BN: bn_bwd_fuse) -- where an engine fuses the two (64 channels and more)."""
    n, h, w, c, same = case
    x, gamma, beta = R.pool_inputs(case, mode, xbf)
    p, mean, var, xwin = _lib.op_bn_relu_pool2_fwd(x, gamma, beta, same, relu_mode=mode, x_bf16=xbf, want_xwin=True)
    p0, mean0, var0 = _lib.op_bn_relu_pool2_fwd(x, gamma, beta, same, relu_mode=mode, x_bf16=xbf)
    assert np.array_equal(p, p0) and np.array_equal(mean, mean0) and np.array_equal(var, var0)
    strangers, rbn = R.xwin_faults(xwin, p, x, gamma, beta, mean, var, mode, same)
    print('EPISTAT pool2_xwin %s mode=%d %s bn(xwin) vs p=%.3f' % ('x'.join(map(str, case)), mode, 'bf16' if xbf else 'f32', rbn))
    assert strangers == 0 and rbn <= 1, (case, mode, strangers, rbn)
    ref_p, ref_win = R.pool_reference(x, gamma, beta, mean, var, mode, same)
    assert relerr(p, ref_p) < R.TOL
    relu = 1 if mode == 1 else 0
    if relu:
        assert R.near_zero_mask_count(xwin, gamma, beta, mean, var) == 0
    rng = np.random.RandomState(c + h)
    co = 64
    wt = (rng.randn(3, 3, c, co) * np.sqrt(2.0 / (9 * co))).astype(np.float32)
    dy = rng.randn(*(p.shape[:3] + (co,))).astype(np.float32)
    dtype = 'bf16_stored_out' if xbf else 'f32'
    if xbf:
        dy = o.bf16_round(dy)
    if c % 64:
        with pytest.raises(_lib.L3Error):          # no engine leaves a 16-channel BatchNorm's reduction to a data gradient
            _lib.op_conv2d_dgrad_bn_bwd(dy, wt, True, xwin, gamma, beta, mean, var, relu, bn_rows=n * h * w, dtype=dtype)
        return
    dx, part, dg, db = _lib.op_conv2d_dgrad_bn_bwd(dy, wt, True, xwin, gamma, beta, mean, var, relu, bn_rows=n * h * w, dtype=dtype)
    t0, t1 = R.bwd_terms(dx, xwin, gamma, beta, mean, var, relu)
    rp = R.partials_ratio(part, t0, t1)
    rf = max(R.sum_ratio(db, t0), R.sum_ratio(dg, t1))
    print('EPISTAT pooled_dgrad %s mode=%d %s nblk=%d partials=%.3f dgamma_dbeta=%.3f' % ('x'.join(map(str, case)), mode, dtype, part.shape[0], rp, rf))
    assert rp <= 1 and rf <= 1, (case, mode, rp, rf)
