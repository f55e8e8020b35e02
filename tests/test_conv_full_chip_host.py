"""The full-chip convolution screen's own yardstick on the CPU (conv_replica_ref.py): the scaled-replica batch against the oracle
called directly on a whole small batch, the locator on a planted single-element error, the restated split-K plans at the points
the GPU cases rely on, and the float division the flat tiles of conv_bf16_halo.hip index with."""
import numpy as np
import pytest

import conv_replica_ref as R
from oracle import l3_oracle as o


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def _small_batch():
    n, h, w, ci, co = 7, 6, 5, 8, 8
    rng = np.random.RandomState(5)
    xb, dyb = rng.randn(3, h, w, ci), rng.randn(3, h, w, co)
    wt = rng.randn(3, 3, ci, co)
    x, dy = R.make_batch(xb, dyb, n)
    return n, xb, dyb, wt, x, dy


def test_batch_construction():
    n, xb, dyb, wt, x, dy = _small_batch()
    k = R.scale_exponents(21)
    assert sorted(k[:7]) == list(range(-3, 4))
    assert len({(r % 3, int(k[r])) for r in range(21)}) == 21                 # 21 distinct (base, scale) pairs
    assert all(k[r] != k[r + 1] for r in range(20))
    assert R.replica_counts(7) == [3, 2, 2] and R.replica_counts(27) == [9, 9, 9]
    for r in range(n):
        assert np.array_equal(x[r], xb[r % 3] * 2.0 ** k[r]) and np.array_equal(dy[r], dyb[r % 3] * 2.0 ** -k[r])
        assert not np.array_equal(x[r], x[(r + 1) % n])
    x32 = R.replicate(xb.astype(np.float32), n, 1)                              # exact in float32 too
    assert x32.dtype == np.float32 and np.array_equal(x32[4], xb[1].astype(np.float32) * np.float32(2.0 ** k[4]))


def test_replica_reference_against_the_oracle_on_the_whole_batch():
    """N = 7, 6x5, 8 -> 8 channels, float64: y, dx, dw, db of the oracle on all seven samples against what the harness derives from
    the three bases.  (The oracle's matrix products may sum a row's terms in an order that depends on the row's place in the
    matrix, so its replicas are held to 1e-13, not to bit equality; the kernels' fixed per-pixel order is what the GPU test pins.)"""
    n, xb, dyb, wt, x, dy = _small_batch()
    zero = np.zeros(wt.shape[3])
    y = o.conv2d_fwd(x, wt, zero, 'same')
    dx, dw, db = o.conv2d_bwd(x, wt, dy, 'same')
    y3 = o.conv2d_fwd(x[:3], wt, zero, 'same')
    dx3 = o.conv2d_bwd(x[:3], wt, dy[:3], 'same')[0]
    for r in range(n):
        assert relerr(R.unscaled(y, r, 1), y3[r % 3]) < 1e-13
        assert relerr(R.unscaled(dx, r, -1), dx3[r % 3]) < 1e-13
    k = R.scale_exponents(n)
    assert relerr(y[5], y[2] * 2.0 ** (k[5] - k[2])) < 1e-13 and relerr(dx[5], dx[2] * 2.0 ** (k[2] - k[5])) < 1e-13
    dw_single = [o.conv2d_bwd(xb[j:j + 1], wt, dyb[j:j + 1], 'same', need_dx=False)[1] for j in range(3)]
    assert relerr(R.wgrad_reference(dw_single, n), dw) < 1e-13
    assert relerr(R.bias_grad_reference(dy), db) < 1e-13
    # ... and under the oracle's bfloat16 operand rounding, which the scales must commute with
    with o.mixed_precision('bf16'):
        xb64, dyb64, w64 = (np.repeat(t, 8, axis=-1) for t in (xb, dyb, np.repeat(wt, 8, axis=2)))       # 64 -> 64 channels
        xm, dym = R.make_batch(xb64, dyb64, n)
        ym = o.conv2d_fwd(xm, w64, np.zeros(64), 'same')
        _, dwm, _ = o.conv2d_bwd(xm, w64, dym, 'same', need_dx=False)
        ym3 = o.conv2d_fwd(xm[:3], w64, np.zeros(64), 'same')
        dwm_single = [o.conv2d_bwd(xb64[j:j + 1], w64, dyb64[j:j + 1], 'same', need_dx=False)[1] for j in range(3)]
    assert relerr(ym3, o.conv2d_fwd(xm[:3], w64, np.zeros(64), 'same')) > 1e-4                          # the rounding is on
    for r in range(n):
        assert relerr(R.unscaled(ym, r, 1), ym3[r % 3]) < 1e-13
    assert relerr(R.wgrad_reference(dwm_single, n), dwm) < 1e-13


def test_planted_single_element_error_is_located():
    n, h, w, c = 7, 6, 5, 8
    rng = np.random.RandomState(9)
    y = R.replicate(rng.randn(3, h, w, c).astype(np.float32), n, 1)
    t = R.Tiling(1, 1, 16, 4)                   # flat tiles of 16 pixels, two 4-channel slices
    assert R.replica_difference('y', y, 1, t) is None
    assert R.replica_difference('dx', R.replicate(y[:3] * 1, n, -1), -1, t) is None
    bad = y.copy()
    bad[5, 3, 2, 6] = np.nextafter(bad[5, 3, 2, 6], np.float32(np.inf))          # one ulp, one element
    msg = R.replica_difference('y', bad, 1, t)
    print(msg)
    # pixel (5 * 6 + 3) * 5 + 2 = 167 -> flat tile 10, workgroup 10 * 2 + 6 // 4 = 21
    assert msg.startswith('y: 1 of %d elements differ; first at sample 5 row 3 column 2 channel 6:' % y.size)
    assert 'block 10 ' in msg and 'workgroup 21 ' in msg
    # 2-D patches: 4x2-pixel patches -> 2 x 3 per image; sample 5, patch row 0, patch column 1 -> patch 31, one 8-channel slice
    msg = R.replica_difference('y', bad, 1, R.Tiling(4, 2, 1, 8))
    assert 'block 31 ' in msg and 'workgroup 31 ' in msg
    # a NaN is a difference, and the earliest sample is the one reported
    bad[3, 0, 0, 0] = np.nan
    msg = R.replica_difference('y', bad, 1, t)
    assert msg.startswith('y: 2 of %d elements differ; first at sample 3 row 0 column 0 channel 0:' % y.size)
    # an error in one of the first three samples shows in every replica of it, at the same pixel (the oracle check of the first
    # three samples is what tells which side is wrong)
    bad = y.copy()
    bad[0, 2, 4, 0] *= np.float32(1.5)
    msg = R.replica_difference('y', bad, 1, t)
    assert msg.startswith('y: 2 of %d elements differ; first at sample 3 row 2 column 4 channel 0:' % y.size)
    # the run-to-run comparison uses the same report
    msg = R.describe_difference('dx run 2', bad, y, t)
    assert msg.startswith('dx run 2: 1 of %d elements differ; first at sample 0 row 2 column 4 channel 0:' % y.size)
    assert R.describe_difference('dx run 2', y, y.copy(), t) is None
    assert R.tiling_blocks(t, n, h, w) == 14 and R.tiling_blocks(R.Tiling(4, 2, 1, 8), n, h, w) == 42
    assert R.tiling_blocks(R.Tiling(4, 4, 32, 64), 16, 56, 56) == 98


def test_restated_weight_gradient_plans():
    """The plans at the GPU cases' geometries: the grids the sources cap (512 / 256 blocks) and the stage counts the cases rely on."""
    p = R.wgrad9_plan(27, 112, 112, 64, 128)
    assert (p['patch'], p['tiles'], p['splits'], p['stages_per_split']) == ('4x16', 2, 256, 21) and R.plan_is_full(p)
    p = R.wgrad9_plan(54, 64, 49, 128, 256)
    assert (p['patch'], p['tiles'], p['splits'], p['stages_per_split']) == ('8x8', 8, 64, 48) and R.plan_is_full(p)
    p = R.wgrad9_plan(105, 28, 28, 256, 512)
    assert (p['patch'], p['tiles'], p['splits'], p['stages_per_split']) == ('4x16', 32, 16, 92) and R.plan_is_full(p)
    assert not R.plan_is_full(R.wgrad9_plan(2, 56, 56, 256, 256))               # N = 2: 25 splits of 16 where 32 are asked for
    p = R.wgw_plan(16, 56, 56, 256, 256)
    assert (p['patch'], p['splits'], p['stages_per_split']) == ('2x4 tiles', 16, 98) and R.plan_is_full(p)
    assert not R.plan_is_full(R.wgw_plan(32, 28, 28, 512, 128))                 # 56 stages per split: below 3 x 32
    assert not R.plan_is_full(R.wgw_plan(8, 112, 112, 64, 64))                  # 98 splits where 256 are asked for


# (H, W) of the 16 ledger convolutions (test_layer_parity_gpu.py LEDGER_CONVS) and of every geometry of
# test_conv_bf16_stored_random_geometries (test_parity_gpu.py), the flat-tile ones included
LEDGER_HW = [(256, 199), (128, 99), (64, 49), (32, 24), (224, 224), (112, 112), (56, 56), (28, 28)]
RANDOM_HW = [(8, 32), (9, 33), (17, 15), (5, 50), (31, 7), (40, 70), (1, 1), (16, 16), (20, 45), (33, 17), (3, 4), (28, 28),
             (56, 56), (32, 24), (64, 49), (6, 5), (13, 56)]
# + the full-chip cases of test_conv_full_chip_gpu.py
FDIV_DIVISORS = sorted({d for h, w in LEDGER_HW + RANDOM_HW + [(112, 112), (32, 32), (64, 49), (28, 28)] for d in (w, h, w + 2, h + 1)})


def test_flat_tile_float_division_is_exact_below_the_guard():
    """fdiv(a, 1/b) = int((float(a) + 0.5f) * (1.0f / b)) for EVERY dividend below 2^22 -- where flat_halo_pixels() stops offering
    flat tiles -- and every divisor the kernel forms (W, H, W + 2, H + 1) at the geometries the suite runs."""
    a = np.arange(R.FDIV_GUARD, dtype=np.int32)
    for b in FDIV_DIVISORS:
        bad = R.fdiv(a, b) != a // b
        assert not bad.any(), 'fdiv(%d, 1/%d) = %d' % (int(np.argmax(bad)), b, int(R.fdiv(int(np.argmax(bad)), b)))


def test_flat_tile_float_division_first_failure_above_the_guard():
    """What raising the guard would cost: the smallest dividend in [2^22, 2^24) at which the formula is off, over the same divisors.
    Recorded here: 5 093 084 for b = 15 (1.21 x the guard); the powers of two never fail below 2^23, where a + 0.5 stops being a float."""
    first = {}
    for b in FDIV_DIVISORS:
        f = R.fdiv_first_failure(b, R.FDIV_GUARD, 1 << 24)
        if f is not None:
            first[b] = f
    b_min = min(first, key=first.get)
    print('fdiv: first failure above 2^22 at a = %d for b = %d; %d of %d divisors fail below 2^24' % (
        first[b_min], b_min, len(first), len(FDIV_DIVISORS)))
    assert (first[b_min], b_min) == (5093084, 15)
    assert all(f >= 1 << 23 for b, f in first.items() if b & (b - 1) == 0)
