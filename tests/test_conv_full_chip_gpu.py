"""Every product convolution kernel with the whole chip busy, checked over its WHOLE output (conv_replica_ref.py).

The convolution kernels keep LDS-DMA loads in flight across raw s_barriers behind counted s_waitcnt vmcnt(n) and run two to four
workgroups per CU, each covering a neighbour's prologue and epilogue.  A wrong wait count, or an LDS region a neighbour still
reads, passes a small launch whenever the load happens to land first -- and the exact tests of these kernels run at N = 2, where
no CU ever holds its full complement of blocks.  Here every case sizes its batch at run time so that the forward launch is at
least 2.5 rounds of (CUs x blocks per CU) workgroups -- two full rounds of replacement and a ragged third -- and checks

  * y and dx of EVERY sample, bit for bit, against the first three samples' (the batch is scaled copies of three base samples;
    a power-of-two scale commutes with every rounding of these kernels) -- which, as flat tiles and tile blocks start at a
    different offset in every sample, also pins that a pixel's sum does not depend on where its tile begins;
  * y and dx of the first three samples against the float64 oracle (under mixed_precision('bf16') for the bf16 forms), within
    the bounds of test_layer_parity_gpu.py, and every other sample against the same float64 result scaled;
  * dw against sum_j count_j dw_j of the oracle's single-sample weight gradients, db against the float64 column sum of dy;
  * three launches, every output bit-identical to the first.

A failure names the output, the count of differing elements, and sample, row, column, channel, block and workgroup of the first.
Each case prints its N, workgroups, rounds, the restated split-K plan of its weight-gradient kernel and every measured error.

Measured on an MI355X (256 CUs), worst over the cases: bf16 forms y 6.4e-7, dx 9.9e-7 of the range (stored-bfloat16 outputs: 2.1e-7
beyond half a spacing), F(4x4,3x3) y 5.8e-6, dx 5.0e-6; dw 7.8e-7 (bf16, 28x28 256->512 at N = 105) and 9.4e-7 (fp32, 56x56 at
N = 16), db 1.0e-7.  The weight gradients sum 8 to 320 times the terms of the N = 2 ledger and still sit below a third of TOL (the
split-K grids are capped, the partial slices are summed in order and the replicas' contributions are equal), so TOL stands as it is
and no bound was derived from a restated summation order.  Every case runs in about a second."""
import collections
import functools
import time

import numpy as np
import pytest

import conv_replica_ref as R
from l3embedding_amd import _lib
from oracle import l3_oracle as o
from test_layer_parity_gpu import TOL, TOL_F4, relerr

pytestmark = pytest.mark.gpu

Case = collections.namedtuple('Case', 'tag h w ci co dtypes fwd dgrad bpc rounds n0')

# The smallest product geometries that select each form.  fwd / dgrad: the tiling of the kernel that writes y / dx (what a failure
# report places its block and workgroup by); bpc: resident workgroups per CU of the forward kernel, with its source; rounds: the
# forward launch holds at least this many times CUs x bpc workgroups (2.5 everywhere: every case runs in a few seconds); n0: the
# fp32 cases take the batch of test_winograd_f4_race_screen instead (their forward is a persistent grid of one workgroup per CU).
CASES = [
    # halo kernel, 2-D 16x16 patches, 128-channel blocks, one halo buffer and a 2-deep filter ring (MODE 1): two blocks per CU,
    # HaloGeom::BLOCKS_PER_CU = MODE == 1 ? 2 (80 KiB of LDS each; __launch_bounds__(512, 4)).  The data gradient (128 -> 64) lands
    # on the 64-channel form; the weight gradient's patch shapes tie at 112 x 112 (4x16 taken).  N = 27 on 256 CUs.
    Case('halo-2d-128ch', 112, 112, 64, 128, ('bf16_stored', 'bf16_stored_out'), R.Tiling(16, 16, 1, 128), R.Tiling(16, 16, 1, 64), 2, 2.5, None),
    # halo kernel, 2-D 8x32 patches, 64-channel blocks on 32-channel chunks (MODE 2): four blocks per CU, HaloGeom::BLOCKS_PER_CU =
    # MODE == 2 ? (WN == 1 ? 4 : 2) (39 KiB each; __launch_bounds__(256, 4)).  N = 642 on 256 CUs.
    Case('halo-2d-64ch', 32, 32, 64, 64, ('bf16_stored',), R.Tiling(8, 32, 1, 64), R.Tiling(8, 32, 1, 64), 4, 2.5, None),
    # flat tiles (MODE 4), odd width: 64 * 49 = 12.25 tiles per image, tiles begin mid-row and span images; two blocks per CU,
    # HaloGeom::BLOCKS_PER_CU = MODE >= 3 ? 2 (the launch sizes the LDS: 66 KiB here).  The data gradient (256 -> 128) is flat too;
    # the weight gradient takes 8x8 patches.  N = 54 on 256 CUs.
    Case('flat-odd-width', 64, 49, 128, 256, ('bf16_stored', 'bf16_stored_out'), R.Tiling(1, 1, 256, 128), R.Tiling(1, 1, 256, 128), 2, 2.5, None),
    # flat tiles (MODE 4), 8 chunks of 32 input channels, 3.0625 tiles per image; weight gradient on 4x16 patches.  N = 105 on 256 CUs.
    Case('flat-8-chunks', 28, 28, 256, 512, ('bf16_stored',), R.Tiling(1, 1, 256, 128), R.Tiling(1, 1, 256, 128), 2, 2.5, None),
    # fp32: F(4x4,3x3) forward and data gradient (conv_wino4.hip: tile blocks of 32 tiles of 4x4 pixels x 64 channels over a
    # persistent grid), Winograd F(3x3,2x2) weight gradient (conv_wgrad_wino.hip).  L3_W4_TAIL=0 keeps the F(4x4) launch to one
    # pass: the split tail sums channel slices separately, so its blocks are legitimately not bit-equal to the others (it has its
    # own tests).  N starts at test_winograd_f4_race_screen's and is raised until the weight gradient's split-K reaches its block
    # target with every block at least 3 x 32 stages long: 16, 55 and 63.
    Case('f4-56x56', 56, 56, 256, 256, ('f32',), R.Tiling(4, 4, 32, 64), R.Tiling(4, 4, 32, 64), 1, None, 16),
    Case('f4-28x28', 28, 28, 512, 128, ('f32',), R.Tiling(4, 4, 32, 64), R.Tiling(4, 4, 32, 64), 1, None, 32),
    Case('f4-112x112', 112, 112, 64, 64, ('f32',), R.Tiling(4, 4, 32, 64), R.Tiling(4, 4, 32, 64), 1, None, 8),
]
PARAMS = [(c, d) for c in CASES for d in c.dtypes]


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _plan(c, n, dtype):
    return (R.wgw_plan if dtype == 'f32' else R.wgrad9_plan)(n, c.h, c.w, c.ci, c.co)


def _workgroups(c, n, dtype):
    return _lib.op_conv2d_stat_blocks((n, c.h, c.w, c.ci), c.co, dtype) * (c.co // c.fwd.bn)


def _batch_size(c, dtype, cus):
    """bf16 forms: the smallest multiple of 3 whose forward launch holds c.rounds x CUs x bpc workgroups; fp32: c.n0.  Either is
    raised until the weight-gradient kernel's plan reaches its block target with >= 3 x its minimum stages per split."""
    n, step = (3, 3) if c.n0 is None else (c.n0, 1)
    if c.n0 is None:
        while _workgroups(c, n, dtype) < c.rounds * cus * c.bpc:
            n += step
    while not R.plan_is_full(_plan(c, n, dtype)):
        n += step
    return n


@functools.lru_cache(maxsize=None)
def _bases(tag):
    """The three base samples as the layer sees them in the network (test_layer_parity_gpu._layer_data): a post-ReLU activation, a
    he_normal filter, an output gradient of BatchNorm-backward magnitude; the bias is zero."""
    c = next(k for k in CASES if k.tag == tag)
    rng = np.random.RandomState(sum(map(ord, tag)) + c.h + c.ci)
    xb = np.maximum(rng.randn(3, c.h, c.w, c.ci), 0).astype(np.float32)
    wt = (rng.randn(3, 3, c.ci, c.co) * np.sqrt(2.0 / (9 * c.ci))).astype(np.float32)
    dyb = (rng.randn(3, c.h, c.w, c.co) * 1e-3).astype(np.float32)
    for t in (xb, wt, dyb):
        t.setflags(write=False)
    return xb, wt, dyb


@functools.lru_cache(maxsize=None)
def _oracle(tag, mixed):
    """float64 y and dx of the first three samples of the batch (the bases at their own scales 2^k(0..2)) and their single-sample
    weight gradients, in which the scales cancel; computed once per case."""
    xb, wt, dyb = _bases(tag)
    x3, dy3 = R.make_batch(xb, dyb, 3)
    x64, w64, dy64 = (t.astype(np.float64) for t in (x3, wt, dy3))
    with o.mixed_precision('bf16' if mixed else None):
        y3 = o.conv2d_fwd(x64, w64, np.zeros(wt.shape[3]), 'same')
        dx3 = o.conv2d_bwd(x64, w64, dy64, 'same')[0]
        dw_single = [o.conv2d_bwd(x64[j:j + 1], w64, dy64[j:j + 1], 'same', need_dx=False)[1] for j in range(3)]
    for t in [y3, dx3] + dw_single:
        t.setflags(write=False)
    return y3, dx3, dw_single


def _oracle_error(out, ref3, sign, stored, tol):
    """Worst of the samples' error / bound against the float64 result of their base, scaled (all of them: the first three are the
    bases themselves).  stored: test_conv_layer_bf16_stored_output's criterion -- bfloat16 values within half a spacing plus the
    fp32 accumulation error (tol x range) of the float64 result; else max |err| / range against tol.  Returns (ratio, error)."""
    span = [float(np.abs(ref3[j]).max()) for j in range(3)]
    worst_ratio, worst_err = 0.0, 0.0
    for r in range(out.shape[0]):
        j = r % 3
        got = R.unscaled(out, r, sign).astype(np.float64)
        err = np.abs(got - ref3[j])
        if stored:
            if not np.array_equal(o.bf16_round(got), got):
                return float('inf'), float('inf')
            err -= 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref3[j]), np.abs(got)) + 1e-300)) - 8)
        e = float(err.max()) / span[j]
        worst_err, worst_ratio = max(worst_err, e), max(worst_ratio, e / tol)
    return worst_ratio, worst_err


@pytest.mark.parametrize('case,dtype', PARAMS, ids=['%s-%s' % (c.tag, d) for c, d in PARAMS])
def test_conv_full_chip(gpu_required, case, dtype, monkeypatch):
    c, t0 = case, time.time()
    f32 = dtype == 'f32'
    if f32:
        monkeypatch.setenv('L3_W4_TAIL', '0')
    cus = _cus()
    n = _batch_size(c, dtype, cus)
    blocks = _lib.op_conv2d_stat_blocks((n, c.h, c.w, c.ci), c.co, dtype)
    wgs, plan = _workgroups(c, n, dtype), _plan(c, n, dtype)
    rounds = wgs / float(cus * c.bpc)
    head = 'FULLCHIP %s %s %dx%d %d->%d' % (c.tag, dtype, c.h, c.w, c.ci, c.co)
    print('%s: N=%d CUs=%d blocks/CU=%d forward workgroups=%d (%d blocks x %d channel slices) rounds=%.2f dgrad workgroups=%d'
          % (head, n, cus, c.bpc, wgs, blocks, c.co // c.fwd.bn, rounds, R.tiling_blocks(c.dgrad, n, c.h, c.w) * (c.ci // c.dgrad.bn)))
    print('%s: weight gradient %s, %s patches: %d tiles x %d splits = %d blocks (target %d), %d stages per split (minimum %d)'
          % (head, plan['kernel'], plan['patch'], plan['tiles'], plan['splits'], plan['blocks'], plan['target'],
             plan['stages_per_split'], plan['min_stages']))
    # the library's own block count is that of the form the case is about (flat tiles / this patch shape / F(4x4) tile blocks)
    assert blocks == R.tiling_blocks(c.fwd, n, c.h, c.w), (blocks, c.fwd)
    assert R.plan_is_full(plan), plan
    if not f32:
        assert n % 3 == 0 and rounds >= c.rounds, (n, wgs, rounds)

    xb, wt, dyb = _bases(c.tag)
    x, dy = R.make_batch(xb, dyb, n)
    zero = np.zeros(c.co, np.float32)
    y = _lib.op_conv2d_fwd(x, wt, zero, True, dtype=dtype)
    dx, dw, db = _lib.op_conv2d_bwd(x, wt, dy, True, dtype=dtype)

    # ---- every sample against the first three, bit for bit ----
    problems = [R.replica_difference('y', y, 1, c.fwd), R.replica_difference('dx', dx, -1, c.dgrad)]
    # ---- the oracle: the first three samples, and every other one against the same float64 result scaled ----
    y3, dx3, dw_single = _oracle(c.tag, not f32)
    stored = dtype == 'bf16_stored_out'
    tol = TOL_F4 if f32 else TOL
    ry, ey = _oracle_error(y, y3, 1, stored, tol)
    rdx, edx = _oracle_error(dx, dx3, -1, stored, tol)
    ry3, _ = _oracle_error(y[:3], y3, 1, stored, tol)
    rdx3, _ = _oracle_error(dx[:3], dx3, -1, stored, tol)
    edw = relerr(dw, R.wgrad_reference(dw_single, n))
    edb = relerr(db, R.bias_grad_reference(dy))
    what = 'excess over half a bfloat16 spacing' if stored else 'error'
    print('%s: y %s %.2e, dx %s %.2e of the range (bound %.1e; first three samples: %.2f and %.2f of it), dw=%.2e db=%.2e (bound %.1e)'
          % (head, what, ey, what, edx, tol, ry3, rdx3, edw, edb, TOL))
    if ry >= 1:
        problems.append('y: %.2f of the oracle bound' % ry)
    if rdx >= 1:
        problems.append('dx: %.2f of the oracle bound' % rdx)
    if not edw < TOL:
        problems.append('dw: %.2e against %.1e' % (edw, TOL))
    if not edb < TOL:
        problems.append('db: %.2e against %.1e' % (edb, TOL))
    if not f32:           # it IS the rounded computation: far from the unrounded fp32 convolution
        assert relerr(y[:1], o.conv2d_fwd(x[:1].astype(np.float64), wt.astype(np.float64), np.zeros(c.co), 'same')) > 1e-4

    # ---- three launches, bit-identical ----
    for run in (2, 3):
        y2 = _lib.op_conv2d_fwd(x, wt, zero, True, dtype=dtype)
        problems.append(R.describe_difference('y of launch %d against launch 1' % run, y2, y, c.fwd))
        del y2
        dx2, dw2, db2 = _lib.op_conv2d_bwd(x, wt, dy, True, dtype=dtype)
        problems.append(R.describe_difference('dx of launch %d against launch 1' % run, dx2, dx, c.dgrad))
        for name, a, b in (('dw', dw2, dw), ('db', db2, db)):
            if not np.array_equal(a, b):
                problems.append('%s of launch %d against launch 1: %d of %d elements differ, first at flat index %d'
                                % (name, run, int((a != b).sum()), a.size, int(np.argmax((a != b).ravel()))))
        del dx2
    problems = [p for p in problems if p]
    print('%s: %s in %.1f s' % (head, 'ok' if not problems else 'FAILED', time.time() - t0))
    assert not problems, '\n'.join([head] + problems)
