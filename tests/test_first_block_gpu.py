"""The backward of a tower's first block alone against float64 (first_block_ref.py): bn_xhat_ones, the coefficient-only exit of
bn_bwd_fast, all ten conv_first_wgrad_kernel<CA, FUSE, RELU> instantiations, wgrad_reduce and first_conv_grads -- each stage judged
on the tensors the operator itself returned for the stage before, and the whole against the straightforward float64 chain that
computes the first layer's data gradient and the input BatchNorm's backward, which the engine replaces by a closed form.

l3_op_first_block_bwd runs the chain as tower_forward / tower_backward_block do (same calls, same order, one reduction scratch; the
weight-gradient partials in a NaN-preset buffer of exactly conv_wgrad_scratch_floats floats with a guard behind it; every output
NaN before the launches).  The convolution's stored output y is an input, so no rounding decision of a forward kernel enters.

  explicit        conv_first_wgrad_kernel<CA, 0, 0>: bn_bwd_fast writes dY and the bias gradient
  deferred        <CA, 1, RELU>: bn_bwd_fast(dx = NULL) leaves cA, cB, cC; the kernel forms dY = cA mask(dA) + (cB y + cC) from fp32 y, dA
  deferred_bf16   <CA, 2, RELU>: the same from bfloat16-stored y, dA

RELU = 0 runs in no model (every first convolution is followed by BatchNorm and ReLU) but is compiled and dispatchable.

Every call is made twice and must be bit-identical in every output (both kernels sum in a fixed order).  Each criterion is printed
as `FIRSTBLK <instantiation> <shape> <criterion> <error / bound>`; profiles/r29_first_block_bounds.txt keeps the worst of each.
"""
import functools

import numpy as np
import pytest

import first_block_ref as R
from l3embedding_amd import _lib

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _run(shape, c, form, relu):
    """One case in one form on the GPU, twice: (failures, ratios)."""
    cs = R.case(shape, c, form == 'deferred_bf16')
    out = _lib.op_first_block_bwd(*R.op_args(cs), relu=relu, form=form)
    again = _lib.op_first_block_bwd(*R.op_args(cs), relu=relu, form=form)
    fails = ['%s differs between two runs' % k for k in out if not np.array_equal(_bits(out[k]), _bits(again[k]))]
    fails += ['%s is not finite' % k for k in out if not np.isfinite(out[k]).all()]
    del again
    res = R.all_ratios(cs, relu, form, out)
    for line in R.lines(cs, relu, form, res):
        print(line)
    fails += ['%s = %.3g' % (k, v) for k, v in sorted(res.items()) if not v <= 1.0]
    return fails, res


_SMALL = [(s, c, f, r) for s, c in R.SMALL_CASES for f, r in R.SMALL_FORMS]
_CAPPED = [(s, c, f, r) for s, c in R.CAPPED_CASES for f, r in R.CAPPED_FORMS]


def _id(p):
    return '%s-%s-relu%d' % (R.tag(p[0], p[1]), p[2], p[3])


@pytest.mark.parametrize('shape,c,form,relu', _SMALL, ids=[_id(p) for p in _SMALL])
def test_first_block_backward(gpu_required, shape, c, form, relu):
    """Partly filled last units, W < 4, wave ranges that start mid-row and cross the image boundary, dead slots at the end of a range,
    empty waves, up to 26 workgroup partials: every instantiation at every shape (first_block_ref.SMALL_SHAPES)."""
    fails, res = _run(shape, c, form, relu)
    assert not fails, fails
    n, h, wd = shape
    assert ('e2e:dw' in res) == (n * h * wd >= R.E2E_MIN_PIXELS) and ('bite:dgamma_in' in res) == (shape in R.BITE_SHAPES)


@pytest.mark.parametrize('shape,c,form,relu', _CAPPED, ids=[_id(p) for p in _CAPPED])
def test_first_block_backward_beyond_the_wave_cap(gpu_required, shape, c, form, relu):
    """More than 65 536 units: 4096 waves of 19 units each (every real batch runs with per_wave > 16), short and empty waves at the
    end, 1024 workgroup partials; the audio and the vision frame."""
    assert R.launch_shape(shape)[2:] == (4096, 19)
    fails, _ = _run(shape, c, form, relu)
    assert not fails, fails


@pytest.mark.parametrize('taps,c,co', R.GRADS_SHAPES)
def test_first_conv_grads_alone(gpu_required, taps, c, co):
    """first_conv_grads on its own at the first layers' shapes, at 25 taps of 10 filters and at one tap of 300 (more columns than
    threads), with and without the bias gradient."""
    gaug, w, gamma, beta = R.grads_inputs(taps, c, co)
    got = _lib.op_first_conv_grads(gaug, w, gamma, beta)
    again = _lib.op_first_conv_grads(gaug, w, gamma, beta)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    res = R.grads_ratios(gaug, w, gamma, beta, *got)
    for k, v in sorted(res.items()):
        print('FIRSTBLK first_conv_grads %dx%dx%d %s %.4g' % (taps, c, co, k, v))
    assert all(v <= 1.0 for v in res.values()), res
    nb = _lib.op_first_conv_grads(gaug, w, gamma, beta, want_dbias=False)
    assert nb[3] is None and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[:3], nb[:3]))


def test_operator_refuses_what_the_first_layer_kernel_would_not_run(gpu_required, monkeypatch):
    """Two input channels (CA = 3), 32 filters, or the kernel switched off: the generic weight gradient must not stand in."""
    cs = R.case((1, 3, 2), 1)
    x, gi, bi, w, y, g2, b2, dA = R.op_args(cs)
    with pytest.raises(_lib.L3Error):
        _lib.op_first_block_bwd(np.repeat(x, 2, -1), np.repeat(gi, 2), np.repeat(bi, 2), np.repeat(w, 2, 2), y, g2, b2, dA, 1, 'deferred')
    with pytest.raises(_lib.L3Error):
        _lib.op_first_block_bwd(x, gi, bi, w[..., :32], y[..., :32], g2[:32], b2[:32], dA[..., :32], 1, 'deferred')
    monkeypatch.setenv('L3_FIRST_WGRAD', '0')
    with pytest.raises(_lib.L3Error):
        _lib.op_first_block_bwd(x, gi, bi, w, y, g2, b2, dA, 1, 'deferred')
