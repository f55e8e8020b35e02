"""The BatchNorm kernels of bn_fused.hip in every storage form, operator by operator (bn_storage_ref.py).

bn_stats_fast, bn_apply_fast, bn_relu_pool2_fwd and the eight bn_bwd_reduce_fast / eight bn_bwd_apply_fast instantiations
<POOL, XBF, DYBF> read x and dy as fp32 or bfloat16, and a run-time flag makes store_quad write y / p / dx as rounded bfloat16.
What the default bf16 engine of cnn_L3_melspec2 runs (engine.hip alloc_everything, "which tensors live in HBM as bfloat16", and
the bn_bwd_fast call of tower_backward; d_bf16 / g_bf16 of the BatchNorm's tensors):

    BatchNorm                                     x -> output                     backward: x, dy -> dx
    after the first conv of a tower               bf16 -> y bf16                  bf16, bf16 -> fp32
    mid-block (2a / 3a / 4a)                      bf16 -> y bf16                  bf16, bf16 -> bf16
    pooled tails (mode 1; vision block 1: mode 2) bf16 -> p bf16, xwin bf16       bf16, bf16 -> bf16
    after the embedding conv                      fp32 -> fp32                    fp32, fp32 -> bf16

L3_BF16_CONV_OUT=0 / L3_BF16_DGRAD_OUT=0 reach the other combinations, every one is instantiated, so every one runs here:
x in {fp32, bf16} x dy in {fp32, bf16} x output in {fp32, bf16}, plain (BN + ReLU) and pooled in both ReLU placements.

Tier A, bit-exact: the store flag is a run-time argument of ONE instantiation, so the value in front of the store is the same in
both calls: the bf16-stored tensor must equal bf16_round (nearest even) of the fp32-stored one bit for bit, and mean, var,
dgamma, dbeta and dbias must not change at all -- dbias is the column sum of the UNROUNDED dx.  Every element of every case.

Tier B, against float64: an fp32-stored tensor within TOL = 3e-6 of the reference's range (the layer tests' bound on the layer
tests' distributions); a bf16-stored one by test_conv_layer_bf16_stored_output's criterion (S.stored_ok: bfloat16 values within
half a spacing + TOL of the range) with at most 1e-3 of its elements not THE nearest bfloat16; the window winners exactly the
reference's; dbias by test_bn_relu_pool_tail_layer's bound.  The three big cases on 64 of their channels (S.BIG_CASES).

Out of reach, not tested: the 65 536-block cap of bn_apply_fast / bn_relu_pool2_fwd (tensors of more than 1 GiB) and the 64-bit
branch of pool_index (N H W >= 2^31).
"""
import functools

import numpy as np
import pytest

import bn_storage_ref as S
from l3embedding_amd import _lib
from oracle import l3_oracle as o

pytestmark = pytest.mark.gpu

# Measured on MI355X, worst over every case and form, in units of the reference's range: y 3.1e-7, p 8.6e-7, dx 7.9e-7, mean
# 6.4e-7, var 2.3e-6 (mode 2 at 33 540 rows: the sums are taken about row 0, up to 3 sigma from the mean), dgamma 6.4e-7, dbeta
# 2.6e-7; bf16-stored y / p / dx: at most 1.2e-7 beyond half a spacing, not the nearest bfloat16 at most 6.6e-4 of the elements
# (2 of 3024; every tensor of 10^5 elements and more below 1.7e-4); dbias at most 2.8e-3 of its bound; no wrong winner.
TOL = S.TOL                 # 3e-6
# One row (variance 0): y = beta is what is left of x scale + shift with scale = gamma / sqrt(eps) = 32 gamma, terms ~100 times the
# result, so its rounding error is not small against the RESULT's range: measured 1.74e-5, and the fp32 restatement (S.plain_f32,
# on the CPU) shows the very same 1.74e-5.  The bound there is 4 x the restatement's error against float64 -- for summation order
# and FMA contraction -- = 6.98e-5, and never below TOL.  (dx is identically 0 there: S.check measures it against the largest of
# the terms that cancel, 5.4e-8, and has no "nearest bfloat16" to count.)
DERIVED = {(1, 16): ('y',)}
STORED = ('y', 'p', 'dx')


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _pool_shape(shape):
    return (shape[0], S.pool_out(shape[1], shape[4]), S.pool_out(shape[2], shape[4]), shape[3])


def _tier_a(fails, what, f32, b16, tensors):
    """f32 / b16: one call's outputs by name with the tensor output stored as fp32 / as bfloat16."""
    for k in f32:
        if k in tensors:
            if not _same_bits(b16[k], o.bf16_round(np.ascontiguousarray(f32[k], np.float32))):
                fails.append('%s: stored %s != bf16_round(fp32 %s) in %d elements' % (what, k, k, int((_bits(b16[k]) != _bits(o.bf16_round(f32[k]))).sum())))
        elif not _same_bits(b16[k], f32[k]):
            fails.append('%s: %s changes with the store' % (what, k))


def _tier_b(fails, figures, what, got, ref, stored, tol, ch):
    sub = {k: (v[..., ch] if ch is not None else v) for k, v in got.items()}
    for name, (ok, fig) in S.check(sub, ref, stored, tol).items():
        key = name + (' bf16' if stored else ' fp32') if name.split(':')[-1] in STORED else name
        figures[key] = max(figures.get(key, 0.0), fig)
        if not ok:
            fails.append('%s: %s = %.3e' % (what, name, fig))


@functools.lru_cache(maxsize=None)
def _run(kind, shape, mode, big):
    """Every form of one case on the GPU: (tier A failures, tier B failures, worst figure per criterion)."""
    a_fails, b_fails, figures = [], [], {}
    ch = S.subset_channels(shape[-1 if kind == 'plain' else 3]) if big else None
    forms_b = [(False, False), (True, True)] if big else S.FORMS           # big: the engine's two input forms against float64
    for xbf in (False, True):
        x, g, bt, _ = S.plain_case(shape, mode, xbf, big) if kind == 'plain' else S.pooled_case(shape, mode, xbf, big)
        gs, bs = (g[ch], bt[ch]) if big else (g, bt)
        fwd = {}
        for obf in (False, True):
            if kind == 'plain':
                fwd[obf] = dict(zip(('y', 'mean', 'var'), _lib.op_bn_relu_fwd(x, g, bt, mode, x_bf16=int(xbf), out_bf16=obf)))
            else:
                fwd[obf] = dict(zip(('p', 'mean', 'var'), _lib.op_bn_relu_pool2_fwd(x, g, bt, shape[4], relu_mode=mode, x_bf16=int(xbf), out_bf16=obf)))
        what = '%s %s mode %d x_%s' % (kind, S.tag(shape), mode, 'bf16' if xbf else 'f32')
        _tier_a(a_fails, what + ' fwd', fwd[False], fwd[True], STORED)
        if kind == 'pooled' and shape in S.ODD_SAME:
            # the training forward: the winners in x's storage type beside an unchanged p
            for obf in (False, True):
                p, mean, var, xwin = _lib.op_bn_relu_pool2_fwd(x, g, bt, shape[4], relu_mode=mode, x_bf16=int(xbf), want_xwin=True, out_bf16=obf)
                if not (_same_bits(p, fwd[obf]['p']) and _same_bits(mean, fwd[obf]['mean']) and _same_bits(var, fwd[obf]['var'])):
                    a_fails.append(what + ' out_bf16=%d: p / mean / var change with want_xwin' % obf)
                fwd[obf]['xwin'] = xwin
        for dbf in (False, True):
            dy = S.gradient(shape if kind == 'plain' else _pool_shape(shape), dbf)
            flags = int(xbf) | (2 if dbf else 0)
            bwd = {}
            for obf in (False, True):
                if kind == 'plain':
                    f = fwd[False]
                    bwd[obf] = dict(zip(('dx', 'dgamma', 'dbeta'), _lib.op_bn_relu_bwd(x, f['y'], dy, g, f['mean'], f['var'], mode, beta=bt, x_bf16=flags, out_bf16=obf)))
                else:
                    bwd[obf] = dict(zip(('dx', 'dgamma', 'dbeta', 'dbias'), _lib.op_bn_relu_pool2_bwd(x, g, bt, dy, shape[4], relu_mode=mode, x_bf16=flags, out_bf16=obf)))
            whatb = what + ' dy_%s' % ('bf16' if dbf else 'f32')
            _tier_a(a_fails, whatb + ' bwd', bwd[False], bwd[True], STORED)
            if (xbf, dbf) not in forms_b:
                continue
            xs, dys = (x[..., ch], dy[..., ch]) if big else (x, dy)
            ref = S.plain_ref(xs, gs, bs, dys, mode, xbf, dbf) if kind == 'plain' else S.pooled_ref(xs, gs, bs, dys, shape[4], mode, xbf, dbf)
            tol = {}
            if shape in DERIVED:
                r32 = S.plain_f32(x, g, bt, dy, mode, xbf, dbf)
                for k in DERIVED[shape]:
                    scale = ref['dx_terms'] if k == 'dx' and not np.any(ref['dx']) else None
                    tol[k] = max(TOL, 4 * S.relerr(r32[k], ref[k], scale))
                    figures['derived bound ' + k] = max(figures.get('derived bound ' + k, 0.0), tol[k])
            for obf in (False, True):
                got = dict(bwd[obf])
                if dbf == xbf:          # the forward has no dy: once per form of x
                    got.update(fwd[obf])
                _tier_b(b_fails, figures, whatb + ' out_%s' % ('bf16' if obf else 'f32'), got, ref, STORED if obf else (), tol, ch)
    return a_fails, b_fails, figures


def test_bf16_store_needs_the_fast_kernels(gpu_required):
    """Only the fast kernels store bfloat16: a channel count outside bn_fast_ok is refused, not served by the generic ones."""
    x = np.ones((6, 10), np.float32)
    v = np.ones(10, np.float32)
    with pytest.raises(_lib.L3Error):
        _lib.op_bn_relu_fwd(x, v, v, 1, out_bf16=True)
    with pytest.raises(_lib.L3Error):
        _lib.op_bn_relu_bwd(x, x, x, v, v, v, 1, beta=v, out_bf16=True)


CASES = [('plain', s, m, False) for s, m in S.PLAIN_CASES] + [('pooled', s, m, False) for s, m in S.POOL_CASES] + \
        [(k, s, m, True) for k, s, m in S.BIG_CASES]
IDS = ['%s-%s-mode%d' % (k, S.tag(s), m) for k, s, m, _ in CASES]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_bf16_store_is_the_rounded_fp32_store_bit_for_bit(gpu_required, case):
    """Tier A.  Any mismatch is a fault of the store (or of a path that differs between the two calls): no tolerance."""
    a_fails = _run(*case)[0]
    assert not a_fails, '\n'.join(a_fails)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_every_storage_form_against_float64(gpu_required, case):
    """Tier B.  Prints the worst figure per criterion and storage form: relerr and stored_ok excess in units of the range,
    nearest_share the share of elements that are not the nearest bfloat16, dbias in units of its bound, xwin the share of wrong
    winners."""
    _, b_fails, figures = _run(*case)
    print('BNSTORE %s %s mode %d: %s' % (case[0], S.tag(case[1]), case[2], '  '.join('%s=%.2e' % kv for kv in sorted(figures.items()))))
    assert not b_fails, '\n'.join(b_fails)
