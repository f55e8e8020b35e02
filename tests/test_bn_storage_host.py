"""bn_storage_ref.py on the CPU: the float64 reference is the oracle's unfused composition, every case of test_bn_storage_gpu.py
meets the unambiguity margins, the fp32 restatement of the kernels passes every criterion (control) and each of its mutants
fails the criterion named for it on at least one of the GPU test's cases."""
import numpy as np
import pytest

import bn_storage_ref as S
import epilogue_stats_ref as E
from oracle import l3_oracle as o


def _f64(*a):
    return [np.asarray(t, np.float32).astype(np.float64) for t in a]


@pytest.mark.parametrize('xbf', [False, True], ids=['x_f32', 'x_bf16'])
def test_reference_is_the_unfused_oracle_composition(xbf):
    for shape, mode in S.POOL_CASES:
        x, g, bt, _ = S.pooled_case(shape, mode, xbf)
        dp = S.gradient((shape[0], S.pool_out(shape[1], shape[4]), S.pool_out(shape[2], shape[4]), shape[3]), xbf)
        r = S.pooled_ref(x, g, bt, dp, shape[4], mode, xbf, xbf)
        x64, g64, b64, dp64 = _f64(x, g, bt, dp)
        pad = 'same' if shape[4] else 'valid'
        if mode == 1:                                     # keras: Conv, BatchNormalization, Activation('relu'), MaxPooling2D
            y, cache = o.bn_fwd(x64, g64, b64, None, None, True)
            a = np.maximum(y, 0)
            p, pc = o.maxpool_fwd(a, 2, 2, 2, 2, pad)
            dx, dg, db = o.bn_bwd(np.where(a > 0, o.maxpool_bwd(dp64, pc), 0), g64, cache, True)
        else:                                             # Conv, Activation('relu'), BatchNormalization, MaxPooling2D
            y, cache = o.bn_fwd(np.maximum(x64, 0), g64, b64, None, None, True)
            p, pc = o.maxpool_fwd(y, 2, 2, 2, 2, pad)
            dr, dg, db = o.bn_bwd(o.maxpool_bwd(dp64, pc), g64, cache, True)
            dx = np.where(x64 > 0, dr, 0)
        for k, v in dict(p=p, dx=dx, dgamma=dg, dbeta=db, mean=cache[2], var=cache[3], dbias=dx.reshape(-1, shape[3]).sum(0)).items():
            assert np.array_equal(r[k], v), (shape, mode, k)
        # the winners, from an independent statement of the first-maximum rule (epilogue_stats_ref)
        p2, win2 = E.pool_reference(x, g, bt, r['mean'], r['var'], mode, shape[4])
        assert np.array_equal(win2, r['xwin']) and S.relerr(p2, r['p']) < 1e-6, (shape, mode)
    for shape, relu in S.PLAIN_CASES:
        x, g, bt, _ = S.plain_case(shape, relu, xbf)
        dy = S.gradient(shape, xbf)
        r = S.plain_ref(x, g, bt, dy, relu, xbf, xbf)
        x64, g64, b64, dy64 = _f64(x, g, bt, dy)
        m, v = x64.mean(0), x64.var(0)
        xh = (x64 - m) / np.sqrt(v + o.BN_EPS)
        y = xh * g64 + b64
        dz = np.where(y > 0, dy64, 0) if relu else dy64
        dx = g64 / np.sqrt(v + o.BN_EPS) * (dz - dz.mean(0) - xh * (dz * xh).mean(0))
        assert np.allclose(r['y'], np.maximum(y, 0) if relu else y, rtol=0, atol=1e-12)
        assert np.allclose(r['dx'], dx, rtol=0, atol=1e-15) and np.allclose(r['dgamma'], (dz * xh).sum(0), rtol=0, atol=1e-15)
        assert np.allclose(r['dbeta'], dz.sum(0), rtol=0, atol=1e-15) and np.allclose(r['var'], v, rtol=0, atol=1e-12)


def _all_cases(xbf):
    for shape, relu in S.PLAIN_CASES:
        yield 'plain', shape, relu, xbf, False
    for shape, mode in S.POOL_CASES:
        yield 'pooled', shape, mode, xbf, False
    for kind, shape, mode in S.BIG_CASES:
        yield kind, shape, mode, xbf, True


@pytest.mark.parametrize('xbf', [False, True], ids=['x_f32', 'x_bf16'])
def test_every_gpu_case_meets_the_margins_and_keeps_its_planted_edges(xbf):
    for kind, shape, mode, xbf, big in _all_cases(xbf):
        x, g, bt, m = S.plain_case(shape, mode, xbf, big) if kind == 'plain' else S.pooled_case(shape, mode, xbf, big)
        assert m['relu_margin'] > S.MARGIN and m['win_margin'] > S.MARGIN, (kind, shape, mode, xbf, m)
        # ... as the float64 reference itself sees them (on the channels it covers)
        ch = S.subset_channels(shape[-1 if kind == 'plain' else 3]) if big else slice(None)
        xs, gs, bs = x[..., ch], g[ch], bt[ch]
        r = S.plain_ref(xs, gs, bs, None, mode, xbf) if kind == 'plain' else S.pooled_ref(xs, gs, bs, None, shape[4], mode, xbf)
        assert r['relu_margin'] > S.MARGIN and r['win_margin'] > S.MARGIN, (kind, shape, mode, xbf, r['relu_margin'], r['win_margin'])
        assert r['relu_margin'] == pytest.approx(m['relu_margin'], rel=1e-9) and r['win_margin'] == pytest.approx(m['win_margin'], rel=1e-9)
        if xbf:
            assert np.array_equal(o.bf16_round(x), x)
        if kind == 'pooled' and shape[1] >= 2 and shape[2] >= 2:
            i0, j0 = (shape[1] // 2 - 1) * 2, (shape[2] // 2 - 1) * 2
            cell = x[-1, i0:i0 + 2, j0:j0 + 2, -3]
            assert cell[0, 1] == cell[1, 0] == cell.max() > cell[0, 0], (shape, cell)
        if kind == 'pooled' and mode == 2:
            zeros = x[x == 0]
            assert zeros.size >= 2 and np.signbit(zeros).any() and not np.signbit(zeros).all(), (shape, zeros)


def _restated(kind, shape, mode, xbf, dbf, obf, mutant=None):
    """(outputs of the fp32 restatement, float64 reference) of one call as the GPU test makes it."""
    if kind == 'plain':
        x, g, bt, _ = S.plain_case(shape, mode, xbf)
        dy = S.gradient(shape, dbf)
        return (S.plain_f32(x, g, bt, dy, mode, xbf, dbf, obf, mutant), S.plain_ref(x, g, bt, dy, mode, xbf, dbf))
    x, g, bt, _ = S.pooled_case(shape, mode, xbf)
    dp = S.gradient((shape[0], S.pool_out(shape[1], shape[4]), S.pool_out(shape[2], shape[4]), shape[3]), dbf)
    return (S.pooled_f32(x, g, bt, dp, shape[4], mode, xbf, dbf, obf, mutant), S.pooled_ref(x, g, bt, dp, shape[4], mode, xbf, dbf))


def _small_calls():
    for xbf, dbf in S.FORMS:
        for obf in (False, True):
            for shape, relu in S.PLAIN_CASES:
                yield 'plain', shape, relu, xbf, dbf, obf
            for shape, mode in S.POOL_CASES:
                yield 'pooled', shape, mode, xbf, dbf, obf


def test_control_the_fp32_restatement_passes_every_criterion():
    worst = {}
    for call in _small_calls():
        got, ref = _restated(*call)
        if call[1] == (1, 16):
            continue          # one row: y and dx cancel to rounding noise, bounded in the GPU test by this restatement itself
        res = S.check(got, ref, stored=('y', 'p', 'dx') if call[5] else ())
        assert not S.failures(res), (call, S.failures(res), res)
        for k, (_, fig) in res.items():
            worst[k] = max(worst.get(k, 0.0), fig)
    print('fp32 restatement, worst figure per criterion:', ' '.join('%s=%.2e' % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize('mutant', sorted(S.MUTANTS))
def test_mutant_is_rejected_by_the_criterion_named_for_it(mutant):
    named, what = S.MUTANTS[mutant]
    for call in _small_calls():
        kind, shape, mode, xbf, dbf, obf = call
        if (mutant == 'truncate' and not obf) or (mutant == 'dy_as_f32' and not dbf) or \
                (mutant in ('gate_ge', 'relu_after_pool') and (kind, mode) != ('pooled', 2)) or \
                (mutant in ('last_max', 'clip_col_shift', 'valid_leftover_grad') and kind != 'pooled'):
            continue
        got, ref = _restated(*call, mutant=mutant)
        failed = [f for f in S.failures(S.check(got, ref, stored=('y', 'p', 'dx') if obf else ())) if f.startswith(named)]
        if failed:
            print('mutant %s (%s): caught by %s on %s %s mode %d x_bf16=%d dy_bf16=%d out_bf16=%d'
                  % (mutant, what, ', '.join(failed), kind, S.tag(shape), mode, xbf, dbf, obf))
            return
    pytest.fail('no case rejects the mutant %s (%s)' % (mutant, what))
