"""CPU checks of tests/head_ref.py, the yardstick of tests/test_head_gpu.py: on every input set of the GPU tests the float32
emulation of each kernel lies within HALF of the kernel's rounding bound of the float64 restatement (so the inputs and the bounds
are sound before the code under test is looked at), and each restatement equals oracle.l3_oracle on one case."""
import numpy as np
import pytest

import head_ref as hr
from l3embedding_amd import _build, _lib
from oracle import l3_oracle as o


def ratio(name, got, ref, bound, mask=None):
    err = np.abs(hr.f64(got) - hr.f64(ref))
    bound = np.broadcast_to(hr.f64(bound), err.shape)
    if mask is not None:
        err, bound = err[mask], bound[mask]
    r = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print('%s: max err / bound = %.3f' % (name, r))
    return err, bound


def within_half(name, got, ref, bound, mask=None):
    err, bound = ratio(name, got, ref, bound, mask)
    assert (err <= 0.5 * bound).all(), name


@pytest.mark.parametrize('B,K,N,relu', hr.DENSE_FWD_CASES)
def test_dense_fwd_emulation_within_half_bound(B, K, N, relu):
    x, w, b, _ = hr.dense_inputs(B, K, N)
    within_half('dense_fwd', hr.dense_fwd_emu(x, w, b, relu), hr.dense_fwd_ref(x, w, b, relu), hr.dense_fwd_bound(x, w, b))


@pytest.mark.parametrize('K,N', [(1030, 130), (7, 2)])
def test_dense_fwd_delta_is_exact_in_the_emulation(K, N):
    ks, x, w, b = hr.dense_delta_inputs(K, N)
    assert ks[0] == 0 and ks[-1] == K - 1
    want = w[ks] + b
    assert np.array_equal(hr.f64(want), hr.f64(w[ks]) + hr.f64(b))          # exactly representable
    assert np.array_equal(hr.dense_fwd_emu(x, w, b, 0), want)


@pytest.mark.parametrize('B,K,N', hr.DENSE_BWD_CASES)
def test_dense_bwd_emulation_within_half_bound(B, K, N):
    x, w, _, dy = hr.dense_inputs(B, K, N)
    for name, got, ref, bound in zip(('dw', 'db', 'dx'), hr.dense_bwd_emu(x, w, dy), hr.dense_bwd_ref(x, w, dy),
                                     hr.dense_bwd_bound(x, w, dy)):
        within_half('dense_bwd ' + name, got, ref, bound)


@pytest.mark.parametrize('soft', [False, True])
@pytest.mark.parametrize('B', hr.SOFTMAX_B)
def test_softmax_ce_emulation_within_half_bound(B, soft):
    z, t, kinds = hr.softmax_inputs(B, soft)
    for gscale in (1.0 / B, 1.0 / (4 * B)):
        ref, bound, emu = hr.softmax_ce_ref(z, t, gscale), hr.softmax_ce_bound(z, t, gscale), hr.softmax_ce_emu(z, t, gscale)
        unsure = bound['unsure']
        assert unsure.sum() <= 0.01 * B
        assert all(kinds[i] in ('far', 'edge') for i in np.nonzero(unsure)[0])
        assert all(unsure[i] for i, k in enumerate(kinds) if k == 'edge')     # the edge rows really are at the threshold
        within_half('probs', emu['probs'], ref['probs'], bound['probs'])
        within_half('dlogits', emu['dlogits'], ref['dlogits'], bound['dlogits'], ~unsure)
        within_half('loss sum', emu['loss_sum'], ref['loss'].sum(), bound['loss_sum'])
        assert emu['correct'] == ref['correct'].sum()
        far = np.array([k == 'far' for k in kinds])
        assert (emu['dlogits'][far] == 0).all() and (ref['dlogits'][far] == 0).all()


def test_softmax_ce_clip_terms():
    """A +-40 difference clips one class at 1e-7 and the other at 1 - 1e-7: the loss is -log of the clipped label's class."""
    z = np.array([[-20.0, 20.0]], hr.F)
    for t, want in (((1, 0), -np.log(hr.f64(hr.CE_EPS))), ((0, 1), -np.log(hr.f64(hr.CE_HI)))):
        ref = hr.softmax_ce_ref(z, np.array([t], hr.F), 1.0)
        assert ref['loss'][0] == want and (ref['dlogits'] == 0).all()
        emu = hr.softmax_ce_emu(z, np.array([t], hr.F), 1.0)
        assert (emu['dlogits'] == 0).all()
        assert abs(emu['loss_sum'] - want) <= 0.5 * hr.softmax_ce_bound(z, np.array([t], hr.F), 1.0)['loss_sum']


@pytest.mark.parametrize('multi', [0, 1])
def test_sumsq_emulation_within_half_bound(multi):
    base, off, n, izero = hr.sumsq_inputs()
    assert sorted(set(off % 4)) == [0, 1, 2, 3] and any(nn < ((4 - (oo & 3)) & 3) for oo, nn in zip(off, n))
    emu, ref = hr.sumsq_emu(base, off, n, multi), hr.sumsq_ref(base, off, n)
    within_half('sumsq multi=%d' % multi, emu, ref, hr.sumsq_bound(base, off, n, multi))
    assert emu[izero] == 0.0 and ref[izero] == 0.0


@pytest.mark.parametrize('n', hr.ADAM_N)
def test_adam_emulation_within_half_bound(n):
    for warm in (False, True):
        p, g, m, v, still = hr.adam_inputs(n, warm)
        for n_l2 in hr.adam_l2_counts(n):
            for gscale in hr.ADAM_GSCALE:
                assert (np.abs(hr.f64(g[g != 0])) * gscale >= 1e-15).all()
                args = (p, g, m, v, n_l2, hr.ADAM_CONST['l2x2'], hr.ADAM_CONST['lr_t'], hr.ADAM_CONST['b1'], hr.ADAM_CONST['b2'],
                        hr.ADAM_CONST['eps'], hr.F(gscale))
                emu, ref, bound = hr.adam_emu(*args), hr.adam_ref(*args), hr.adam_bound(*args)
                for name, a, r, b in zip('pmv', emu, ref, bound):
                    err = np.abs(hr.f64(a) - r)
                    assert (err <= 0.5 * b).all(), (name, n, n_l2, gscale, warm, float((err / np.maximum(b, 1e-300)).max()))
                keep = still & (np.arange(n) >= n_l2)
                assert keep.any() or n_l2 == n
                for a, a0 in zip(emu, (p, m, v)):
                    assert np.array_equal(a[keep].view(np.uint32), a0[keep].view(np.uint32))


@pytest.mark.parametrize('zero_debias', [0, 1])
@pytest.mark.parametrize('replicas', [1, 2, 3])
def test_bn_moving_emulation_within_half_bound(zero_debias, replicas):
    d = hr.bn_inputs(replicas)
    for step in hr.BN_STEPS:
        for i, (C, so) in enumerate(zip(d['c'], d['slot_off'])):
            vals = hr.bn_values(d, i, replicas)
            args = (d['moving'][so:so + C], d['biased'][so:so + C], vals, hr.BN_MOMENTUM, zero_debias, step)
            for name, a, r, b in zip(('moving', 'biased'), hr.bn_moving_emu(*args), hr.bn_moving_ref(*args), hr.bn_moving_bound(*args)):
                within_half('bn %s C=%d step=%d' % (name, C, step), a, r, b)
    if replicas > 1:
        slots = [d['gathered'][r * d['stride']:r * d['stride'] + d['total']] for r in range(replicas)]
        assert all(np.abs(a - b).min() > 1 for k, a in enumerate(slots) for b in slots[k + 1:])


# ---- pins: each restatement against oracle.l3_oracle on one case ----------------------------------------------------------------
@pytest.fixture(scope='module')
def oracle_step():
    P = o.init_params('tiny_L3', seed=7)
    P['dense_2/kernel'] = (P['dense_2/kernel'] / 64).astype(np.float32)      # keeps every row inside the probability clip
    P['dense_1/bias'] = (0.1 * np.random.RandomState(3).standard_normal(P['dense_1/bias'].shape)).astype(np.float32)
    v, a, l = o.synthetic_batch(3, seed=11)
    out, grads = o.loss_and_grads('tiny_L3', P, v, a, l, True, np.float64)
    return P, l, out, grads


def test_restatements_equal_the_oracle_head(oracle_step):
    P, l, out, grads = oracle_step
    f = out['fwd']
    h0, h1 = f['h0'], f['h1']
    assert np.allclose(hr.dense_fwd_ref(h0, P['dense_1/kernel'], P['dense_1/bias'], 1), h1, rtol=1e-13, atol=0)
    assert np.allclose(hr.dense_fwd_ref(h1, P['dense_2/kernel'], P['dense_2/bias'], 0), out['logits'], rtol=1e-13, atol=1e-300)
    ce = hr.softmax_ce_ref(out['logits'], l, 1.0 / 3)
    assert np.allclose(ce['probs'], out['probs'], rtol=1e-13, atol=0)
    assert ((ce['q'] > 1e-3) & (ce['q'] < 1 - 1e-3)).all()
    assert np.isclose(ce['loss'].mean(), out['data_loss'], rtol=1e-13)
    assert ce['correct'].mean() == out['acc']
    reg2 = 2 * o.L2_WEIGHT * hr.f64(P['dense_2/kernel'])
    dw2, db2, dh1 = hr.dense_bwd_ref(h1, P['dense_2/kernel'], ce['dlogits'])
    assert np.allclose(dw2 + reg2, grads['dense_2/kernel'], rtol=1e-12, atol=1e-18)
    assert np.allclose(db2, grads['dense_2/bias'], rtol=1e-12, atol=1e-18)
    dz1 = np.where(h1 > 0, dh1, 0)
    dw1, db1, _ = hr.dense_bwd_ref(h0, P['dense_1/kernel'], dz1)
    assert np.allclose(dw1 + 2 * o.L2_WEIGHT * hr.f64(P['dense_1/kernel']), grads['dense_1/kernel'], rtol=1e-12, atol=1e-18)
    assert np.allclose(db1, grads['dense_1/bias'], rtol=1e-12, atol=1e-18)
    assert np.abs(grads['dense_1/kernel']).max() > 0


def test_sumsq_restatement_equals_the_oracle_l2_penalty(oracle_step):
    P = oracle_step[0]
    kernels = [n for n, _, _, kind in o.param_table('tiny_L3') if kind == 'kernel']
    base = np.concatenate([P[n].ravel() for n in kernels])
    n = np.array([P[k].size for k in kernels])
    off = np.concatenate([[0], np.cumsum(n)[:-1]])
    assert np.isclose(o.L2_WEIGHT * hr.sumsq_ref(base, off, n).sum(), o.l2_penalty(P, 'tiny_L3'), rtol=1e-13)


def test_adam_restatement_equals_the_oracle():
    p, g, m, v, _ = hr.adam_inputs(257, True)
    n_l2, l2x2, gscale, lr = 100, 2 * o.L2_WEIGHT, 0.25, 1e-4
    st = o.AdamState()
    st.t, st.m, st.v = 1, {'x': hr.f64(m)}, {'x': hr.f64(v)}
    P = {'x': hr.f64(p).copy()}
    grad = hr.f64(g) * gscale + np.where(np.arange(257) < n_l2, l2x2 * hr.f64(p), 0.0)
    o.adam_update(P, {'x': grad}, st, lr)
    lr_t = lr * np.sqrt(1.0 - o.ADAM_B2 ** 2) / (1.0 - o.ADAM_B1 ** 2)
    pn, mn, vn = hr.adam_ref(p, g, m, v, n_l2, l2x2, lr_t, o.ADAM_B1, o.ADAM_B2, o.ADAM_EPS, gscale)
    assert np.allclose(pn, P['x'], rtol=1e-14, atol=0) and np.allclose(mn, st.m['x'], rtol=1e-13, atol=0)
    assert np.allclose(vn, st.v['x'], rtol=1e-13, atol=0)


@pytest.mark.parametrize('zero_debias', [False, True])
def test_bn_moving_restatement_equals_the_oracle(zero_debias):
    d = hr.bn_inputs(3)
    i, C, so = 3, int(d['c'][3]), int(d['slot_off'][3])
    vals = hr.bn_values(d, i, 3)
    st = o.BNMovingState(zero_debias)
    st.biased['x'], st.step['x'] = hr.f64(d['biased'][so:so + C]), 4
    P = {'x': hr.f64(d['moving'][so:so + C])}
    for val in vals:
        st.update(P, 'x', val)
    mv, b = hr.bn_moving_ref(d['moving'][so:so + C], d['biased'][so:so + C], vals, o.BN_MOMENTUM, zero_debias, 7)
    assert np.allclose(mv, P['x'], rtol=1e-13, atol=0)
    if zero_debias:
        assert np.allclose(b, st.biased['x'], rtol=1e-13, atol=0)


def test_head_ops_refuse_what_the_launch_cannot_hold():
    """(K + 8 N) * 4 bytes of dynamic LDS above 64 KiB, and ranges outside the base buffer, are L3_EINVAL before any launch (and
    before the device is looked for: this runs without a GPU)."""
    _build.build()
    x = np.zeros((1, 16384), np.float32)
    with pytest.raises(_lib.L3Error, match='dynamic LDS'):
        _lib.op_head_dense_fwd(x, np.zeros((16384, 8), np.float32), np.zeros(8, np.float32), 0)
    with pytest.raises(_lib.L3Error, match='dynamic LDS'):
        _lib.op_head_dense_bwd(np.zeros((1, 1), np.float32), np.zeros((1, 16385), np.float32), np.zeros((1, 16385), np.float32))
    with pytest.raises(_lib.L3Error, match='outside base'):
        _lib.op_sumsq(np.zeros(8, np.float32), [4], [5], 1)
    with pytest.raises(_lib.L3Error, match='range count'):
        _lib.op_sumsq(np.zeros(8, np.float32), [0] * 25, [1] * 25, 1)
