"""The head, loss, L2-sum, Adam and BatchNorm moving-average kernels of csrc/elementwise.hip on their own (l3_op_head_dense_*,
l3_op_softmax_ce2, l3_op_sumsq, l3_op_adam_scaled, l3_op_bn_moving_update) against the float64 restatements and rounding bounds of
tests/head_ref.py, and the engine's plumbing around them (forward_all, loss_and_head_backward, l2_sums, do_update, read_results)
from the engine's own intermediate values.  tests/test_head_host.py shows on the CPU that a float32 emulation of every kernel
stays within half of each bound on the same inputs.  Every test prints max err / bound before it asserts."""
import numpy as np
import pytest

import head_ref as hr
from l3embedding_amd import _lib
from oracle import l3_oracle as o

pytestmark = pytest.mark.gpu


def within(name, got, ref, bound, mask=None):
    err = np.abs(hr.f64(got) - hr.f64(ref))
    bound = np.broadcast_to(hr.f64(bound), err.shape)
    if mask is not None:
        err, bound = err[mask], bound[mask]
    r = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print('%s: max err / bound = %.3f' % (name, r))
    assert (err <= bound).all(), (name, r)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- dense ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,K,N,relu', hr.DENSE_FWD_CASES)
def test_dense_fwd(gpu_required, B, K, N, relu):
    x, w, b, _ = hr.dense_inputs(B, K, N)
    y = _lib.op_head_dense_fwd(x, w, b, relu)
    within('dense_fwd B=%d K=%d N=%d' % (B, K, N), y, hr.dense_fwd_ref(x, w, b, relu), hr.dense_fwd_bound(x, w, b))


@pytest.mark.parametrize('K,N', [(1030, 130), (7, 2)])
def test_dense_fwd_delta_rows_bit_for_bit(gpu_required, K, N):
    """x = e_k at the first and last k of every K slice returns row k of w plus b exactly: no slice is dropped or read twice."""
    ks, x, w, b = hr.dense_delta_inputs(K, N)
    y = _lib.op_head_dense_fwd(x, w, b, 0)
    bad = [k for i, k in enumerate(ks) if not np.array_equal(bits(y[i]), bits(w[k] + b))]
    print('dense_fwd delta K=%d: %d rows, max err / bound = %.3f (exact)' % (K, len(ks), 0.0 if not bad else np.inf))
    assert bad == [], bad


@pytest.mark.parametrize('B,K,N', hr.DENSE_BWD_CASES)
def test_dense_bwd(gpu_required, B, K, N):
    x, w, _, dy = hr.dense_inputs(B, K, N)
    got = _lib.op_head_dense_bwd(x, w, dy)
    for name, a, r, bd in zip(('dw', 'db', 'dx'), got, hr.dense_bwd_ref(x, w, dy), hr.dense_bwd_bound(x, w, dy)):
        within('dense_bwd %s B=%d K=%d N=%d' % (name, B, K, N), a, r, bd)


@pytest.mark.parametrize('B,K,N', [(9, 1000, 300), (257, 128, 2)])
def test_dense_bwd_one_hot_is_exact(gpu_required, B, K, N):
    x, w, _, _ = hr.dense_inputs(B, K, N)
    for b0, n0 in ((0, 0), (B - 1, N - 1), (B // 2, N // 2)):
        dy = np.zeros((B, N), np.float32)
        dy[b0, n0] = 1
        dw, db, dx = _lib.op_head_dense_bwd(x, w, dy)
        want_dw = np.zeros((K, N), np.float32)
        want_dw[:, n0] = x[b0]
        want_dx = np.zeros((B, K), np.float32)
        want_dx[b0] = w[:, n0]
        assert np.array_equal(dw, want_dw) and np.array_equal(dx, want_dx) and np.array_equal(db, dy.sum(axis=0))
    print('dense_bwd one-hot B=%d K=%d N=%d: max err / bound = 0.000 (exact)' % (B, K, N))


# ---- loss ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('soft', [False, True])
@pytest.mark.parametrize('B', hr.SOFTMAX_B)
def test_softmax_ce(gpu_required, B, soft):
    """Ties, +-40 differences (both classes clipped: gradient exactly 0), q within a few ulp of the clip threshold (left out of the
    gradient comparison by the mask `unsure`, at most 1 % of the rows), one-hot and (0.3, 0.7) labels, gscale 1 / B and 1 / 4B."""
    z, t, kinds = hr.softmax_inputs(B, soft)
    for gscale in (1.0 / B, 1.0 / (4 * B)):
        ref, bound = hr.softmax_ce_ref(z, t, gscale), hr.softmax_ce_bound(z, t, gscale)
        probs, dz, loss, correct = _lib.op_softmax_ce2(z, t, gscale)
        unsure = bound['unsure']
        print('B=%d: %d of %d rows outside the gradient comparison' % (B, unsure.sum(), B))
        assert unsure.sum() <= 0.01 * B
        within('softmax probs B=%d' % B, probs, ref['probs'], bound['probs'])
        within('softmax dlogits B=%d gscale=%g' % (B, gscale), dz, ref['dlogits'], bound['dlogits'], ~unsure)
        within('softmax loss sum B=%d' % B, loss, ref['loss'].sum(), bound['loss_sum'])
        assert correct == ref['correct'].sum()
        far = np.array([k == 'far' for k in kinds])
        assert (dz[far] == 0).all()
        tie = np.array([k == 'tie' for k in kinds])
        assert (probs[tie] == 0.5).all()


def test_softmax_ce_clip_terms(gpu_required):
    """A +-40 difference: q is clipped at 1e-7 and at 1 - 1e-7, the gradient is exactly 0 and the loss is -log(1e-7) or
    -log(1 - 1e-7), whichever class the label names."""
    z = np.array([[-20.0, 20.0]], np.float32)
    for t, want in (((1, 0), -np.log(hr.f64(hr.CE_EPS))), ((0, 1), -np.log(hr.f64(hr.CE_HI)))):
        t = np.array([t], np.float32)
        probs, dz, loss, correct = _lib.op_softmax_ce2(z, t, 1.0)
        within('softmax clip term t=%s' % (t[0],), loss, want, hr.softmax_ce_bound(z, t, 1.0)['loss_sum'])
        assert (dz == 0).all() and correct == float(t[0, 1])


# ---- sums of squares -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sumsq_case():
    base, off, n, izero = hr.sumsq_inputs()
    return base, off, n, izero, hr.sumsq_ref(base, off, n)


@pytest.mark.parametrize('multi', [0, 1])
def test_sumsq(gpu_required, sumsq_case, multi):
    base, off, n, izero, ref = sumsq_case
    got = _lib.op_sumsq(base, off, n, multi)
    bound = hr.sumsq_bound(base, off, n, multi)
    for i in np.argsort(-np.abs(got - ref) / np.maximum(bound, 1e-300))[:3]:
        print('  range n=%d off%%4=%d: err / bound = %.3f' % (n[i], off[i] % 4, abs(got[i] - ref[i]) / max(bound[i], 1e-300)))
    within('sumsq multi=%d' % multi, got, ref, bound)
    assert got[izero] == 0.0


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', hr.ADAM_N)
def test_adam(gpu_required, n):
    """adam_kernel against float64 with gscale != 1 and the L2 boundary n_l2 inside one launch; m, v zero (first step) or warm.
    Elements with g = m = v = 0 behind n_l2 keep their bits; the elements either side of n_l2 are looked at on their own.
    Not covered: a denormal v (|g| gscale is kept >= 1e-15, so g^2 stays normal)."""
    c = hr.ADAM_CONST
    worst = [0.0, 0.0, 0.0]
    for warm in (False, True):
        p, g, m, v, still = hr.adam_inputs(n, warm)
        for n_l2 in hr.adam_l2_counts(n):
            for gscale in hr.ADAM_GSCALE:
                args = (p, g, m, v, n_l2, c['l2x2'], c['lr_t'], c['b1'], c['b2'], c['eps'], np.float32(gscale))
                got = _lib.op_adam_scaled(p, g, m, v, n_l2, c['l2x2'], c['lr_t'], c['b1'], c['b2'], c['eps'], gscale)
                ref, bound = hr.adam_ref(*args), hr.adam_bound(*args)
                for k, (a, r, b) in enumerate(zip(got, ref, bound)):
                    err = np.abs(hr.f64(a) - r)
                    worst[k] = max(worst[k], float((err / np.maximum(b, 1e-300)).max()))
                    assert (err <= b).all(), ('pmv'[k], n, n_l2, gscale, warm, int(np.argmax(err / np.maximum(b, 1e-300))))
                keep = still & (np.arange(n) >= n_l2)
                for a, a0 in zip(got, (p, m, v)):
                    assert np.array_equal(bits(a[keep]), bits(a0[keep]))
                # either side of the boundary: the gradient that went into m says whether the element was decayed
                gi = (hr.f64(got[1]) - hr.f64(c['b1']) * hr.f64(m)) / (1 - hr.f64(c['b1']))
                for i, decayed in ((n_l2 - 1, True), (n_l2, False)):
                    if 0 <= i < n:
                        plain = hr.f64(g[i]) * gscale
                        want = plain + (hr.f64(c['l2x2']) * hr.f64(p[i]) if decayed else 0.0)
                        other = plain + (0.0 if decayed else hr.f64(c['l2x2']) * hr.f64(p[i]))
                        assert abs(gi[i] - want) <= 10 * bound[1][i] < abs(want - other) / 4, (n, n_l2, i, decayed)
    print('adam n=%d: max err / bound = %.3f (p) %.3f (m) %.3f (v)' % (n, worst[0], worst[1], worst[2]))


# ---- BatchNorm moving averages -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zero_debias', [0, 1])
@pytest.mark.parametrize('replicas', [1, 2, 3])
def test_bn_moving_update(gpu_required, zero_debias, replicas):
    """One launch over a table of C = 1, 3, 64, 512, 513 against float64 and against oracle.BNMovingState applied `replicas` times
    (replicas 1 from the batch vectors, 2 and 3 from a gathered buffer with a stride above the packed size and distinct slots).
    bn_moving_pack returns the batch vectors back to back; sentinels behind every C stay."""
    d = hr.bn_inputs(replicas)
    mom = hr.BN_MOMENTUM
    worst = 0.0
    for step in hr.BN_STEPS:
        packed0 = np.full(d['total'] + 5, hr.SENTINEL, np.float32)
        moving, biased, packed = _lib.op_bn_moving_update(d['c'], d['slot_off'], d['moving'], d['biased'], d['batch'], mom,
                                                          zero_debias, step, d['gathered'], replicas, d['stride'], packed0)
        want_packed = np.concatenate([d['batch'][so:so + C] for C, so in zip(d['c'], d['slot_off'])] + [packed0[d['total']:]])
        assert np.array_equal(bits(packed), bits(want_packed))
        for i, (C, so) in enumerate(zip(d['c'], d['slot_off'])):
            m0, b0, vals = d['moving'][so:so + C], d['biased'][so:so + C], hr.bn_values(d, i, replicas)
            ref = hr.bn_moving_ref(m0, b0, vals, mom, zero_debias, step)
            bound = hr.bn_moving_bound(m0, b0, vals, mom, zero_debias, step)
            for a, r, b in zip((moving[so:so + C], biased[so:so + C]), ref, bound):
                err = np.abs(hr.f64(a) - r)
                worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
                assert (err <= b).all(), (C, step)
            assert (moving[so + C:so + C + 3] == hr.SENTINEL).all() and (biased[so + C:so + C + 3] == hr.SENTINEL).all()
            if not zero_debias:
                assert np.array_equal(bits(biased[so:so + C]), bits(b0))
            if step >= replicas:
                # the oracle holds momentum 0.99 in float64, the kernel 0.99f: the restatement at both values gives that difference
                st = o.BNMovingState(bool(zero_debias))
                st.biased['x'], st.step['x'] = hr.f64(b0), step - replicas
                P = {'x': hr.f64(m0)}
                for val in vals:
                    st.update(P, 'x', val)
                ref64 = hr.bn_moving_ref(m0, b0, vals, o.BN_MOMENTUM, zero_debias, step)[0]
                assert np.allclose(ref64, P['x'], rtol=1e-13, atol=0)
                assert (np.abs(hr.f64(moving[so:so + C]) - P['x']) <= bound[0] + np.abs(ref64 - ref[0])).all()
    print('bn_moving_update zero_debias=%d replicas=%d: max err / bound = %.3f' % (zero_debias, replicas, worst))


# ---- the engine's wiring of these kernels ----------------------------------------------------------------------------------------
def _dev_read(ptr, n):
    import torch
    from l3embedding_amd.training_utils import _DevArray
    return torch.as_tensor(_DevArray(ptr, n), device='cuda:0').cpu().numpy().copy()


def _engine(mt, B, GB, zero_debias):
    """An engine with a live head (dense_2 / 64: no row inside the probability clip) and every bias, beta and gamma moved off its
    initial 0 / 1, so that a decay that reached them would show."""
    e = _lib.Engine(mt, B, global_batch=GB, bn_zero_debias=zero_debias, seed=5)
    rng = np.random.RandomState(17)
    for name, shape, tr in e.param_table():
        if tr and not name.endswith('/kernel'):
            e.set_param(name, e.get_param(name, shape) + (0.1 * rng.standard_normal(shape)).astype(np.float32))
    shape = dict((n, s) for n, s, _ in e.param_table())['dense_2/kernel']
    e.set_param('dense_2/kernel', e.get_param('dense_2/kernel', shape) * np.float32(1.0 / 64))
    v, a, l = o.synthetic_batch(B, seed=23)
    e.upload_batch(v, a, l)
    return e, l


def _forward_backward(e):
    e.step_forward(True)
    for b in range(1, e.bucket_count()):
        e.step_backward_bucket(b)
    e.sync()


def _check_head(e, labels, GB):
    """h1, logits, probs, the loss and the four head gradients from the engine's own h0 (taken as given)."""
    B = e.batch
    P = e.get_params()
    w1, b1, w2, b2 = [P['dense_%s' % k] for k in ('1/kernel', '1/bias', '2/kernel', '2/bias')]
    h0 = e.activation('h0').reshape(B, -1)
    h1 = e.activation('h1').reshape(B, -1)
    logits = e.activation('logits').reshape(B, 2)
    probs = e.activation('probs').reshape(B, 2)
    assert h0.shape[1] == w1.shape[0] and np.abs(h0).max() > 0
    within('engine h1', h1, hr.dense_fwd_ref(h0, w1, b1, 1), hr.dense_fwd_bound(h0, w1, b1))
    within('engine logits', logits, hr.dense_fwd_ref(h1, w2, b2, 0), hr.dense_fwd_bound(h1, w2, b2))
    gs = 1.0 / GB
    ce, cb = hr.softmax_ce_ref(logits, labels, gs), hr.softmax_ce_bound(logits, labels, gs)
    assert not cb['unsure'].any() and np.abs(ce['dlogits']).min() > 0
    within('engine probs', probs, ce['probs'], cb['probs'])
    # gradients: each operator's bound at the float64 operands widened by their own bounds, plus what the operand's error brings
    A = np.abs
    dl, e_dl = ce['dlogits'], cb['dlogits']
    g = dict((n, e.get_grad(n, P[n].shape)) for n in ('dense_1/kernel', 'dense_1/bias', 'dense_2/kernel', 'dense_2/bias'))
    bw, bb, bx = hr.dense_bwd_bound(h1, w2, A(dl) + e_dl)
    dw2, db2, dh1 = hr.dense_bwd_ref(h1, w2, dl)
    within('engine dense_2/kernel grad', g['dense_2/kernel'], dw2, bw + A(hr.f64(h1)).T @ e_dl)
    within('engine dense_2/bias grad', g['dense_2/bias'], db2, bb + e_dl.sum(axis=0))
    e_dh1 = bx + e_dl @ A(hr.f64(w2)).T
    mask = h1 > 0
    dz1, e_dz1 = np.where(mask, dh1, 0), np.where(mask, e_dh1, 0)
    bw, bb, _ = hr.dense_bwd_bound(h0, w1, A(dz1) + e_dz1)
    dw1, db1, _ = hr.dense_bwd_ref(h0, w1, dz1)
    within('engine dense_1/kernel grad', g['dense_1/kernel'], dw1, bw + A(hr.f64(h0)).T @ e_dz1)
    within('engine dense_1/bias grad', g['dense_1/bias'], db1, bb + e_dz1.sum(axis=0))
    assert mask.any() and not mask.all() and np.abs(dw1).max() > 0
    # loss = CE mean + 1e-5 sum over the kernels oracle.l2_penalty regularises; accuracy exactly
    kernels = [n for n, _, _, kind in o.param_table(e.model_type) if kind == 'kernel']
    assert sorted(kernels) == sorted(n for n in P if n.endswith('/kernel')) and len(kernels) <= hr.SUMSQ_MAX_SEGS
    reg = reg_bound = 0.0
    for n in kernels:
        flat = P[n].ravel()
        reg += 1e-5 * hr.sumsq_ref(flat, [0], [flat.size])[0]
        reg_bound += 1e-5 * max(hr.sumsq_bound(np.concatenate([np.zeros(a, np.float32), flat]), [a], [flat.size], 1)[0]
                                for a in range(4))          # whatever the tensor's alignment in the arena
    loss, acc = e.step_results()
    want = ce['loss'].sum() / B + reg
    # + the engine's 1e-5f (2.6e-8 relative) and the rounding of the double result to float32
    within('engine loss', loss, want, cb['loss_sum'] / B + reg_bound + 2.6e-8 * reg + hr.EPS * abs(want))
    assert acc == np.float32(ce['correct'].sum()) / np.float32(B)
    assert np.isclose(reg, o.l2_penalty(P, e.model_type), rtol=1e-12)
    return P


def _check_update(e, P, state, lr, grad_scale, zero_debias):
    """step_update from the engine's own gradients and batch statistics: Adam on every trainable tensor (decay on kernels only),
    the moving averages of every BatchNormalization.  `state` carries the float64 moments / biased accumulators and the bounds on
    their float32 counterparts from one step to the next."""
    G = e.get_grads()
    ptr, n = e.bn_stats_pack()
    e.sync()
    stats = _dev_read(ptr, n)
    e.step_update(lr, grad_scale)
    e.sync()
    Q = e.get_params()
    state['t'] += 1
    c = hr.ADAM_CONST
    lr_t = hr.adam_lr_t(lr, state['t'], c['b1'], c['b2'])
    worst = 0.0
    for name, g in G.items():
        p = P[name].ravel()
        m, v, em, ev = state['adam'].get(name, (np.zeros(p.size), np.zeros(p.size), 0.0, 0.0))
        n_l2 = p.size if name.endswith('/kernel') else 0
        args = (p, g.ravel(), m, v, n_l2, c['l2x2'], lr_t.v, c['b1'], c['b2'], c['eps'], np.float32(grad_scale))
        ref = hr.adam_ref(*args)
        bound = hr.adam_bound(*args[:6], lr_t, *args[7:], em=em, ev=ev)
        err = np.abs(hr.f64(Q[name].ravel()) - ref[0])
        worst = max(worst, float((err / np.maximum(bound[0], 1e-300)).max()))
        assert (err <= bound[0]).all(), (name, state['t'], worst)
        state['adam'][name] = (ref[1], ref[2], bound[1], bound[2])
    print('engine %s adam step %d: max err / bound = %.3f over %d tensors' % (e.model_type, state['t'], worst, len(G)))
    off, worst = 0, 0.0
    for name, shape, _ in e.param_table():
        if not name.endswith('/moving_mean'):
            continue
        C = shape[0]
        for nm, val in ((name, stats[off:off + C]), (name[:-len('moving_mean')] + 'moving_variance', stats[off + C:off + 2 * C])):
            b, eb = state['bn'].get(nm, (np.zeros(C), 0.0))
            ref = hr.bn_moving_ref(P[nm], b, val[None, :], hr.BN_MOMENTUM, zero_debias, state['t'])
            bound = hr.bn_moving_bound(P[nm], b, val[None, :], hr.BN_MOMENTUM, zero_debias, state['t'], eb=eb)
            err = np.abs(hr.f64(Q[nm]) - ref[0])
            worst = max(worst, float((err / np.maximum(bound[0], 1e-300)).max()))
            assert (err <= bound[0]).all(), (nm, state['t'])
            assert state['t'] > 1 or not np.array_equal(Q[nm], P[nm])      # (a debiased average of one repeated value stays)
            state['bn'][nm] = (ref[1], bound[1])
        off += 2 * C
    assert off == n
    print('engine %s moving averages step %d: max err / bound = %.3f' % (e.model_type, state['t'], worst))
    return Q


@pytest.mark.parametrize('mt,B,GB,zero_debias', [('tiny_L3', 3, 0, True), ('tiny_L3', 3, 0, False), ('cnn_L3_melspec2', 2, 8, True)])
def test_engine_head_and_update_wiring(gpu_required, mt, B, GB, zero_debias):
    """Two steps through the public Engine.  Before each update: the head, loss and head gradients from the engine's own h0
    (gscale = 1 / global_batch, the in-place ReLU backward, the concat order of h0 against dense_1's rows).  Then step_update(lr,
    grad_scale=0.25): every trainable tensor within the Adam bound of the float64 update from the GPU's gradient x 0.25 with L2
    decay on kernels only (a merged launch must not decay the bias / BatchNorm tensors behind a kernel), and every moving mean /
    variance within its bound of the update from the batch statistics the engine holds (bn_stats_pack)."""
    e, labels = _engine(mt, B, GB, zero_debias)
    state = dict(t=0, adam={}, bn={})
    try:
        for _ in range(2):
            _forward_backward(e)
            P = _check_head(e, labels, GB if GB else B)
            _check_update(e, P, state, 1e-4, 0.25, zero_debias)
        assert e.optimizer_steps() == (2, 2)
    finally:
        e.close()
