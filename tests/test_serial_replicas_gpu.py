"""Serial replicas: the R replicas of multi_gpu_model (training_utils.py:121-170) one after another on ONE engine
(l3_replicas_upload* -> l3_step_replicas / l3_eval_replicas), from the fold kernel up to train_serial_replicas.

The reference of the step is the data-parallel step by hand, the scheme of test_dp_native_gpu._emulate: one engine per slice,
forward and every backward bucket, the gradient arenas summed in replica order, the packed BatchNorm batch statistics concatenated
replica-major into bn_stats_replicas(R), step_update.  It does the same additions in the same order, so the serial step must equal
it bit for bit; the float64 oracle (oracle.dp_train_step) anchors the whole step with the bounds of the native data-parallel test.
Controls show that the comparison sees the order of the replicas."""
import json
import os

import numpy as np
import pytest

from dp_native_worker import DATA_SEED, SEED, live_head
from l3embedding_amd import _lib
from oracle import l3_oracle as o

pytestmark = pytest.mark.gpu
T = 48000


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _arena(e):
    import torch
    from l3embedding_amd.training_utils import _DevArray
    ptr, n = e.grad_arena()
    e.sync()
    return torch.as_tensor(_DevArray(ptr, n), device='cuda:0').cpu().numpy()


# ---- the fold kernel alone ------------------------------------------------------------------------------------------------
FOLD_SIZES = (1, 3, 4, 5, 63, 64, 65, 1023, 1025, 2 ** 20 + 3)


def _fold_operands(n, seed):
    """Two float32 vectors whose element-wise sums cover: exact sums, sums that round (magnitudes up to 2^24 apart), subnormal
    operands and subnormal results, +0 / -0 in every pairing, cancellation to +0."""
    rs = np.random.RandomState(seed)
    a = (rs.randn(n) * np.exp2(rs.randint(-30, 30, n))).astype(np.float32)
    b = (rs.randn(n) * np.exp2(rs.randint(-30, 30, n))).astype(np.float32)
    tiny = np.float32(2.0 ** -149)
    special = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (tiny, tiny), (tiny, -tiny), (3 * tiny, 2.0 ** -126),
               (2.0 ** -126, -2.0 ** -127), (1.0, 2.0 ** -24), (1.0, 3 * 2.0 ** -25), (16777216.0, 1.0), (1.5, -1.5),
               (-0.0, tiny), (3.4e38, -3.4e38), (1e-40, 1e-41)]
    idx = rs.permutation(n)[:min(n, 4 * len(special))]
    for k, i in enumerate(idx):
        a[i], b[i] = special[k % len(special)]
    return a, b


@pytest.mark.parametrize('off', [0, 1, 3])
@pytest.mark.parametrize('mode', ['set', 'add', 'out'])
def test_arena_fold_is_numpy_float32_addition(gpu_required, mode, off):
    """acc = g, acc += g and g = acc + g on [off, off + n) of two arenas: the bits of NumPy's float32 a + b at every size around
    the 4-float vectors and the 256-thread blocks, from a start that is and is not 16-byte aligned; nothing outside the range moves."""
    for n in FOLD_SIZES:
        total = off + n + 5
        acc, g = _fold_operands(total, seed=1000 + n)
        got_acc, got_g = _lib.op_arena_fold(acc, g, off, n, mode)
        want_acc, want_g = acc.copy(), g.copy()
        s = slice(off, off + n)
        if mode == 'set':
            want_acc[s] = g[s]
        elif mode == 'add':
            want_acc[s] = acc[s] + g[s]
        else:
            want_g[s] = acc[s] + g[s]
        assert want_acc.dtype == np.float32 and want_g.dtype == np.float32
        assert np.array_equal(bits(got_acc), bits(want_acc)), (n, mode, off)
        assert np.array_equal(bits(got_g), bits(want_g)), (n, mode, off)
    with pytest.raises(_lib.L3Error, match='outside the 8 floats'):
        _lib.op_arena_fold(np.zeros(8, np.float32), np.zeros(8, np.float32), 5, 4, 'add')


# ---- the step against the hand emulation -----------------------------------------------------------------------------------
def _global_batch(GB, form, seed=DATA_SEED):
    """float: oracle.synthetic_batch; raw: uint8 frames, int16 PCM, int32 one-hot labels; aug: raw + parameter records."""
    if form == 'float':
        return o.synthetic_batch(GB, seed=seed)
    rs = np.random.RandomState(seed)
    v = rs.randint(0, 256, (GB, 224, 224, 3)).astype(np.uint8)
    a = (rs.randn(GB, 1, T) * 6000).clip(-32768, 32767).astype(np.int16)
    lab = rs.randint(0, 2, GB)
    return v, a, np.stack([lab, 1 - lab], 1).astype(np.int32)


def _aug_params(GB, seed=7):
    import random
    from l3embedding_amd import augment
    return augment.draw_params(random.Random(seed), GB)


def _upload_slice(e, form, batch, lo, hi, params=None):
    v, a, l = batch
    if form == 'float':
        e.upload_batch(v[lo:hi], a[lo:hi], l[lo:hi])
    elif form == 'aug':
        e.upload_batch_raw_aug(v[lo:hi], a[lo:hi], l[lo:hi], params[lo:hi], params['u_gain'][lo:hi])
    else:
        e.upload_batch_raw(v[lo:hi], a[lo:hi], l[lo:hi])


def _at(x, k):
    """Step k's entry of a per-step list, or the one entry every step uses."""
    return x[k] if isinstance(x, list) else x


def _emulate(mt, GB, R, steps, lr, batch, form='float', params=None, dtype='f32'):
    """The R-replica step by hand: engine r holds slice r (test_dp_native_gpu._emulate).  batch / params: one for every step, or a
    list with one per step."""
    import torch
    from l3embedding_amd.training_utils import _DevArray
    B = GB // R
    engs, flats = [], []
    for r in range(R):
        e = _lib.Engine(mt, B, seed=SEED, global_batch=GB, dtype=dtype)
        live_head(e)
        ptr, n = e.grad_arena()
        engs.append(e)
        flats.append(torch.as_tensor(_DevArray(ptr, n), device='cuda:0'))
    losses, accs = [], []
    for k in range(steps):
        for r, e in enumerate(engs):
            if k == 0 or isinstance(batch, list):
                _upload_slice(e, form, _at(batch, k), r * B, (r + 1) * B, _at(params, k))
            e.step_forward(True)
            for b in range(1, e.bucket_count()):
                e.step_backward_bucket(b)
            e.sync()
        total = flats[0]
        for f in flats[1:]:
            total = total + f                          # replica order: ((f0 + f1) + f2) + ...
        total = total.clone()
        for f in flats:
            f.copy_(total)
        packed = []
        for e in engs:
            ptr, n = e.bn_stats_pack()
            e.sync()
            packed.append(torch.as_tensor(_DevArray(ptr, n), device='cuda:0').clone())
        gathered = torch.cat(packed)
        for e in engs:
            torch.as_tensor(_DevArray(e.bn_stats_replicas(R), gathered.numel()), device='cuda:0').copy_(gathered)
        torch.cuda.synchronize()
        for e in engs:
            e.step_update(lr, 1.0)
            e.sync()
        res = [e.step_results() for e in engs]
        losses.append(sum(B * r[0] for r in res) / GB)
        accs.append(sum(B * r[1] for r in res) / GB)
    out = dict(params=engs[0].get_params(), arena=flats[0].cpu().numpy(), losses=losses, accs=accs, steps=engs[0].optimizer_steps())
    for e in engs:
        e.close()
    return out


def _serial(mt, GB, R, steps, lr, batch, form='float', params=None, dtype='f32', staged=False):
    """The same step on ONE engine.  batch / params: as _emulate's.  staged: every step's batch after the first arrives over the
    copy stream while the step before it runs, and a step's results are read after the next step has been enqueued."""
    e = _lib.Engine(mt, GB // R, seed=SEED, global_batch=GB, dtype=dtype)
    live_head(e)

    def send(stage, k):
        v, a, l = _at(batch, k)
        p = _at(params, k)
        if form == 'float':
            e.replicas_upload(v, a, l, R)
        elif form == 'aug':
            (e.replicas_stage_raw_aug if stage else e.replicas_upload_raw_aug)(v, a, l, p, p['u_gain'], R)
        else:
            (e.replicas_stage_raw if stage else e.replicas_upload_raw)(v, a, l, R)
    losses, accs = [], []
    if not staged:
        for k in range(steps):
            if k == 0 or isinstance(batch, list):
                send(False, k)
            e.step_replicas(lr)
            loss, acc = e.step_results()
            losses.append(loss), accs.append(acc)
    else:
        send(False, 0)                                 # the first batch is uploaded, every later one staged behind a running step
        for k in range(steps):
            e.step_replicas(lr)
            e.results_enqueue(k & 1)
            if k + 1 < steps:
                send(True, k + 1)
            if k > 0:
                loss, acc = e.results_wait((k - 1) & 1)
                losses.append(loss), accs.append(acc)
        loss, acc = e.results_wait((steps - 1) & 1)
        losses.append(loss), accs.append(acc)
    out = dict(params=e.get_params(), arena=_arena(e), losses=losses, accs=accs, steps=e.optimizer_steps())
    e.close()
    return out


def _same_bits(got, want):
    diff = [k for k in want['params'] if not np.array_equal(bits(got['params'][k]), bits(want['params'][k]))]
    assert diff == [], diff                            # every parameter and every moving statistic
    assert np.array_equal(bits(got['arena']), bits(want['arena']))


def _check_step(got, em, R, steps):
    names = list(em['params'])
    assert any('moving_mean' in k for k in names) and any('moving_variance' in k for k in names)
    _same_bits(got, em)
    assert tuple(got['steps']) == (steps, R * steps) == tuple(em['steps'])
    for g, w in ((got['losses'], em['losses']), (got['accs'], em['accs'])):
        assert len(g) == steps
        for x, y in zip(g, w):
            print('serial %.8f  emulation %.8f' % (x, y))
            assert abs(x - y) <= 1e-6 * max(1.0, abs(y)), (g, w)
    live = np.count_nonzero(got['arena']) / got['arena'].size
    print('non-zero share of the summed gradient arena after the last step: %.3f' % live)
    assert live > 0.5                                  # a sum of zeros would check nothing


def _permuted(batch, order, B):
    rows = np.concatenate([np.arange(r * B, (r + 1) * B) for r in order])
    return tuple(x[rows] for x in batch)


def _oracle(mt, GB, R, steps, lr, batch):
    P = o.init_params(mt, seed=SEED)
    e0 = _lib.Engine(mt, 2, seed=SEED)
    live_head(e0)
    P.update(e0.get_params())                          # the engine's own initial weights
    e0.close()
    v, a, l = batch
    adam, bn = o.AdamState(), o.BNMovingState(zero_debias=True)
    losses = [o.dp_train_step(mt, P, adam, bn, v, a, l, lr, R)['loss'] for _ in range(steps)]
    return P, losses


def test_step_replicas_melspec2_two_replicas(gpu_required):
    """cnn_L3_melspec2, global batch 6 as 2 replicas of 3, two steps at lr 1e-3: the bits of the hand emulation; the oracle's bounds
    of the native data-parallel test (moving variances < 2e-3, loss within 1e-3); the replicas fed in the other order -- with two
    replicas, reversed and slices 0 and 1 swapped are one permutation -- change the moving statistics and the weights."""
    mt, GB, R, steps, lr = 'cnn_L3_melspec2', 6, 2, 2, 1e-3
    batch = _global_batch(GB, 'float')
    em = _emulate(mt, GB, R, steps, lr, batch)
    got = _serial(mt, GB, R, steps, lr, batch)
    _check_step(got, em, R, steps)
    rev = _serial(mt, GB, R, steps, lr, _permuted(batch, [1, 0], GB // R))
    moving = [k for k in em['params'] if 'moving_' in k]
    d_moving = max(relerr(rev['params'][k], em['params'][k]) for k in moving)
    d_all = max(relerr(rev['params'][k], em['params'][k]) for k in em['params'])
    print('control, replicas in the other order: moving statistics %.1e, all parameters %.1e' % (d_moving, d_all))
    assert d_moving > 0 and d_all > 0
    P, oracle_losses = _oracle(mt, GB, R, steps, lr, batch)
    d_var = max(relerr(got['params'][k], P[k]) for k in em['params'] if 'moving_variance' in k)
    print('oracle: moving variances %.1e, losses %s against %s' % (d_var, got['losses'], oracle_losses))
    assert d_var < 2e-3
    for g, w in zip(got['losses'], oracle_losses):
        assert abs(g - w) < 1e-3 * max(1.0, abs(w)), (g, w)


@pytest.mark.parametrize('lr', [0.0, 1e-3])
def test_step_replicas_tiny_three_replicas(gpu_required, lr):
    """tiny_L3, global batch 6 as 3 replicas of 2, three steps.  lr 0: frozen weights, the moving statistics depend on the data and
    on the order of the replicas alone -- within 2e-5 of the oracle's three virtual replicas, and the reversed order changes them.
    lr 1e-3: slices 0 and 1 swapped change the weights."""
    mt, GB, R, steps = 'tiny_L3', 6, 3, 3
    batch = _global_batch(GB, 'float')
    em = _emulate(mt, GB, R, steps, lr, batch)
    got = _serial(mt, GB, R, steps, lr, batch)
    _check_step(got, em, R, steps)
    moving = [k for k in em['params'] if 'moving_' in k]
    rev = _serial(mt, GB, R, steps, lr, _permuted(batch, [2, 1, 0], GB // R))
    d_rev = max(relerr(rev['params'][k], em['params'][k]) for k in moving)
    print('control, replicas in reverse order: moving statistics %.1e' % d_rev)
    assert d_rev > 0
    if lr > 0:
        swap = _serial(mt, GB, R, steps, lr, _permuted(batch, [1, 0, 2], GB // R))
        d_swap = max(relerr(swap['params'][k], em['params'][k]) for k in em['params'])
        print('control, slices 0 and 1 swapped: %.1e' % d_swap)
        assert d_swap > 0
    else:
        P, _ = _oracle(mt, GB, R, steps, lr, batch)
        d_mean = max(relerr(got['params'][k], P[k]) for k in moving if 'moving_mean' in k)
        d_var = max(relerr(got['params'][k], P[k]) for k in moving if 'moving_variance' in k)
        print('oracle: moving means %.1e, variances %.1e' % (d_mean, d_var))
        assert d_mean < 2e-5 and d_var < 2e-5, (d_mean, d_var)


def test_one_replica_is_step_resident(gpu_required):
    mt, B, steps, lr = 'tiny_L3', 3, 2, 1e-3
    batch = _global_batch(B, 'float')
    got = _serial(mt, B, 1, steps, lr, batch)
    e = _lib.Engine(mt, B, seed=SEED, global_batch=B)
    live_head(e)
    e.upload_batch(*batch)
    losses = []
    for _ in range(steps):
        e.step_resident(lr)
        losses.append(e.step_results()[0])
    want = dict(params=e.get_params(), arena=_arena(e))
    assert e.optimizer_steps() == tuple(got['steps']) == (steps, steps)
    e.close()
    _same_bits(got, want)
    assert losses == got['losses']


# ---- input forms -----------------------------------------------------------------------------------------------------------
FORMS = dict(mt='tiny_L3', GB=4, R=2, steps=3, lr=1e-3)


@pytest.fixture(scope='module')
def raw_runs(gpu_required):
    """The uploaded raw run and the uploaded augmented run: the references of the staged ones."""
    c = FORMS
    batch = [_global_batch(c['GB'], 'raw', seed=DATA_SEED + k) for k in range(c['steps'])]       # another batch every step
    params = [_aug_params(c['GB'], seed=7 + k) for k in range(c['steps'])]
    raw = _serial(c['mt'], c['GB'], c['R'], c['steps'], c['lr'], batch, form='raw')
    aug = _serial(c['mt'], c['GB'], c['R'], c['steps'], c['lr'], batch, form='aug', params=params)
    return batch, params, raw, aug


def test_raw_global_batch_equals_its_scaled_floats(raw_runs):
    """Slice r of a raw global batch is scaled by upload_batch_raw's kernels from rows [rB, (r + 1)B): the run equals the float
    run of the rows op_preprocess scales (the same kernels) and the emulation fed upload_batch_raw per slice, bit for bit."""
    c = FORMS
    batch, _, raw, _ = raw_runs
    floats = []
    for v8, a16, lab in batch:
        v, a = _lib.op_preprocess(video_u8=v8, audio_i16=a16)
        floats.append((v, a.reshape(a16.shape), lab.astype(np.float32)))
    flt = _serial(c['mt'], c['GB'], c['R'], c['steps'], c['lr'], floats)
    _same_bits(raw, flt)
    assert raw['losses'] == flt['losses'] and tuple(raw['steps']) == (c['steps'], c['R'] * c['steps'])
    em = _emulate(c['mt'], c['GB'], c['R'], c['steps'], c['lr'], batch, form='raw')
    _same_bits(raw, em)


def test_staged_global_batch_equals_the_uploaded_one(raw_runs):
    """Every batch after the first staged behind the running step and adopted by the next; each step's results read through
    results_enqueue / results_wait after the following step was enqueued."""
    c = FORMS
    batch, params, raw, aug = raw_runs
    got = _serial(c['mt'], c['GB'], c['R'], c['steps'], c['lr'], batch, form='raw', staged=True)
    _same_bits(got, raw)
    assert got['losses'] == raw['losses'] and got['accs'] == raw['accs']
    got = _serial(c['mt'], c['GB'], c['R'], c['steps'], c['lr'], batch, form='aug', params=params, staged=True)
    _same_bits(got, aug)
    assert got['losses'] == aug['losses']


def test_augmented_global_batch_equals_the_per_slice_uploads(raw_runs):
    """R * B records: slice r is augmented by upload_batch_raw_aug's kernels with records [rB, (r + 1)B)."""
    c = FORMS
    batch, params, raw, aug = raw_runs
    em = _emulate(c['mt'], c['GB'], c['R'], c['steps'], c['lr'], batch, form='aug', params=params)
    _same_bits(aug, em)
    assert any(not np.array_equal(aug['params'][k], raw['params'][k]) for k in raw['params'])      # the records did something


# ---- bf16 engine -----------------------------------------------------------------------------------------------------------
def test_bf16_engine_two_replicas(gpu_required):
    """Mixed-precision engine, cnn_L3_melspec2, global batch 4 as 2 replicas.  The emulation runs twice: where the bf16 step
    reproduces its own bits the serial step must equal it bit for bit, else its losses stay within the oracle's 1e-3 of the
    emulation's.  Observed on the MI355X: see profiles/r25_serial_replicas.txt."""
    mt, GB, R, steps, lr = 'cnn_L3_melspec2', 4, 2, 2, 1e-3
    batch = _global_batch(GB, 'float')
    em1 = _emulate(mt, GB, R, steps, lr, batch, dtype='bf16')
    em2 = _emulate(mt, GB, R, steps, lr, batch, dtype='bf16')
    got = _serial(mt, GB, R, steps, lr, batch, dtype='bf16')
    same = all(np.array_equal(bits(em1['params'][k]), bits(em2['params'][k])) for k in em1['params']) and \
        np.array_equal(bits(em1['arena']), bits(em2['arena']))
    print('bf16 emulation reproduces its own bits: %s' % same)
    assert tuple(got['steps']) == (steps, R * steps)
    if same:
        _check_step(got, em1, R, steps)
    else:
        for g, w in zip(got['losses'], em1['losses']):
            print('bf16 serial loss %.6f, emulation %.6f' % (g, w))
            assert abs(g - w) < 1e-3 * max(1.0, abs(w)), (g, w)


# ---- model level -----------------------------------------------------------------------------------------------------------
def test_serial_model_trains_like_the_engine(gpu_required, tmp_path):
    """multi_gpu_model(..., 2, serial=True): train_on_batch of a float and of a raw batch of 4 equals the engine-level step in
    bits, test_on_batch is a one-replica model's within 1e-6, and the checkpoint is a 2-replica model's."""
    from l3embedding_amd import model
    from l3embedding_amd.training_utils import multi_gpu_model
    mt, GB, R, lr = 'tiny_L3', 4, 2, 1e-3
    m, _, _ = model.MODELS[mt]()
    m = multi_gpu_model(m, R, serial=True)
    assert m.replicas == R and m.serial
    m.compile(model.Adam(lr=lr), loss='categorical_crossentropy', metrics=['accuracy'])
    P0 = m._weights_dict()
    P0['dense_2/kernel'] = P0['dense_2/kernel'] * np.float32(1.0 / 64)
    m._assign(P0)
    e = _lib.Engine(mt, GB // R, global_batch=GB)
    e.set_params(P0)
    fv, fa, fl = _global_batch(GB, 'float')
    rv, ra, rl = _global_batch(GB, 'raw')
    got = m.train_on_batch([fv, fa], fl)
    e.replicas_upload(fv, fa, fl, R)
    e.step_replicas(lr)
    assert list(e.step_results()) == got
    got = m.train_on_batch([rv, ra], rl.astype(np.int64))
    e.replicas_upload_raw(rv, ra, rl, R)
    e.step_replicas(lr)
    assert list(e.step_results()) == got
    W, We = m._engine.get_params(), e.get_params()
    assert [k for k in We if not np.array_equal(bits(W[k]), bits(We[k]))] == []
    assert m._engine.optimizer_steps() == e.optimizer_steps() == (2, 2 * R)
    e.close()
    # test_on_batch: inference-mode BatchNorm does not depend on how the batch is cut
    m1, _, _ = model.MODELS[mt]()
    m1.compile(model.Adam(lr=lr), loss='categorical_crossentropy', metrics=['accuracy'])
    m1._assign(We)
    for x, y in (([fv, fa], fl), ([rv, ra], rl.astype(np.int64))):
        ev, ev1 = m.test_on_batch(x, y), m1.test_on_batch(x, y)
        print('test_on_batch: serial replicas %s, one replica %s' % (ev, ev1))
        assert abs(ev[0] - ev1[0]) <= 1e-6 * max(1.0, abs(ev1[0])) and abs(ev[1] - ev1[1]) <= 1e-6
    path = str(tmp_path / 'model_latest.h5')
    m.save_weights(path)
    m2 = model.load_model(path, mt, src_num_gpus=R)
    w, w2 = m.get_weights(), m2.get_weights()
    assert len(w) == len(w2) == 42 and all(np.array_equal(x, y) for x, y in zip(w, w2))


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _blobs(tmp_path):
    from l3embedding_amd import h5lite
    rng = np.random.RandomState(5)
    for split in ('tiny_train', 'tiny_valid'):
        d = tmp_path / 'data' / split
        d.mkdir(parents=True)
        for i in range(2):
            root = h5lite.Group()
            lab = rng.randint(0, 2, 6)
            root.create_dataset('audio', rng.randint(-32768, 32768, (6, 1, 48000)).astype(np.int16), compression='gzip')
            root.create_dataset('video', rng.randint(0, 256, (6, 224, 224, 3)).astype(np.uint8), compression='gzip')
            root.create_dataset('label', np.stack([lab, 1 - lab], 1).astype(np.int64), compression='gzip')
            h5lite.write_file(str(d / ('%d_%d_0.h5' % (20171021 + i, i))), root)
    return str(tmp_path / 'data' / 'tiny_train'), str(tmp_path / 'data' / 'tiny_valid')


def test_train_serial_replicas_end_to_end(gpu_required, tmp_path):
    """train_serial_replicas on the blobs of test_train_entry_point_and_resume: tiny_L3, gpus 2, global batch 4, two epochs of two
    steps, then one more epoch from continue_model_dir; then the same run augmented."""
    import pickle
    from l3embedding_amd import model, train as TR
    tr_dir, va_dir = _blobs(tmp_path)
    args = dict(train_epoch_size=2, validation_epoch_size=1, train_batch_size=4, validation_batch_size=4, model_type='tiny_L3',
                learning_rate=1e-3, checkpoint_interval=1, gpus=2)
    out = str(tmp_path / 'out')
    hist = TR.train_serial_replicas(tr_dir, va_dir, out, num_epochs=2, **args)
    assert all(len(hist.history[k]) == 2 for k in ('loss', 'acc', 'val_loss', 'val_acc'))
    root = os.path.join(out, 'embedding', 'tiny', 'tiny_L3')
    runs = os.listdir(root)
    assert len(runs) == 1
    md = os.path.join(root, runs[0])
    for f in ('config.json', 'model.json', 'model_spec.pkl', 'model_latest.h5', 'model_best_valid_accuracy.h5',
              'model_best_valid_loss.h5', 'model_checkpoint.01.h5', 'model_checkpoint.02.h5', 'history_csvlog.csv',
              'history_checkpoint.pkl', 'history.pkl'):
        assert os.path.exists(os.path.join(md, f)), f
    cfg = json.load(open(os.path.join(md, 'config.json')))
    assert cfg['serial_replicas'] is True and cfg['gpus'] == 2 and cfg['train_batch_size'] == 4 and 'augment' not in cfg
    m = model.load_model(os.path.join(md, 'model_latest.h5'), 'tiny_L3', src_num_gpus=2)       # an N-replica checkpoint
    assert len(m.get_weights()) == 42
    TR.train_serial_replicas(tr_dir, va_dir, out, num_epochs=3, continue_model_dir=md, **args)
    rows = open(os.path.join(md, 'history_csvlog.csv')).read().strip().split('\n')
    assert [r.split(',')[0] for r in rows] == ['epoch', '0', '1', '2']
    assert os.path.exists(os.path.join(md, 'model_checkpoint.03.h5'))
    assert len(pickle.load(open(os.path.join(md, 'history.pkl'), 'rb'))['loss']) == 1              # the resumed run's own epoch
    # the same run with every training batch augmented
    out_a = str(tmp_path / 'out_aug')
    hist_a = TR.train_serial_replicas(tr_dir, va_dir, out_a, augment=True, num_epochs=2, **args)
    root_a = os.path.join(out_a, 'embedding', 'tiny', 'tiny_L3')
    cfg_a = json.load(open(os.path.join(root_a, os.listdir(root_a)[0], 'config.json')))
    assert cfg_a['serial_replicas'] is True and cfg_a['augment'] is True and cfg_a['augment_random_state'] == 20180123
    assert len(hist_a.history['loss']) == 2 and hist_a.history['loss'] != hist.history['loss']


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_numbers(gpu_required):
    mt, B = 'tiny_L3', 2
    v, a, l = _global_batch(2 * B, 'float')
    e = _lib.Engine(mt, B, seed=SEED, global_batch=2 * B)
    with pytest.raises(_lib.L3Error, match=r'l3_step_replicas: no resident global batch .*batch 2, global_batch 4'):
        e.step_replicas(1e-3)
    with pytest.raises(_lib.L3Error, match=r'l3_eval_replicas: no resident global batch'):
        e.eval_replicas()
    with pytest.raises(_lib.L3Error, match=r'replicas = 0, must be >= 1'):
        e.replicas_upload(v[:0], a[:0], l[:0], 0)
    with pytest.raises(_lib.L3Error, match=r'3 replicas of batch 2 are 6 rows, the engine\'s global_batch is 4'):
        e.replicas_upload(np.concatenate([v, v[:2]]), np.concatenate([a, a[:2]]), np.concatenate([l, l[:2]]), 3)
    with pytest.raises(ValueError, match=r'3 rows for 2 replicas of batch 2 \(4 rows\)'):
        e.replicas_upload(v[:3], a[:3], l[:3], 2)
    e.replicas_upload(v, a, l, 2)
    e.step_replicas(1e-3)
    with pytest.raises(_lib.L3Error, match=r'probs / logits after a replicas step: .* 2 rows, not of the global batch of 4'):
        e.step_results(want_probs=True)
    loss, acc = e.step_results()
    assert np.isfinite(loss) and e.optimizer_steps() == (1, 2)
    e.close()
    e = _lib.Engine(mt, B, seed=SEED, global_batch=2 * B, dp_moving='rank_local')
    with pytest.raises(_lib.L3Error, match=r'L3_DP_MOVING_RANK_LOCAL \(1\) applies one moving-average update per step, 2 replicas apply 2'):
        e.replicas_upload(v, a, l, 2)
    e.close()


def test_an_engine_with_a_communicator_is_refused(gpu_required):
    """Its step is l3_step_dp; without the communicator the same engine takes the global batch."""
    mt, B = 'tiny_L3', 2
    v, a, l = _global_batch(B, 'float')
    e = _lib.Engine(mt, B, seed=SEED, global_batch=B)
    e.comm_init(_lib.comm_unique_id(), 1, 0)
    with pytest.raises(_lib.L3Error, match=r'l3_replicas_upload: the engine holds a communicator of 1 ranks; its step is l3_step_dp'):
        e.replicas_upload(v, a, l, 1)
    e.comm_destroy()
    e.replicas_upload(v, a, l, 1)
    e.step_replicas(1e-3)
    assert e.optimizer_steps() == (1, 1)
    e.close()
