"""The transitions between the ways a batch in the stored dtypes reaches the engine: uploaded or staged, as a single batch or as a
resident global batch of serial replicas, plain or augmented.  tiny_L3, batch 2, three steps at lr 1e-3 (five where a staged set is
refilled), a fresh random raw batch per step; every comparison is on the bits of every parameter and of the gradient arena."""
import numpy as np
import pytest

from dp_native_worker import DATA_SEED, SEED, live_head
from l3embedding_amd import _lib
from test_serial_replicas_gpu import _arena, _aug_params, _global_batch, _same_bits, bits

pytestmark = pytest.mark.gpu
MT, B, LR, STEPS = 'tiny_L3', 2, 1e-3, 3


def _batches(rows, n, first=0):
    return [_global_batch(rows, 'raw', seed=DATA_SEED + first + k) for k in range(n)]


def _engine(R=1):
    e = _lib.Engine(MT, B, seed=SEED, global_batch=R * B)
    live_head(e)
    return e


def _state(e):
    out = dict(params=e.get_params(), arena=_arena(e), steps=e.optimizer_steps())
    e.close()
    return out


def _uploaded(batches, R=1):
    """The reference of every case: each step's batch uploaded, then the step."""
    e = _engine(R)
    for v, a, l in batches:
        if R > 1:
            e.replicas_upload_raw(v, a, l, R)
            e.step_replicas(LR)
        else:
            e.upload_batch_raw(v, a, l)
            e.step_resident(LR)
    return _state(e)


def test_upload_supersedes_a_staged_single_batch(gpu_required):
    X, Y = _batches(B, STEPS, first=100), _batches(B, STEPS)
    e = _engine()
    for x, y in zip(X, Y):
        e.stage_batch_raw(*x)
        e.upload_batch_raw(*y)
        e.step_resident(LR)
    _same_bits(_state(e), _uploaded(Y))


def test_upload_supersedes_a_staged_global_batch(gpu_required):
    R = 2
    X, Y = _batches(R * B, STEPS, first=100), _batches(R * B, STEPS)
    e = _engine(R)
    for x, y in zip(X, Y):
        e.replicas_stage_raw(*x, R)
        e.replicas_upload_raw(*y, R)
        e.step_replicas(LR)
    _same_bits(_state(e), _uploaded(Y, R))


def test_partial_upload_leaves_the_other_inputs(gpu_required):
    """upload_batch_raw(video_u8=V2) after a full upload of (V1, A1, L1) is a full upload of (V2, A1, L1)."""
    first, second = _batches(B, STEPS), _batches(B, STEPS, first=100)
    e = _engine()
    for (v1, a1, l1), (v2, _, _) in zip(first, second):
        e.upload_batch_raw(v1, a1, l1)
        e.upload_batch_raw(video_u8=v2)
        e.step_resident(LR)
    _same_bits(_state(e), _uploaded([(s[0], f[1], f[2]) for f, s in zip(first, second)]))


def test_batch_gains_follow_the_adopted_batch(gpu_required):
    """The gains of a batch staged with its records, read after the step that adopted it; of the last slice of an augmented global
    batch; none after a plain adoption."""
    (v, a, l), = _batches(B, 1)
    p = _aug_params(B)
    _, want = _lib.op_augment_audio(a.reshape(B, -1), p['u_gain'])
    e = _engine()
    e.stage_batch_raw_aug(v, a, l, p, p['u_gain'])
    e.step_resident(LR)
    assert np.array_equal(e.batch_gains(), want)
    e.stage_batch_raw(v, a, l)
    e.step_resident(LR)
    with pytest.raises(_lib.L3Error, match='not augmented'):
        e.batch_gains()
    e.close()
    R = 2
    (v, a, l), = _batches(R * B, 1)
    p = _aug_params(R * B)
    _, want = _lib.op_augment_audio(a.reshape(R * B, -1), p['u_gain'])
    e = _engine(R)
    e.replicas_upload_raw_aug(v, a, l, p, p['u_gain'], R)
    e.step_replicas(LR)
    assert np.array_equal(e.batch_gains(), want[(R - 1) * B:])
    e.replicas_stage_raw(v, a, l, R)
    e.step_replicas(LR)
    with pytest.raises(_lib.L3Error, match='not augmented'):
        e.batch_gains()
    e.close()


def test_global_and_single_batches_on_one_engine(gpu_required):
    """global_batch == batch: a one-replica global batch, then a single batch, is two single batches; a single batch staged in front
    of step_replicas does not displace the resident global batch."""
    X, Y, Z = _batches(B, 3)
    e = _engine()
    e.replicas_upload_raw(*X, 1)
    e.step_replicas(LR)
    e.upload_batch_raw(*Y)
    e.step_resident(LR)
    _same_bits(_state(e), _uploaded([X, Y]))
    e = _engine()
    e.replicas_upload_raw(*X, 1)
    for _ in range(STEPS):
        e.stage_batch_raw(*Z)
        e.step_replicas(LR)
    got = _state(e)
    want = _uploaded([X] * STEPS)
    _same_bits(got, want)
    assert got['steps'] == want['steps'] == (STEPS, STEPS)


def test_tower_step_adopts_a_staged_batch(gpu_required):
    X, Z = _batches(B, 2)
    e = _engine()
    e.upload_batch_raw(*X)
    e.stage_batch_raw(*Z)
    e.tower_step('vision', backward=False)
    got = e.activation('vision_model/input')
    e.close()
    want, _ = _lib.op_preprocess(video_u8=Z[0])
    assert np.array_equal(bits(got), bits(want.ravel()))
    assert not np.array_equal(got, _lib.op_preprocess(video_u8=X[0])[0].ravel())


@pytest.mark.parametrize('R', [1, 2])
def test_a_staged_set_is_refilled_behind_every_step(gpu_required, R):
    """Five steps with the next batch staged behind each: the third and later fills reuse a set that a queued step may still read.
    Each step's results are read one step late, so the host does not serialise the streams."""
    steps = 5
    batches = _batches(R * B, steps)
    e = _engine(R)
    if R > 1:
        send = lambda stage, b: (e.replicas_stage_raw if stage else e.replicas_upload_raw)(*b, R)
        step = e.step_replicas
    else:
        send = lambda stage, b: (e.stage_batch_raw if stage else e.upload_batch_raw)(*b)
        step = e.step_resident
    send(False, batches[0])
    losses = []
    for k in range(steps):
        step(LR)
        e.results_enqueue(k & 1)
        if k + 1 < steps:
            send(True, batches[k + 1])
        if k > 0:
            losses.append(e.results_wait((k - 1) & 1)[0])
    losses.append(e.results_wait((steps - 1) & 1)[0])
    assert len(losses) == steps and all(np.isfinite(losses))
    got = _state(e)
    want = _uploaded(batches, R)
    _same_bits(got, want)
    assert got['steps'] == want['steps'] == (steps, R * steps)
