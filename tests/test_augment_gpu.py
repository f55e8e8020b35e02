"""GPU tests of the training-set augmentation (csrc/augment.hip, l3embedding_amd/augment.py) against the float64 yardstick
of tests/augment_ref.py: the two operators, the engine paths that augment a batch in the pass that scales it, and the blob
rewriter.  The float64 references are computed once per module and shared."""
import random

import numpy as np
import pytest

from l3embedding_amd import _lib, augment, blobfeed, h5lite
from l3embedding_amd.model import MODELS, Adam

import augment_ref as R

pytestmark = pytest.mark.gpu

H, W = 230, 245                 # frames larger than the crop by (6, 21): no multiple of the kernel's 4-pixel groups, rows that
                                # start at every byte alignment
T = 48000


def video_case():
    """Six frames, one per image class and corner of the parameter space: starts 0 and the
    maxima (5, 20), both flips, both orders, factors {0.5, 1.0, 1.49}, deltas {-32/255, 0, +32/255}."""
    rs = np.random.RandomState(20180123)
    grey = rs.randint(0, 256, (H, W, 1))
    levels = np.array([0, 1, 127, 128, 254, 255])
    frames = np.stack([
        rs.randint(0, 256, (H, W, 3)),                                          # uniform random
        np.clip(grey + rs.randint(-6, 7, (H, W, 3)), 0, 255),                   # near grey: a grey +- 6 per channel
        np.repeat(grey, 3, -1),                                                 # exact greys
        levels[rs.randint(0, 6, (H, W, 3))],                                    # the ends and the middle of the range
        rs.randint(0, 256, (H, W, 3)),
        np.clip(grey[::-1] + rs.randint(-6, 7, (H, W, 3)), 0, 255),
    ]).astype(np.uint8)
    d = np.float32(32. / 255.)
    p = np.zeros(6, augment.PARAMS)
    p['start_x'] = [0, 5, 3, 5, 0, 2]
    p['start_y'] = [0, 20, 20, 0, 7, 13]
    p['flip'] = [0, 1, 0, 1, 1, 0]
    p['sat_first'] = [1, 0, 1, 0, 0, 1]
    p['saturation'] = np.float32([0.5, 1.49, 1.0, 1.49, 0.5, 1.49])
    p['brightness'] = [d, -d, 0, d, -d, 0]
    return frames, p


def audio_case():
    """Eight rows: two full-scale random, peak 100, silence, one holding -32768, one whose peak is +32767, a ramp, and a second
    quiet row; u covers both ends of [0, 1) and the middle."""
    rs = np.random.RandomState(7)
    rows = np.zeros((8, T), np.int16)
    rows[0] = rs.randint(-32768, 32768, T)
    rows[1] = rs.randint(-32767, 32768, T)
    rows[2] = rs.randint(-100, 101, T)
    rows[2, 17] = 100
    rows[4] = rs.randint(-20000, 20000, T)
    rows[4, 47999] = -32768
    rows[5] = rs.randint(-30000, 30000, T)
    rows[5, 0] = 32767
    rows[6] = np.linspace(-12000, 12000, T).astype(np.int16)
    rows[7] = rs.randint(-3, 4, T)
    top = 1.0 - 2.0 ** -53
    u = np.array([top, 0.5, top, 0.5, top, top, 0.0, 0.0])
    return rows, u


@pytest.fixture(scope='module')
def video():
    frames, p = video_case()
    want = R.augment_video(frames, p)
    want.setflags(write=False)
    got_u8, got_f32 = _lib.op_augment_video(frames, p, out='both')
    return frames, p, want, got_u8, got_f32


def test_video_operator_against_float64(video):
    """No value off by more than one level, and at most 1e-4 of the values off at all.  The cap is a condition, not a measurement.
    (An fp32 NumPy evaluation of saturation's closed form misses it on these frames -- 48 484 of 903 168 values, the rounding ties
    of factor 0.5 -- which is why the kernel follows the original's float64 operations instead: DESIGN.md 8e.)"""
    frames, p, want, got, _ = video
    assert got.shape == want.shape == (6, 224, 224, 3) and got.dtype == np.uint8
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    frac = float((diff != 0).mean())
    print('augment_video: max |diff| = %d level(s), %d of %d values differ (%.2e)' % (diff.max(), (diff != 0).sum(), diff.size, frac))
    assert diff.max() <= 1
    assert frac <= 1e-4


def test_video_identity_is_the_crop():
    frames, p = video_case()
    ident = augment.identity_params(len(frames))
    ident['start_x'], ident['start_y'] = p['start_x'], p['start_y']
    got = _lib.op_augment_video(frames, ident)
    for i in range(len(frames)):
        x0, y0 = int(p['start_x'][i]), int(p['start_y'][i])
        assert np.array_equal(got[i], frames[i, x0:x0 + 224, y0:y0 + 224])
    # ... and in the other order of the two colour operations
    ident['sat_first'] = 0
    assert np.array_equal(_lib.op_augment_video(frames, ident), got)


def test_video_float_form_is_preprocess_of_the_byte_form(video):
    _, _, _, got_u8, got_f32 = video
    scaled, _ = _lib.op_preprocess(video_u8=got_u8)
    assert got_f32.dtype == np.float32 and np.array_equal(got_f32.view(np.uint32), scaled.view(np.uint32))


def test_video_operator_rejects_a_crop_outside_the_frame():
    frames, p = video_case()
    p['start_y'][3] = 22
    with pytest.raises(_lib.L3Error, match='record 3'):
        _lib.op_augment_video(frames, p)


def test_audio_operator_bit_exact_against_float64():
    rows, u = audio_case()
    want, want_gains = R.augment_audio(rows, u)
    (got, got_f32), gains = _lib.op_augment_audio(rows, u, out='both')
    assert np.array_equal(gains.view(np.uint64), want_gains.view(np.uint64)), (gains, want_gains)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    _, scaled = _lib.op_preprocess(audio_i16=got)
    assert np.array_equal(got_f32.view(np.uint32), scaled.view(np.uint32))
    assert 0.9 <= gains.min() and gains.max() <= 1.1                               # sample.py:157
    # a row length that is no multiple of the 8-sample vectors takes the kernel's scalar path
    odd = rows[:, :4001]
    want, want_gains = R.augment_audio(odd, u)
    got, gains = _lib.op_augment_audio(odd, u)
    assert np.array_equal(gains.view(np.uint64), want_gains.view(np.uint64)) and np.array_equal(got, want)


# ---- engine paths -------------------------------------------------------------------------------------------------------
B = 4


def _raw_batches(n):
    rs = np.random.RandomState(99)
    out = []
    for _ in range(n):
        v = rs.randint(0, 256, (B, 224, 224, 3)).astype(np.uint8)
        a = (rs.randn(B, 1, T) * 6000).clip(-32768, 32767).astype(np.int16)
        lab = rs.randint(0, 2, B)
        out.append(([v, a], np.stack([lab, 1 - lab], 1).astype(np.int64)))
    return out


def _model():
    m, _, _ = MODELS['tiny_L3'](num_gpus=1)
    m.compile(Adam(lr=1e-3), loss='categorical_crossentropy', metrics=['accuracy'])
    return m


class _Record(object):
    """Callback that keeps every step's (loss, acc); declares its batch hooks passive so that fit_generator stages batches."""
    batch_hooks_are_passive = True

    def __init__(self):
        self.steps = []

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    on_train_end = on_epoch_begin = on_epoch_end = on_batch_begin = lambda self, *a, **k: None

    def on_batch_end(self, step, logs=None):
        self.steps.append((logs['loss'], logs['acc']))


def test_engine_augments_as_the_operator_does():
    """train_on_batch on inputs that carry .augment == train_on_batch on the raw batch augment_batch made of them, bit for bit;
    the loss is not the un-augmented batch's; l3_batch_gains returns the operator's gains."""
    (x, y), = _raw_batches(1)
    params = augment.draw_params(random.Random(5), B)
    done = augment.augment_batch(x[0], x[1], params)
    got = _model().train_on_batch(augment.AugmentedInputs(x, params), y)
    want = _model().train_on_batch([done['video'], done['audio']], y)
    plain = _model().train_on_batch(x, y)
    assert got == want
    assert got[0] != plain[0]
    m = _model()
    m.train_on_batch(augment.AugmentedInputs(x, params), y)
    assert np.array_equal(m._engine.batch_gains(), done['audio_gain'])
    m.train_on_batch(x, y)
    with pytest.raises(_lib.L3Error, match='not augmented'):
        m._engine.batch_gains()
    with pytest.raises(ValueError, match='raw batches'):
        m.train_on_batch(augment.AugmentedInputs([x[0].astype(np.float32), x[1].astype(np.float32)], params), y)


def test_staged_augmented_steps_match_unstaged_ones():
    """Three fit_generator steps over AugmentingFeed (batches 2 and 3 go through l3_stage_batch_raw_aug and adopt_staged) ==
    the same three augmented batches through train_on_batch."""
    batches = _raw_batches(3)
    rec = _Record()
    _model().fit_generator(augment.AugmentingFeed(iter(batches), 11), 3, 1, verbose=0, callbacks=[rec], max_queue_size=0)
    rng, m, want = random.Random(11), _model(), []
    for x, y in batches:
        want.append(tuple(m.train_on_batch(augment.AugmentedInputs(x, augment.draw_params(rng, B)), y)))
    assert rec.steps == want


def test_plain_staged_batch_after_an_augmented_one():
    """augmented, plain, augmented through the staged path == the same sequence unstaged: nothing of a staged augmentation
    outlives its batch, in either direction."""
    batches = _raw_batches(3)
    params = [augment.draw_params(random.Random(s), B) for s in (1, 2)]
    mixed = [(augment.AugmentedInputs(batches[0][0], params[0]), batches[0][1]), batches[1],
             (augment.AugmentedInputs(batches[2][0], params[1]), batches[2][1])]
    rec = _Record()
    _model().fit_generator(iter(mixed), 3, 1, verbose=0, callbacks=[rec], max_queue_size=0)
    m = _model()
    want = [tuple(m.train_on_batch(x, y)) for x, y in mixed]
    assert rec.steps == want
    # the middle step is the one a model sees that was never given an augmented batch
    m2 = _model()
    done = augment.augment_batch(batches[0][0][0], batches[0][0][1], params[0])
    first = tuple(m2.train_on_batch([done['video'], done['audio']], batches[0][1]))
    second = tuple(m2.train_on_batch(*batches[1]))
    assert rec.steps[:2] == [first, second]


def test_rewrite_one_blob(tmp_path):
    (x, y), = _raw_batches(1)
    src, dst = tmp_path / 'src', tmp_path / 'dst'
    src.mkdir()
    root = h5lite.Group()
    root.create_dataset('audio', x[1], compression='gzip')
    root.create_dataset('video', x[0], compression='gzip')
    root.create_dataset('label', y)
    root.create_dataset('audio_start_sample_idx', np.arange(B))
    h5lite.write_file(str(src / 'blob_0.h5'), root)
    assert augment.rewrite(str(src), str(dst), random_state=3) == ['blob_0.h5']
    want = augment.augment_batch(x[0], x[1], augment.draw_params(random.Random(3), B))
    with h5lite.File(str(dst / 'blob_0.h5')) as f:
        got = {k: node.read() for k, node in f.root.children.items()}
    assert set(got) == {'audio', 'video', 'label', 'audio_start_sample_idx'} | set(augment.METADATA_KEYS)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got['label'], y) and not np.array_equal(got['video'], x[0])
    feed = blobfeed.BlobFeed(str(dst), B)           # the metadata datasets do not reach a batch (train.py:149-151)
    batch = next(feed)
    feed.close()
    assert sorted(batch) == ['audio', 'label', 'video']
    assert np.array_equal(batch['video'], want['video']) and np.array_equal(batch['audio'], want['audio'])
