"""GPU tests of the sampled batches (csrc/avsample.hip, the sampled fill of csrc/batch_feed.hip, l3embedding_amd/avsample.py):
the mono mix, the operator against the NumPy oracle of tests/avsample_ref.py, against the reference's own outputs
(tests/golden/ref_avsample.npz) and against tests/image_ref.py, the engine paths against the raw-batch paths they must equal bit
for bit, the refusals, fit_generator over a ClipSampler and the blob writer.  Banks and references are made once per module."""
import os
import random

import numpy as np
import pytest

from l3embedding_amd import _lib, augment, avsample, h5lite, train
from l3embedding_amd.model import MODELS, Adam

import augment_ref
import avsample_ref as A
import image_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
T = A.T
B = 4           # the engine tests of tests/test_augment_gpu.py: tiny_L3, batches of 4


@pytest.fixture(scope='module')
def ref():
    with np.load(os.path.join(GOLDEN, 'ref_avsample.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def bank():
    """The fixture's three clips as their sampler saw them (no resize)."""
    clips = A.fixture_clips()
    b = avsample.ClipBank(0, sum(f.size for f, _ in clips), sum(len(a) + 8 for _, a in clips), resize=None)
    for (f, a), name in zip(clips, A.FIXTURE_NAMES):
        b.add(f, a, 48000, name=os.path.basename(name))
    yield b
    b.close()


RESIZE_SHAPES = [(3, 120, 160), (2, 360, 480)]          # an upscale to 256 x 342; a shrink by 1.4


@pytest.fixture(scope='module')
def resize_clips():
    out = []
    for i, (t, h, w) in enumerate(RESIZE_SHAPES):
        rs = np.random.RandomState(40 + i)
        out.append((rs.randint(0, 256, (t, h, w, 3)).astype(np.uint8), rs.randint(-32768, 32768, (60001 + 11 * i, 2 + i)).astype(np.int16)))
    return out


@pytest.fixture(scope='module')
def resize_bank(resize_clips):
    b = avsample.ClipBank(0, sum(f.size for f, _ in resize_clips), sum(len(a) + 8 for _, a in resize_clips), resize=256)
    for f, a in resize_clips:
        b.add(f, a, 48000)
    yield b
    b.close()


def drawn(ref, prefix, aug, bank):
    rows = [avsample.draw_samples(random.Random(int(s)), int(p[0]), int(p[1]), 1, aug, bank.clips)[0]
            for s, p in zip(ref[prefix + '_seed'], ref[prefix + '_pair'])]
    return np.array(rows, avsample.SAMPLE)


def record(video_clip, frame, audio_clip, audio_start, start_x, start_y, label=0):
    r = np.zeros(1, avsample.SAMPLE)
    r['video_clip'], r['frame'], r['audio_clip'], r['audio_start'] = video_clip, frame, audio_clip, audio_start
    r['start_x'], r['start_y'], r['label'], r['sat_first'], r['saturation'] = start_x, start_y, label, 1, 1.0
    return r[0]


# ---- the mono mix -------------------------------------------------------------------------------------------------------
EDGES = [(-3, -4), (-1, 0), (3, 4), (1, 0), (32767, 32767), (32767, 32766), (-32768, -32768), (-32768, -32767), (-32768, 32767)]


@pytest.mark.parametrize('channels', [1, 2, 3, 8])
def test_downmix_equals_numpy(channels):
    """l3_clipbank_audio == audio.mean(axis=-1).astype('int16') (sample.py:445-448) exactly: lengths 1, 7 (the element-wise tail
    alone) and 60 001 (235 workgroups and a tail of one), sums that are odd, negative and at both ends of the range."""
    rs = np.random.RandomState(channels)
    cases = []
    for n in (1, 7, 60001):
        x = rs.randint(-32768, 32768, (n, channels)).astype(np.int16)
        if n > len(EDGES):
            for i, (a, b) in enumerate(EDGES):
                x[i] = ([a, b] * channels)[:channels]
            x[len(EDGES)] = -32768
            x[len(EDGES) + 1] = 32767
            x[len(EDGES) + 2] = [-1] * (channels - 1) + [0]
        cases.append(x)
    b = avsample.ClipBank(0, 64, sum(len(x) + 8 for x in cases), resize=256)
    try:
        for x in cases:
            cid = b.add(np.zeros((1, 1, 1, 3), np.uint8), x, 48000)
            want = x.mean(axis=-1).astype('int16')
            got = b.audio(cid)
            assert got.dtype == np.int16 and np.array_equal(got, want), (channels, len(x), np.nonzero(got != want)[0][:5])
            assert np.array_equal(want, A.downmix(x))
        assert A.downmix(np.array([EDGES[0], EDGES[1]], np.int16)).tolist() == [-3, 0]
    finally:
        b.close()


# ---- the operator -------------------------------------------------------------------------------------------------------
def test_operator_equals_the_oracle_and_the_reference(ref, bank):
    """Un-augmented, no resize: bytes and samples == tests/avsample_ref.py == the reference's generate_sample, exactly."""
    rec = drawn(ref, 'plain', False, bank)
    video, audio, gains = _lib.op_sample_batch(bank, rec, False)
    want_v, want_a = A.cut(A.fixture_clips(), rec)
    assert gains is None and video.dtype == np.uint8 and audio.dtype == np.int16
    assert np.array_equal(video, want_v) and np.array_equal(audio, want_a)
    assert np.array_equal(video, ref['plain_video']) and np.array_equal(audio, ref['plain_audio'][:, 0])


def test_operator_at_the_ends_of_every_range(bank):
    """Crops at (0, 0) and at the far corner, first and last frame, the last start a clip allows (every alignment of the source
    offset modulo the 8-sample vectors), a clip shorter than a second and one of exactly a second."""
    clips = A.fixture_clips()
    rec = [record(0, 0, 0, 0, 0, 0), record(0, 39, 0, 72000 - T, 232 - 224, 240 - 224), record(1, 6, 1, 0, 256 - 224, 300 - 224),
           record(2, 29, 2, 0, 230 - 224, 0), record(1, 0, 0, 23999, 0, 300 - 224)]
    rec += [record(2, 3, 0, 1000 + k, k % 7, 1) for k in range(1, 8)]
    rec = np.array(rec, avsample.SAMPLE)
    video, audio, _ = _lib.op_sample_batch(bank, rec, False)
    want_v, want_a = A.cut(clips, rec)
    assert np.array_equal(video, want_v) and np.array_equal(audio, want_a)
    assert not audio[2, 30000:].any() and audio[2, :30000].any()
    # what the bank holds of a mono clip is the clip
    for i, (_, a) in enumerate(clips):
        assert np.array_equal(bank.audio(i), a)


def test_operator_resizes_as_image_frames_does(resize_bank, resize_clips):
    """resize=256 on 120 x 160 clips (an upscale to 256 x 342) and 360 x 480 clips: the window of csrc/frames.hip's resize, equal
    to tests/image_ref.py exactly; crops at (0, 0), at the far corner and in between; the audio is the mono mix's."""
    infos = resize_bank.clips
    assert [tuple(c[1:5]) for c in infos] == [(120, 160, 256, 342), (360, 480, 256, 342)]
    rec = np.array([record(0, 0, 0, 0, 0, 0), record(0, 2, 1, 12000, 32, 118), record(0, 1, 0, 5, 13, 57),
                    record(1, 0, 1, 12012, 0, 0), record(1, 1, 0, 12001, 32, 118), record(1, 1, 1, 77, 31, 1)], avsample.SAMPLE)
    video, audio, _ = _lib.op_sample_batch(resize_bank, rec, False)
    for i, r in enumerate(rec):
        c = infos[int(r['video_clip'])]
        frame = resize_clips[int(r['video_clip'])][0][int(r['frame'])]
        want, _ = image_ref.frame_ref(frame, [0, c.height, c.width, c.out_height, c.out_width, int(r['start_x']), int(r['start_y'])])
        assert np.array_equal(video[i], want), i
        mono = A.downmix(resize_clips[int(r['audio_clip'])][1])
        assert np.array_equal(audio[i], A.one_second(mono, int(r['audio_start']))), i


def test_operator_augmented(ref, bank):
    """Audio rows and gains == the oracle == the reference, bit for bit.  Frames == op_augment_video(op_image_frames(...)) of the
    existing operators bit for bit, and within the existing condition of test_video_operator_against_float64 of the float64
    oracle: no value off by more than one level, at most 1e-4 of the values off at all."""
    clips = A.fixture_clips()
    rec = drawn(ref, 'aug', True, bank)
    video, audio, gains = _lib.op_sample_batch(bank, rec, True)
    crops, seconds = A.cut(clips, rec)
    want_a, want_g = augment_ref.augment_audio(seconds, rec['u_gain'])
    assert np.array_equal(gains.view(np.uint64), want_g.view(np.uint64)) and np.array_equal(audio, want_a)
    assert np.array_equal(audio, ref['aug_audio'][:, 0]) and np.array_equal(gains, ref['aug_audio_gain'])
    # the existing operators on the same frames
    frames = [clips[int(r['video_clip'])][0][int(r['frame'])] for r in rec]
    pixels = np.concatenate([f.reshape(-1) for f in frames])
    table = np.array([[0, f.shape[0], f.shape[1], f.shape[0], f.shape[1], r['start_x'], r['start_y']] for f, r in zip(frames, rec)],
                     np.int64)
    sizes = np.array([f.size for f in frames], np.int64)
    table[:, 0] = np.cumsum(sizes) - sizes
    u8, _ = _lib.op_image_frames(pixels, table, want_f32=False)
    assert np.array_equal(u8, crops)
    zero_crop = rec.copy()
    zero_crop['start_x'] = zero_crop['start_y'] = 0
    assert np.array_equal(video, _lib.op_augment_video(u8, zero_crop))
    want_v = augment_ref.augment_video(crops, zero_crop)
    diff = np.abs(video.astype(np.int32) - want_v.astype(np.int32))
    frac = float((diff != 0).mean())
    print('sampled augment_video: max |diff| = %d level(s), %d of %d values differ (%.2e)' % (diff.max(), (diff != 0).sum(), diff.size, frac))
    assert diff.max() <= 1
    assert frac <= 1e-4
    assert rec['flip'].any() and not rec['flip'].all()


# ---- engine paths -------------------------------------------------------------------------------------------------------
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


def _batches(bank, n, aug, seed=3):
    s = avsample.ClipSampler(bank, batch_size=B, random_state=seed, k=2, rate=3, augment=aug)
    return [next(s) for _ in range(n)]


def _as_raw(x):
    """The raw batch a sampled one must equal: the operator's un-augmented outputs, and for an augmented batch its records with
    the crop taken out."""
    v, a, _ = _lib.op_sample_batch(x.bank, x.sample_records, False)
    arrays = [v, a.reshape(len(a), 1, T)]
    if not x.augmented:
        return arrays
    rows = np.zeros(len(v), augment.PARAMS)
    for name in augment.PARAMS.names:
        rows[name] = x.sample_records[name]
    rows['start_x'] = rows['start_y'] = 0
    return augment.AugmentedInputs(arrays, rows)


def _same_weights(m1, m2):
    p1, p2 = m1._engine.get_params(), m2._engine.get_params()
    return list(p1) == list(p2) and all(np.array_equal(p1[k].view(np.uint32), p2[k].view(np.uint32)) for k in p1)


@pytest.mark.parametrize('aug', [False, True])
def test_engine_sampled_equals_raw(bank, aug):
    """upload_batch_sampled == upload_batch_raw[_aug] of the operator's outputs with zero crop offsets: loss, accuracy,
    batch_gains and every weight after the step, bit for bit."""
    (x, y), = _batches(bank, 1, aug)
    m1, m2 = _model(), _model()
    got = m1.train_on_batch(x, y)
    want = m2.train_on_batch(_as_raw(x), y)
    assert got == want
    assert _same_weights(m1, m2)
    if aug:
        g = m1._engine.batch_gains()
        assert np.array_equal(g.view(np.uint64), m2._engine.batch_gains().view(np.uint64))
        assert np.array_equal(g, _lib.op_sample_batch(bank, x.sample_records, True)[2])
    else:
        with pytest.raises(_lib.L3Error, match='not augmented'):
            m1._engine.batch_gains()


def test_engine_sampled_through_the_resize(resize_bank):
    (x, y), = _batches(resize_bank, 1, True, seed=9)
    m1, m2 = _model(), _model()
    assert m1.train_on_batch(x, y) == m2.train_on_batch(_as_raw(x), y)
    assert _same_weights(m1, m2)


@pytest.mark.parametrize('aug', [False, True])
def test_staged_sampled_steps_match_unstaged_ones(bank, aug):
    """Three fit_generator steps (batches 2 and 3 go through l3_stage_batch_sampled and are adopted) == the same three batches
    through train_on_batch == their raw equivalents."""
    batches = _batches(bank, 3, aug)
    rec = _Record()
    m0 = _model()
    m0.fit_generator(iter(batches), 3, 1, verbose=0, callbacks=[rec], max_queue_size=0)
    m1, m2 = _model(), _model()
    want = [tuple(m1.train_on_batch(x, y)) for x, y in batches]
    raw = [tuple(m2.train_on_batch(_as_raw(x), y)) for x, y in batches]
    assert rec.steps == want == raw
    assert _same_weights(m0, m1) and _same_weights(m1, m2)


def test_plain_and_sampled_staged_batches_follow_each_other(bank):
    """sampled (augmented), blob, sampled, blob through the staged path == the same sequence unstaged == the sequence with every
    sampled batch replaced by its raw equivalent: nothing of a sampled fill outlives its batch, in either direction."""
    s = _batches(bank, 2, True, seed=4)
    rs = np.random.RandomState(99)
    blobs = []
    for _ in range(2):
        lab = rs.randint(0, 2, B)
        blobs.append(([rs.randint(0, 256, (B, 224, 224, 3)).astype(np.uint8),
                       (rs.randn(B, 1, T) * 6000).clip(-32768, 32767).astype(np.int16)], np.stack([lab, 1 - lab], 1).astype(np.int64)))
    mixed = [s[0], blobs[0], s[1], blobs[1]]
    rec = _Record()
    _model().fit_generator(iter(mixed), 4, 1, verbose=0, callbacks=[rec], max_queue_size=0)
    m1, m2 = _model(), _model()
    want = [tuple(m1.train_on_batch(x, y)) for x, y in mixed]
    alone = [tuple(m2.train_on_batch(x if isinstance(x, list) else _as_raw(x), y)) for x, y in mixed]
    assert rec.steps == want == alone
    # ... and starting with a blob
    rec = _Record()
    _model().fit_generator(iter(mixed[1:]), 3, 1, verbose=0, callbacks=[rec], max_queue_size=0)
    m3 = _model()
    assert rec.steps == [tuple(m3.train_on_batch(x if isinstance(x, list) else _as_raw(x), y)) for x, y in mixed[1:]]


def test_refusals_name_the_sample_and_launch_nothing(bank):
    (x, y), = _batches(bank, 1, False)
    m = _model()
    m.train_on_batch(x, y)
    e = m._engine
    e.step_forward(training=False)
    before = e.step_results()
    good = x.sample_records

    def refused(field, value, row, match, fn=e.upload_batch_sampled):
        bad = good.copy()
        bad[field][row] = value
        with pytest.raises(_lib.L3Error, match=match) as err:
            fn(bank, bad, False)
        assert 'error -1' in str(err.value) and 'sample %d' % row in str(err.value)

    refused('video_clip', 3, 1, 'video_clip 3')
    refused('audio_clip', -1, 2, 'audio_clip -1')
    refused('frame', bank.clips[int(good['video_clip'][3])].frames, 3, 'frame')
    refused('frame', -1, 0, 'frame')
    last = max(bank.clips[int(good['audio_clip'][0])].samples - T, 0)
    refused('audio_start', last + 1, 0, 'audio_start')
    refused('audio_start', -1, 1, 'audio_start')
    refused('start_x', bank.clips[int(good['video_clip'][2])].out_height - 224 + 1, 2, 'crop')
    refused('start_y', -1, 3, 'crop')
    refused('label', 2, 1, 'label')
    refused('frame', -1, 2, 'frame', fn=e.stage_batch_sampled)
    with pytest.raises(_lib.L3Error, match='sample 1'):
        bad = good.copy()
        bad['frame'][1] = 1000
        _lib.op_sample_batch(bank, bad, False)
    with pytest.raises(_lib.L3Error, match='3 sample records for a batch of 4'):
        e.upload_batch_sampled(bank, good[:3], False)
    if _lib.load().l3_device_count() > 1:
        other = avsample.ClipBank(1, 1 << 20, 1 << 16, resize=256)
        with pytest.raises(_lib.L3Error, match='device'):
            e.upload_batch_sampled(other, good, False)
        other.close()
    # nothing was launched and nothing staged: the resident batch is the one the step trained on
    e.step_forward(training=False)
    assert e.step_results() == before
    # a full bank
    frame = 3 * 230 * 230
    small = avsample.ClipBank(0, 3 * frame, 50000, resize=None)
    try:
        small.add(np.zeros((2, 230, 230, 3), np.uint8), np.zeros(40000, np.int16), 48000)
        with pytest.raises(_lib.L3Error, match='error -3.*full') as err:          # the pixels
            small.add(np.zeros((2, 230, 230, 3), np.uint8), np.zeros(100, np.int16), 48000)
        assert str(2 * frame) in str(err.value) and str(3 * frame) in str(err.value)
        with pytest.raises(_lib.L3Error, match='error -3.*full') as err:          # the samples
            small.add(np.zeros((1, 230, 230, 3), np.uint8), np.zeros(20000, np.int16), 48000)
        assert '20000' in str(err.value) and '50000' in str(err.value)
        assert len(small.clips) == 1 and small.usage() == (2 * frame, 3 * frame, 40000, 50000)
        assert small.add(np.zeros((1, 230, 230, 3), np.uint8), np.zeros(10000, np.int16), 48000) == 1
    finally:
        small.close()


def test_fit_generator_over_a_clip_sampler(bank):
    """2 epochs x 3 steps from a ClipSampler == the same records through train_on_batch, bit for bit."""
    kw = dict(batch_size=B, random_state=21, k=2, rate=5, augment=True)
    rec = _Record()
    hist = _model().fit_generator(avsample.ClipSampler(bank, **kw), 3, 2, verbose=0, callbacks=[rec])
    s, m = avsample.ClipSampler(bank, **kw), _model()
    want = [tuple(m.train_on_batch(*next(s))) for _ in range(6)]
    assert rec.steps == want
    epochs = []
    for steps in (want[:3], want[3:]):
        total = 0.0
        for loss, _ in steps:
            total += loss * B
        epochs.append(total / (3 * B))
    assert hist.history['loss'] == epochs


def test_write_blobs(bank, tmp_path):
    """One blob read back by train.data_generator == sample_batch of its records; the datasets the feed delivers have the dtypes
    of tests/golden/ref_blobs, and the metadata travels under generate_sample's keys.  (audio_start_sample_idx is the float
    generate_sample returns, sample.py:166,382; ref_blobs holds an integer stand-in under that name.)"""
    kw = dict(batch_size=B, random_state=8, k=2, rate=3, augment=True)
    paths = avsample.write_blobs(avsample.ClipSampler(bank, **kw), 1, str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ['8_0_0.h5']
    x, y = next(avsample.ClipSampler(bank, **kw))
    want = avsample.sample_batch(bank, x.sample_records, True)
    feed = train.data_generator(str(tmp_path), batch_size=B)
    batch = next(feed)
    feed.close()
    assert sorted(batch) == ['audio', 'label', 'video']
    for k in batch:
        assert np.array_equal(batch[k], want[k]), k
    assert np.array_equal(want['label'], y)
    with h5lite.File(paths[0]) as f:
        got = {k: node.read() for k, node in f.root.children.items()}
    with h5lite.File(os.path.join(GOLDEN, 'ref_blobs', 'blob_0.h5')) as f:
        golden = {k: node.read() for k, node in f.root.children.items()}
    assert set(golden) <= set(got)
    for k in ('audio', 'video', 'label'):
        assert got[k].dtype == golden[k].dtype and got[k].ndim == golden[k].ndim, k
    assert set(got) == {'audio', 'video', 'label', 'audio_file', 'video_file', 'audio_start_sample_idx',
                        'video_start_frame_idx'} | set(augment.METADATA_KEYS)
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    assert got['audio_start_sample_idx'].dtype == np.float64 and got['audio_file'].dtype.kind == 'S'
    assert np.array_equal(got['video_bounding_box_start_x'], x.sample_records['start_x'])
