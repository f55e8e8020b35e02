"""Host tests of l3embedding_amd/avsample.py: the sampling rule against samples computed by the reference's own generate_sample
(tests/golden/ref_avsample.npz, made by tests/golden/make_avsample_fixture.py), the NumPy oracle of tests/avsample_ref.py against
the same, pair formation, the multiplexer's stated rule and the refusals.  No GPU."""
import os
import random

import numpy as np
import pytest

from l3embedding_amd import _lib, avsample
from l3embedding_amd.model import MODELS, Adam

import augment_ref
import avsample_ref as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_avsample.npz')
NAMES = [os.path.basename(n).encode() for n in A.FIXTURE_NAMES]


@pytest.fixture(scope='module')
def ref():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_infos():
    return [avsample.clip_info(nf, h, w, ns, resize=None, name=name)
            for (_, nf, h, w, ns, _), name in zip(A.FIXTURE_CLIPS, A.FIXTURE_NAMES)]


def fixture_records(ref, prefix, augment):
    infos = fixture_infos()
    rows = [avsample.draw_samples(random.Random(int(s)), int(p[0]), int(p[1]), 1, augment, infos)[0]
            for s, p in zip(ref[prefix + '_seed'], ref[prefix + '_pair'])]
    return np.array(rows, avsample.SAMPLE)


def test_fixture_holds_the_cases_the_rule_has(ref):
    assert len(ref['plain_seed']) >= 12 and len(ref['aug_seed']) >= 24
    assert ref['plain_video'].shape[1:] == (224, 224, 3) and ref['plain_audio'].shape[1:] == (1, A.T)
    for prefix in ('plain', 'aug'):
        clip_a = np.array([NAMES.index(n) for n in ref[prefix + '_audio_file']])
        clip_v = np.array([NAMES.index(n) for n in ref[prefix + '_video_file']])
        start = np.rint(ref[prefix + '_audio_start_sample_idx'] * A.T).astype(int)
        frames = np.array([A.FIXTURE_CLIPS[c][1] for c in clip_v])
        duration = np.minimum(A.FPS, frames - (start / float(A.T) * A.FPS).astype(int))
        assert (clip_a == 1).any() and (clip_a == 2).any()                      # shorter than a second; exactly a second
        assert ((clip_v == 1) & (duration > 0)).any()                           # a frame draw over 7 frames
        assert ((clip_v == 0) & (duration > 0) & (duration < A.FPS)).any()      # a late start
        assert (duration <= 0).any() and (duration == A.FPS).any()
        assert set(ref[prefix + '_label'][:, 0]) == {0, 1}


@pytest.mark.parametrize('prefix,augment', [('plain', False), ('aug', True)])
def test_draw_samples_gives_the_references_draws(ref, prefix, augment):
    """Every field of every record: choices, label row, start, frame, crop, and for augmented samples flip, the two factors and
    -- through augment_ref.audio_gain on the slice -- the gain, bit for bit."""
    rec = fixture_records(ref, prefix, augment)
    clips = A.fixture_clips()
    assert [NAMES[i] for i in rec['audio_clip']] == list(ref[prefix + '_audio_file'])
    assert [NAMES[i] for i in rec['video_clip']] == list(ref[prefix + '_video_file'])
    assert np.array_equal(rec['audio_start'].astype(np.float64) / float(A.T), ref[prefix + '_audio_start_sample_idx'])
    assert np.array_equal(rec['frame'], ref[prefix + '_video_start_frame_idx'])
    assert np.array_equal(rec['start_x'], ref[prefix + '_video_bounding_box_start_x'])
    assert np.array_equal(rec['start_y'], ref[prefix + '_video_bounding_box_start_y'])
    assert np.array_equal(avsample.labels_of(rec), ref[prefix + '_label'])
    if not augment:
        assert not rec['flip'].any() and (rec['saturation'] == 1).all() and (rec['brightness'] == 0).all()
        return
    assert np.array_equal(rec['flip'] != 0, ref['aug_video_horizontal_flip'])
    assert np.array_equal(rec['saturation'].view(np.uint32), ref['aug_video_saturation_factor'].astype(np.float32).view(np.uint32))
    assert np.array_equal(rec['brightness'].view(np.uint32), ref['aug_video_brightness_delta'].astype(np.float32).view(np.uint32))
    gains = np.array([augment_ref.audio_gain(A.one_second(clips[int(r['audio_clip'])][1], int(r['audio_start'])), r['u_gain'])
                      for r in rec])
    assert np.array_equal(gains.view(np.uint64), ref['aug_audio_gain'].astype(np.float64).view(np.uint64))
    assert len(set(rec['sat_first'])) == 2


def test_oracle_equals_the_references_outputs(ref):
    """tests/avsample_ref.py on the drawn records == the reference's un-augmented frames and every audio row, exactly."""
    clips = A.fixture_clips()
    rec = fixture_records(ref, 'plain', False)
    video, audio = A.cut(clips, rec)
    assert np.array_equal(video, ref['plain_video'])
    assert np.array_equal(audio, ref['plain_audio'][:, 0])
    rec = fixture_records(ref, 'aug', True)
    _, audio = A.cut(clips, rec)
    rows, gains = augment_ref.augment_audio(audio, rec['u_gain'])
    assert np.array_equal(rows, ref['aug_audio'][:, 0])
    assert np.array_equal(gains, ref['aug_audio_gain'])


def test_downmix_oracle_truncates_toward_zero():
    x = np.array([[-3, -4], [-1, 0], [3, 4], [32767, 32767], [-32768, -32768], [-32768, 32767]], np.int16)
    assert A.downmix(x).tolist() == [-3, 0, 3, 32767, -32768, 0]
    assert A.downmix(x[:, 0]).tolist() == x[:, 0].tolist()


class _Scripted(object):
    """A stand-in for random.Random whose choice() answers are scripted and whose shuffle() reverses."""

    def __init__(self, choices):
        self.choices = list(choices)

    def choice(self, seq):
        return seq[self.choices.pop(0)]

    def shuffle(self, x):
        x.reverse()


def test_pair_formation_known_answer():
    """sample.py:538-553 by hand: clip 0 draws 0 (itself: again) then 2; clip 1 draws 1, then 0; clip 2 draws 2, 2, then 1.
    Pairs [(0, 2), (1, 0), (2, 1)], then the shuffle -- here a reversal."""
    rng = _Scripted([0, 2, 1, 0, 2, 2, 1])
    assert avsample.form_pairs(rng, 3) == [(2, 1), (1, 0), (0, 2)]
    assert rng.choices == []
    # two distractors per clip: two pairs per clip, in clip order before the shuffle
    rng = _Scripted([1, 2, 0, 0, 1, 0])
    assert avsample.form_pairs(rng, 3, 2) == [(2, 0), (2, 1), (1, 0), (1, 0), (0, 2), (0, 1)]
    # the sampler's pairs are form_pairs of its own generator, every clip once in front and never paired with itself
    bank = _Bank(5)
    s = avsample.ClipSampler(bank, random_state=7, num_distractors=2)
    assert s.pairs == avsample.form_pairs(random.Random(7), 5, 2)
    assert sorted(a for a, _ in s.pairs) == sorted(list(range(5)) * 2) and all(a != b for a, b in s.pairs)
    with pytest.raises(ValueError, match='at least two clips'):
        avsample.ClipSampler(_Bank(1))


class _Bank(object):
    """What ClipSampler needs of a bank to draw: .clips"""

    def __init__(self, n):
        self.clips = [avsample.clip_info(20 + 7 * i, 240 + i, 320, 40000 + 30000 * i, resize=256, name='c%d' % i) for i in range(n)]


def _take(sampler, n_batches):
    out = []
    for _ in range(n_batches):
        x, y = next(sampler)
        assert np.array_equal(y, avsample.labels_of(x.sample_records)) and y.dtype == np.int64
        out.append(x.sample_records.copy())
    return np.concatenate(out)


def test_multiplexer_follows_its_stated_rule():
    bank = _Bank(6)
    kw = dict(batch_size=16, k=3, rate=4, augment=True)
    a = _take(avsample.ClipSampler(bank, random_state=5, **kw), 6)
    b = _take(avsample.ClipSampler(bank, random_state=5, **kw), 6)
    c = _take(avsample.ClipSampler(bank, random_state=6, **kw), 6)
    assert a.tobytes() == b.tobytes()                     # reproducible from its seed
    assert a.tobytes() != c.tobytes()
    s = avsample.ClipSampler(bank, random_state=5, **kw)
    s.trace = []
    rec = _take(s, 6)
    assert rec.tobytes() == a.tobytes()                   # tracing changes nothing
    budgets = np.random.RandomState(5)
    for i, (pair, left, active) in enumerate(s.trace):
        assert len(active) <= 3 and pair in active        # never more than k pairs, and the sample's pair is one of them
        assert {int(rec['video_clip'][i]), int(rec['audio_clip'][i])} <= set(pair)
        assert left >= 0
    # budgets: every run of one slot's pair ends at 0 after max(1, poisson(rate)) samples; the first three are the generator's first
    first = [max(1, int(budgets.poisson(4))) for _ in range(3)]
    spent = {}
    for pair, left, active in s.trace:
        spent.setdefault(pair, []).append(left)
    for pair, want in zip(s.pairs[:3], first):
        run = spent[pair][:want]
        assert run == list(range(want - 1, -1, -1)), (pair, want, run)
    # every record is within its clips
    for r in rec:
        v, au = bank.clips[int(r['video_clip'])], bank.clips[int(r['audio_clip'])]
        assert 0 <= r['frame'] < v.frames and 0 <= r['audio_start'] <= max(au.samples - A.T, 0)
        assert 0 <= r['start_x'] < v.out_height - 224 and 0 <= r['start_y'] < v.out_width - 224


def test_multiplexer_without_cycle_ends():
    bank = _Bank(4)
    s = avsample.ClipSampler(bank, batch_size=4, random_state=3, k=2, rate=3, cycle=False)
    s.trace = []
    n = 0
    with pytest.raises(StopIteration):
        for _ in range(1000):
            next(s)
            n += 1
    assert 0 < n < 1000
    # every pair was opened once and spent whole
    ends = [pair for pair, left, _ in s.trace if left == 0]
    assert sorted(ends) == sorted(s.pairs)
    # cycle=True goes on past the list
    s = avsample.ClipSampler(bank, batch_size=4, random_state=3, k=2, rate=3, cycle=True)
    _take(s, n + 8)


class _FakeHandle(object):
    def __init__(self, device, pixel_bytes, audio_samples, resize):
        self.h, self.added = None, []

    def add(self, frames, audio):
        self.added.append((frames.shape, audio.shape))
        return len(self.added) - 1

    def info(self, clip):
        (t, h, w, _), (n, _) = self.added[clip]
        return tuple(avsample.clip_info(t, h, w, n, self.resize)[:6])

    def close(self):
        pass


def test_refusals(monkeypatch):
    monkeypatch.setattr(_lib, 'ClipBank', _FakeHandle)
    frames, audio = np.zeros((3, 230, 240, 3), np.uint8), np.zeros((50000, 2), np.int16)
    bank = avsample.ClipBank(0, 1 << 20, 1 << 20, resize=None)
    bank._handle.resize = None
    with pytest.raises(ValueError, match='resample.resample'):
        bank.add(frames, audio, 44100)
    with pytest.raises(ValueError, match='225'):
        bank.add(frames[:, :224], audio, 48000)
    with pytest.raises(ValueError, match='uint8 frames and int16 PCM'):
        bank.add(frames.astype(np.float32), audio, 48000)
    assert bank._handle.added == []                       # nothing reached the library
    assert bank.add(frames, audio, 48000, name='x') == 0 and bank.clips[0].samples == 50000 and bank.clips[0].name == 'x'
    with pytest.raises(ValueError, match='at least two clips'):
        avsample.ClipSampler(bank)
    with pytest.raises(ValueError, match='pixel_bytes'):
        avsample.ClipBank(0)
    with pytest.raises(ValueError, match='resize'):
        avsample.ClipBank(0, 1, 1, resize=224)
    # a resizing bank takes small frames: read_video's rule makes them 256 on the shorter side
    small = avsample.ClipBank(0, 1 << 20, 1 << 20)
    small._handle.resize = 256
    small.add(np.zeros((2, 120, 160, 3), np.uint8), audio[:, 0], 48000)
    assert small.clips[0][3:5] == (256, 342)
    # replicas > 1, data-parallel or serial, refuse a sampled batch before any engine exists
    rec = np.zeros(4, avsample.SAMPLE)
    for serial in (True, False):
        m, _, _ = MODELS['tiny_L3'](num_gpus=1)
        m.compile(Adam(lr=1e-3), loss='categorical_crossentropy', metrics=['accuracy'])
        m.as_data_parallel(2, serial=serial)
        with pytest.raises(ValueError, match='2-replica'):
            m.train_on_batch(avsample.SampledInputs(bank, rec), avsample.labels_of(rec))
        assert m._engine is None


# ---- train_sampled -------------------------------------------------------------------------------------------------------
class _StubModel(object):
    """Stands in for the engine-backed model: records what fit_generator was handed."""

    def compile(self, *a, **k):
        pass

    def get_config(self):
        return {}

    def to_json(self):
        return '{}'

    def save_weights(self, path, overwrite=True):
        open(path, 'wb').close()

    def fit_generator(self, generator, steps_per_epoch, epochs=1, validation_data=None, **_):
        self.train_batches = [next(generator) for _ in range(2)]
        self.validation_batches = [next(validation_data)]
        from l3embedding_amd.model import History
        return History()


def test_train_sampled_config_and_feeds(tmp_path, monkeypatch):
    """The training feed is a ClipSampler over the bank with the recorded arguments; validation still comes from blobs, plain;
    config.json is train()'s plus `sampled` and `sampler_args`; train() itself is as before."""
    import inspect
    import json
    from l3embedding_amd import h5lite, train as T
    stub = _StubModel()
    monkeypatch.setitem(T.MODELS, 'tiny_L3', lambda num_gpus=0: (stub, None, None))
    va = str(tmp_path / 'set_valid')
    os.makedirs(va)
    rs = np.random.RandomState(0)
    root = h5lite.Group()
    root.create_dataset('audio', rs.randint(-99, 99, (8, 1, 48)).astype(np.int16))
    root.create_dataset('video', rs.randint(0, 256, (8, 224, 224, 3)).astype(np.uint8))
    root.create_dataset('label', np.stack([np.arange(8) % 2, 1 - np.arange(8) % 2], 1).astype(np.int64))
    h5lite.write_file(os.path.join(va, 'blob.h5'), root)
    bank = _Bank(4)
    kw = dict(num_epochs=1, train_epoch_size=2, validation_epoch_size=1, train_batch_size=4, validation_batch_size=4,
              model_type='tiny_L3', disable_logging=True, random_state=31)
    T.train_sampled(bank, va, str(tmp_path / 'out'), 'set_train', sampler_args=dict(augment=True, k=2, rate=3), **kw)
    want = avsample.ClipSampler(bank, batch_size=4, random_state=31, augment=True, k=2, rate=3)
    for x, y in stub.train_batches:
        wx, wy = next(want)
        assert x.bank is bank and x.augmented and x.sample_records.tobytes() == wx.sample_records.tobytes() and np.array_equal(y, wy)
    vx, vy = stub.validation_batches[0][:2]
    assert vx[0].dtype == np.uint8 and not hasattr(vx, 'sample_records') and not hasattr(vx, 'augment')
    (path,) = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / 'out')) for f in fs if f == 'config.json']
    assert os.sep + os.path.join('embedding', 'set', 'tiny_L3') + os.sep in path
    with open(path) as fh:
        config = json.load(fh)
    assert config['sampled'] is True
    assert config['sampler_args'] == dict(batch_size=4, random_state=31, augment=True, k=2, rate=3)
    assert set(config) == set(inspect.signature(T.train).parameters) | {'username', 'model_id', 'model_dir', 'git_commit', 'backend',
                                                                         'sampled', 'sampler_args'}
    with pytest.raises(TypeError, match='bogus'):
        T.train_sampled(bank, va, str(tmp_path / 'x'), 'set_train', bogus=1)
    with pytest.raises(ValueError, match='one GPU'):
        T.train_sampled(bank, va, str(tmp_path / 'x'), 'set_train', gpus=2)
    with pytest.raises(ValueError, match='batch_size'):
        T.train_sampled(bank, va, str(tmp_path / 'x'), 'set_train', sampler_args=dict(batch_size=8), **kw)
