"""Framing of whole clips (data/usc/features.py:18-28,256-306) on the host: features.frame_table against a NumPy
restatement of the reference's padding + librosa.util.frame, load_audio on PCM16 WAV files, and how
EmbeddingModel.predict_clips lays frames into engine batches and calls (with a NumPy stand-in for the engine)."""
import wave

import numpy as np
import pytest

from l3embedding_amd import features, model

F = 48000
LENGTHS = [0, 1, 47999, 48000, 48001, 52799, 52800, 10 * F + 3]
HOPS = [0.05, 0.1, 0.25, 1.0]


def ref_frames(audio, hop_size, sr=48000):
    """features.py:276-300 restated: np.pad + strided framing (librosa.util.frame)."""
    hop_length = int(hop_size * sr)
    frame_length = sr * 1
    audio_length = len(audio)
    if audio_length < frame_length:
        pad_length = frame_length - audio_length
    else:
        pad_length = int(np.ceil(audio_length - frame_length) / hop_length) * hop_length - (audio_length - frame_length)
    if pad_length > 0:
        left_pad = pad_length // 2
        audio = np.pad(audio, (left_pad, pad_length - left_pad), mode='constant')
    n_frames = 1 + (len(audio) - frame_length) // hop_length
    x = np.lib.stride_tricks.as_strided(audio, shape=(n_frames, frame_length),
                                        strides=(audio.strides[0] * hop_length, audio.strides[0]))
    return np.array(x)


def frames_from_table(samples, table):
    out = np.zeros((len(table), F), np.float32)
    j = np.arange(F)
    for r, (start, lo, hi) in enumerate(table):
        idx = start + j
        ok = (idx >= lo) & (idx < hi)
        out[r, ok] = samples[idx[ok]]
    return out


def clip(n, seed):
    return np.random.RandomState(seed).uniform(-1, 1, n).astype(np.float32)


@pytest.mark.parametrize('hop_size', HOPS)
def test_frame_table_matches_reference_framing(hop_size):
    clips = [clip(n, i) for i, n in enumerate(LENGTHS)]
    hop = int(hop_size * 48000)
    table, counts = features.frame_table([len(c) for c in clips], hop)
    assert table.dtype == np.int64 and table.shape == (counts.sum(), 3)
    samples = np.concatenate(clips)
    got = frames_from_table(samples, table)
    r = 0
    for c, n in zip(clips, counts):
        ref = ref_frames(c, hop_size)
        assert n == len(ref)
        assert np.array_equal(got[r:r + n], ref)
        r += n


def test_frame_counts_and_quirks():
    hop = 4800
    _, counts = features.frame_table(LENGTHS, hop)
    assert counts.tolist() == [1, 1, 1, 1, 1, 1, 2, 91]
    t, _ = features.frame_table([0], hop)
    assert frames_from_table(np.zeros(0, np.float32), t).any() == False  # noqa: E712  (one all-zero frame)
    # a 2.5 s clip at hop 0.1: 1 + 72000 // 4800 frames, the last 0.5 - 0.3 s of the tail dropped (no padding)
    assert features.frame_table([120000], hop)[1].tolist() == [16]
    with pytest.raises(ValueError):
        features.frame_table([F], 0)
    with pytest.raises(ValueError):
        features.frame_table([F], int(0 * 48000))


def write_wav(path, pcm, rate=48000, width=2):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


@pytest.mark.parametrize('channels', [1, 2])
def test_load_audio_pcm16(tmp_path, channels):
    x = np.random.RandomState(channels).randint(-32768, 32768, size=(7001, channels)).astype('<i2')
    p = tmp_path / 'clip.wav'
    write_wav(p, x)
    got = features.load_audio(str(p), 48000)
    ref = (x.astype(np.float32) / 32768).mean(-1)
    assert got.dtype == np.float32 and np.array_equal(got, ref)


def test_load_audio_rejects_other_widths_and_rates(tmp_path):
    p24 = tmp_path / 'clip24.wav'
    with wave.open(str(p24), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(3)
        w.setframerate(48000)
        w.writeframes(b'\x00\x01\x02' * 100)
    with pytest.raises(ValueError, match='decode'):
        features.load_audio(str(p24), 48000)
    p = tmp_path / 'clip44.wav'
    write_wav(p, np.zeros((100, 1), '<i2'), rate=44100)
    with pytest.raises(ValueError, match='resample'):
        features.load_audio(str(p), 48000)


def test_gather_op_validates_its_table_on_the_host():
    # checked before any device is touched: the same errors with or without a GPU
    from l3embedding_amd import _lib
    s = np.zeros(10, np.float32)
    for table, what in (([[0, 0, 11]], 'hi > n_samples'), ([[0, 5, 4]], 'lo > hi'), ([[0, -1, 4]], 'lo < 0')):
        with pytest.raises(_lib.L3Error, match='error -1: .*' + what):
            _lib.op_gather_frames(s, np.array(table, np.int64))
    lib = _lib.load()
    assert lib.l3_op_gather_frames(0, None, 0, None, 0, None) == -1
    assert b'NULL' in lib.l3_last_error(None)


def test_get_l3_frames_uniform_rejects_other_models():
    with pytest.raises(TypeError):
        features.get_l3_frames_uniform(np.zeros(100, np.float32), object())


# -- predict_clips with a NumPy stand-in for the engine: the gathered frame is the "embedding" ----------------------------
class FakeLib(object):
    def l3_embed_dim(self, h, vision, ph, pw):
        return F


class FakeEngine(object):
    lib, h = FakeLib(), None

    def __init__(self, batch):
        self.batch = batch
        self.calls = []

    def embed_audio_frames(self, samples, table, pool, out=None):
        s = np.ascontiguousarray(samples, np.float32)
        assert (table[:, 1] >= 0).all() and (table[:, 1] <= table[:, 2]).all() and (table[:, 2] <= s.size).all()
        self.calls.append((s.size, len(table)))
        out[:] = frames_from_table(s, table)
        return out


class FakeBase(object):
    def __init__(self, batch, scope):
        self._engine = None
        self.db_max_scope = scope
        self.eng = FakeEngine(batch)

    def _ensure_engine(self, batch):
        return self.eng


@pytest.mark.parametrize('scope', ['sample', 'batch'])
def test_predict_clips_layout_and_call_split(monkeypatch, scope):
    lengths = [30000, 0, 5 * F + 17, 48000, 100, 3 * F]
    clips = [clip(n, 10 + i) for i, n in enumerate(lengths)]
    hop = 9600
    base = FakeBase(3, scope)
    em = model.EmbeddingModel(base, 'audio', (8, 8))
    monkeypatch.setattr(model.EmbeddingModel, 'CLIP_CALL_FRAMES', 7)       # -> 6 frames (two engine batches) per call
    monkeypatch.setattr(model.EmbeddingModel, 'CLIP_CALL_SAMPLES', 3 * F)
    got = em.predict_clips(clips, hop)
    assert len(got) == len(clips)
    for c, g in zip(clips, got):
        assert np.array_equal(g, ref_frames(c, hop / 48000.0))
    calls = base.eng.calls
    assert len(calls) > 2 and all(n <= 6 or n == 3 for _, n in calls)
    assert all(s <= 3 * F or n == 3 for s, n in calls)
    if scope == 'batch':           # every clip starts an engine batch: 1 + 1 + 21 + 1 + 1 + 11 frames padded to multiples of 3
        assert sum(n for _, n in calls) == 3 + 3 + 21 + 3 + 3 + 12
    else:
        assert sum(n for _, n in calls) == 1 + 1 + 21 + 1 + 1 + 11
    assert em.predict_clips([], hop) == []
