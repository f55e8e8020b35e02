"""Resampling and dataset generation on the host: the NumPy restatement of resampy (tests/resample_ref.py) against physics,
the kaiser_best table, the two time conventions, output lengths, read_wav on every supported encoding, argument validation of
the resample entry points (before any device call), predict_clips(rates=...) with a stand-in engine, and the 05 walkers / CLI
with a stand-in model through to classifier.train with a stand-in MLP."""
import csv
import json
import logging
import os
import struct
import wave

import numpy as np
import pytest

from l3embedding_amd import _lib, classifier, cli_embedding_samples, features, model, resample, usc_generate
from resample_ref import resample_ref
from test_clip_frames import F, FakeBase, FakeEngine, frames_from_table

RATES = [8000, 22050, 44100, 96000]


def _edges(n, sr=48000, margin=0.1):
    t = np.arange(n) / float(sr)
    return (t >= margin) & (t <= n / float(sr) - margin)


@pytest.mark.parametrize('sr', RATES)
def test_restatement_reproduces_a_sine(sr):
    win, nt = resample.kaiser_best()
    x = np.sin(2 * np.pi * 1000 * np.arange(sr) / sr).astype(np.float32)
    y = resample_ref(x, sr, 48000, win, nt)
    ref = np.sin(2 * np.pi * 1000 * np.arange(y.size) / 48000.0)
    assert np.abs(y - ref)[_edges(y.size)].max() <= 2e-6


@pytest.mark.parametrize('sr', RATES)
def test_restatement_dc_gain(sr):
    win, nt = resample.kaiser_best()
    y = resample_ref(np.ones(sr, np.float32), sr, 48000, win, nt)
    assert np.abs(y - 1)[_edges(y.size)].max() <= 2e-6


def test_kaiser_best_table():
    win, nt = resample.kaiser_best()
    assert nt == 512 and win.shape == (32769,) and win.dtype == np.float64
    assert win[0] == resample.KAISER_BEST['rolloff']
    assert resample.kaiser_best()[0] is win                 # cached
    try:
        from scipy.signal import windows
    except ImportError:
        return
    p = resample.KAISER_BEST
    ref = p['rolloff'] * np.sinc(p['rolloff'] * np.linspace(0, 64, 32769)) * windows.kaiser(65537, p['beta'])[32768:]
    assert np.abs(win - ref).max() <= 1e-15


@pytest.mark.parametrize('sr', [8000, 11025, 16000, 22050, 32000, 44100, 96000, 192000])
def test_time_conventions_differ_by_float32_ulps(sr):
    # exact rational time (the kernel) against resampy's accumulated f64 register, on these inputs: 9.54e-7 of max|x| at 8 kHz
    # (8 float32 ulps), 8.34e-7 at 16 and 32 kHz, 5.96e-7 at 44.1, 4.17e-7 at 22.05, 3.58e-7 at 11.025, 0 at 96 and 192 kHz
    # (1 / ratio is exact there).  The 1e-6 bound is the issue's; 8 kHz passes it with only 5 % to spare.
    win, nt = resample.kaiser_best()
    x = np.random.RandomState(sr).uniform(-1, 1, 2 * sr + 13).astype(np.float32)
    a = resample_ref(x, sr, 48000, win, nt, exact_time=True)
    b = resample_ref(x, sr, 48000, win, nt, exact_time=False)
    assert np.abs(a - b).max() <= 1e-6 * np.abs(x).max()


def test_output_lengths_and_errors():
    for n, sr in ((1, 8000), (7, 44100), (44101, 44100), (3, 96000), (2, 96000), (12345, 22050), (999, 11025), (4, 192000)):
        assert resample.output_length(n, sr, 48000) == int(n * (48000.0 / sr))
        win, nt = resample.kaiser_best()
        assert resample_ref(np.zeros(n, np.float32), sr, 48000, win, nt).size == int(n * (48000.0 / sr))
    with pytest.raises(ValueError, match=r'Input signal length=1 is too small to resample from 96000->48000'):
        resample.output_length(1, 96000, 48000)
    with pytest.raises(ValueError, match='Input signal length=1 is too small'):
        resample.resample(np.zeros(1, np.float32), 96000, 48000)
    with pytest.raises(ValueError, match='Invalid sample rate: sr_orig=0'):
        resample.resample(np.zeros(10, np.float32), 0, 48000)
    with pytest.raises(ValueError, match='whole numbers'):
        resample.resample(np.zeros(10, np.float32), 44100.5, 48000)
    with pytest.raises(NotImplementedError):
        resample.resample(np.zeros(10, np.float32), 44100, 48000, filter='kaiser_fast')


def test_resample_ops_validate_on_the_host():
    # checked before any device is touched: the same errors with or without a GPU
    win, nt = resample.kaiser_best()
    x = np.zeros(100, np.float32)
    for call, what in ((lambda: _lib.op_resample(x, 0, 48000, win, nt, 0, 10), 'sr_orig <= 0'),
                       (lambda: _lib.op_resample(x, 44100, -1, win, nt, 0, 10), 'sr_new <= 0'),
                       (lambda: _lib.op_resample(x, 44100, 48000, win, nt, 100, 10), 'past the output length'),
                       (lambda: _lib.op_resample(x[:1], 96000, 48000, win, nt, 0, 0), 'too short'),
                       (lambda: _lib.op_resample_clips(x, [(50, 60, 44100, 0, 1, 0)], 48000, win, nt, 10), 'outside the upload'),
                       (lambda: _lib.op_resample_clips(x, [(-1, 60, 44100, 0, 1, 0)], 48000, win, nt, 10), 'outside the upload'),
                       (lambda: _lib.op_resample_clips(x, [(0, 60, 44100, 0, 5, 8)], 48000, win, nt, 10), 'destination'),
                       (lambda: _lib.op_resample_clips(x, [(0, 60, 48000, 0, 61, 0)], 48000, win, nt, 100, True), 'past'),
                       # t * sr_orig must stay inside int64 for every output the row asks for
                       (lambda: _lib.op_resample_clips(x, [(0, 1 << 40, 1 << 24, 0, 1, 0)], 48000, win, nt, 10), '2\\^62'),
                       (lambda: _lib.op_resample_clips(x, [(0, 1 << 40, 8000, 0, 1, 0)], 1 << 24, win, nt, 10), '2\\^62')):
        with pytest.raises(_lib.L3Error, match='error -1: .*' + what):
            call()
    lib = _lib.load()
    assert lib.l3_op_resample(0, None, 0, 44100, 48000, None, 0, 512, 0, 0, None) == -1
    assert b'NULL' in lib.l3_last_error(None)


# -- read_wav ------------------------------------------------------------------------------------------------------------------
def _stdlib_wav(path, frames_bytes, nch, width, rate):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(nch)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(frames_bytes)


def _riff(path, tag, nch, rate, bits, data, extensible_sub=None):
    block = nch * bits // 8
    if extensible_sub is None:
        fmt = struct.pack('<HHIIHH', tag, nch, rate, rate * block, block, bits)
    else:
        guid = struct.pack('<H', extensible_sub) + b'\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'
        fmt = struct.pack('<HHIIHHHHI', 0xFFFE, nch, rate, rate * block, block, bits, 22, bits, 0) + guid
    extra = b'LIST' + struct.pack('<I', 5) + b'INFOx\x00'         # an odd-sized chunk before the data: pad byte honoured
    body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + extra + b'data' + struct.pack('<I', len(data)) + data
    with open(str(path), 'wb') as fh:
        fh.write(b'RIFF' + struct.pack('<I', len(body)) + body)


@pytest.mark.parametrize('nch', [1, 2])
def test_read_wav_pcm_known_answers(tmp_path, nch):
    r = np.random.RandomState(nch)
    n = 501
    u8 = r.randint(0, 256, size=(n, nch)).astype(np.uint8)
    _stdlib_wav(tmp_path / 'u8.wav', u8.tobytes(), nch, 1, 8000)
    x, sr = features.read_wav(str(tmp_path / 'u8.wav'))
    assert sr == 8000 and x.dtype == np.float32
    assert np.array_equal(x, ((u8.astype(np.float32) - 128) / np.float32(128)).mean(-1))
    i16 = r.randint(-32768, 32768, size=(n, nch)).astype('<i2')
    _stdlib_wav(tmp_path / 'i16.wav', i16.tobytes(), nch, 2, 22050)
    x, sr = features.read_wav(str(tmp_path / 'i16.wav'))
    assert sr == 22050 and np.array_equal(x, (i16.astype(np.float32) * np.float32(2.0 ** -15)).mean(-1))
    i24 = r.randint(-(1 << 23), 1 << 23, size=(n, nch))
    _stdlib_wav(tmp_path / 'i24.wav', np.ascontiguousarray(i24.astype('<i4').view(np.uint8).reshape(-1, 4)[:, :3]).tobytes(),
                nch, 3, 44100)
    x, sr = features.read_wav(str(tmp_path / 'i24.wav'))
    assert sr == 44100 and np.array_equal(x, (i24.astype(np.float32) * np.float32(2.0 ** -23)).mean(-1))
    assert x.min() < -0.5 and x.max() > 0.5 or nch == 2                # the sign extension at work
    i32 = r.randint(-(1 << 31), (1 << 31) - 1, size=(n, nch)).astype('<i4')
    _stdlib_wav(tmp_path / 'i32.wav', i32.tobytes(), nch, 4, 96000)
    x, sr = features.read_wav(str(tmp_path / 'i32.wav'))
    assert sr == 96000 and np.array_equal(x, (i32.astype(np.float32) * np.float32(2.0 ** -31)).mean(-1))
    _riff(tmp_path / 'e24.wav', 0, nch, 16000, 24, i24.astype('<i4').view(np.uint8).reshape(-1, 4)[:, :3].tobytes(),
          extensible_sub=1)
    x, sr = features.read_wav(str(tmp_path / 'e24.wav'))
    assert sr == 16000 and np.array_equal(x, (i24.astype(np.float32) * np.float32(2.0 ** -23)).mean(-1))


@pytest.mark.parametrize('nch', [1, 2])
def test_read_wav_float_known_answers(tmp_path, nch):
    r = np.random.RandomState(10 + nch)
    f32 = r.uniform(-1.5, 1.5, size=(333, nch)).astype('<f4')
    _riff(tmp_path / 'f32.wav', 3, nch, 44100, 32, f32.tobytes())
    x, sr = features.read_wav(str(tmp_path / 'f32.wav'))
    assert sr == 44100 and np.array_equal(x, f32.mean(-1))
    f64 = r.randn(333, nch).astype('<f8')
    _riff(tmp_path / 'f64.wav', 3, nch, 48000, 64, f64.tobytes())
    x, sr = features.read_wav(str(tmp_path / 'f64.wav'))
    assert sr == 48000 and np.array_equal(x, f64.astype(np.float32).mean(-1))
    _riff(tmp_path / 'ef.wav', 0, nch, 32000, 32, f32.tobytes(), extensible_sub=3)
    x, sr = features.read_wav(str(tmp_path / 'ef.wav'))
    assert sr == 32000 and np.array_equal(x, f32.mean(-1))


@pytest.mark.parametrize('nch', [1, 2])
def test_read_wav_equals_load_audio_on_pcm16_48k(tmp_path, nch):
    pcm = np.random.RandomState(nch).randint(-32768, 32768, size=(7001, nch)).astype('<i2')
    _stdlib_wav(tmp_path / 'c.wav', pcm.tobytes(), nch, 2, 48000)
    x, sr = features.read_wav(str(tmp_path / 'c.wav'))
    assert sr == 48000 and np.array_equal(x, features.load_audio(str(tmp_path / 'c.wav'), 48000))
    # at the asked rate read_audio does not resample (no device needed)
    assert np.array_equal(features.read_audio(str(tmp_path / 'c.wav'), 48000), x)


def test_read_wav_rejects_other_encodings(tmp_path):
    for tag, name in ((2, 'MS ADPCM'), (7, 'mu-law'), (6, 'A-law'), (0x11, 'IMA ADPCM')):
        _riff(tmp_path / 'x.wav', tag, 1, 8000, 8 if tag in (6, 7) else 4, b'\x00' * 64)
        with pytest.raises(ValueError, match=name):
            features.read_wav(str(tmp_path / 'x.wav'))
    _riff(tmp_path / 'e.wav', 0, 1, 8000, 8, b'\x00' * 64, extensible_sub=7)
    with pytest.raises(ValueError, match='sub-format mu-law'):
        features.read_wav(str(tmp_path / 'e.wav'))
    (tmp_path / 'n.wav').write_bytes(b'ID3\x04' + b'\x00' * 64)
    with pytest.raises(ValueError, match='not a RIFF WAVE'):
        features.read_wav(str(tmp_path / 'n.wav'))


# -- predict_clips(rates=...) with a stand-in engine that resamples with the restatement -----------------------------------------
class ResamplingFakeEngine(FakeEngine):
    def embed_audio_clips_resampled(self, native, clips, half_window, num_table, n_samples, table, pool, out=None):
        buf = np.zeros(n_samples, np.float32)
        for x_off, L, sr, t0, n, y_off in np.asarray(clips).tolist():
            assert 0 <= x_off and x_off + L <= native.size and 0 <= y_off and y_off + n <= n_samples
            c = native[x_off:x_off + L]
            full = c if sr == 48000 else resample_ref(c, sr, 48000, half_window, num_table)
            buf[y_off:y_off + n] = full[t0:t0 + n]
        self.calls.append((n_samples, len(table)))
        out[:] = frames_from_table(buf, table)
        return out


NATIVE = [(44100 + 3 * 4410, 44100), (30000, 48000), (20000, 22050), (0, 48000), (2 * 96000 + 5, 96000), (500, 8000),
          (3 * 44100 + 77, 44100)]


@pytest.mark.parametrize('scope', ['sample', 'batch'])
def test_predict_clips_rates_layout(monkeypatch, scope):
    base = FakeBase(3, scope)
    base.eng = ResamplingFakeEngine(3)
    em = model.EmbeddingModel(base, 'audio', (8, 8))
    monkeypatch.setattr(model.EmbeddingModel, 'CLIP_CALL_FRAMES', 7)
    monkeypatch.setattr(model.EmbeddingModel, 'CLIP_CALL_SAMPLES', 2 * F)
    r = np.random.RandomState(0)
    clips = [r.randn(n).astype(np.float32) for n, _ in NATIVE]
    rates = [q for _, q in NATIVE]
    win, nt = resample.kaiser_best()
    got = em.predict_clips(clips, 4800, rates=rates)
    n_calls = len(base.eng.calls)
    ref = em.predict_clips([c if q == 48000 else resample_ref(c, q, 48000, win, nt) for c, q in zip(clips, rates)], 4800)
    assert n_calls > 2 and base.eng.calls[:n_calls] == base.eng.calls[n_calls:]         # the same calls, the same packing
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    with pytest.raises(ValueError, match='one rate per clip'):
        em.predict_clips(clips, 4800, rates=rates[:-1])
    with pytest.raises(ValueError, match='too small'):
        em.predict_clips([np.zeros(1, np.float32)], 4800, rates=[96000])


# -- 05 walkers and CLI with a stand-in model --------------------------------------------------------------------------------------
class StandInModel(object):
    """predict_clips(clips, hop, rates): one row per frame, [clip length, rate, hop, frame index]"""
    def __init__(self):
        self.calls = []

    def predict_clips(self, clips, hop_length, batch_size=32, rates=None):
        self.calls.append(len(clips))
        return [np.array([[c.size, r, hop_length, k] for k in range(1 + c.size // 48000)], np.float32)
                for c, r in zip(clips, rates)]


def _tone_wav(path, n, rate):
    _stdlib_wav(path, (np.arange(n) % 200 * 100).astype('<i2').tobytes(), 1, 2, rate)


def test_esc50_and_dcase_layout_labels_and_skip(tmp_path):
    data, out = tmp_path / 'esc', tmp_path / 'out'
    for f in range(1, 6):
        os.makedirs(str(data / ('fold%d' % f)))
        for c in (3, 17):
            _tone_wav(data / ('fold%d' % f) / ('%d-1000%d-A-%d.wav' % (f, c, c)), 44100 + f, 44100)
    m = StandInModel()
    usc_generate.generate_esc50_folds(str(data), str(out), l3embedding_model=m, hop_size=0.1)
    assert m.calls == [2] * 5                                   # one predict_clips call per fold, both files in it
    with np.load(str(out / 'fold3' / '3-100017-A-17.npz')) as z:
        assert int(z['y']) == 17 and z['X'][0].tolist() == [44103, 44100, 4800, 0]     # native samples and rate
    os.remove(str(out / 'fold2' / '2-10003-A-3.npz'))
    m2 = StandInModel()
    written = usc_generate.generate_esc50_fold_data(str(data), 1, str(out), l3embedding_model=m2)
    assert written == [str(out / 'fold2' / '2-10003-A-3.npz')] and m2.calls == [1]
    # DCASE 2013: CLASS_TO_INT[basename[:-2]]
    dc = tmp_path / 'dcase'
    for f in (1, 2):
        os.makedirs(str(dc / ('fold%d' % f)))
        _tone_wav(dc / ('fold%d' % f) / ('busystreet0%d.wav' % f), 1000, 44100)
        _tone_wav(dc / ('fold%d' % f) / ('tubestation1%d.wav' % f), 1000, 44100)
    usc_generate.generate_dcase2013_folds(str(dc), str(tmp_path / 'dout'), l3embedding_model=StandInModel())
    with np.load(str(tmp_path / 'dout' / 'fold2' / 'tubestation12.npz')) as z:
        assert int(z['y']) == 9
    with np.load(str(tmp_path / 'dout' / 'fold1' / 'busystreet01.npz')) as z:
        assert int(z['y']) == 1
    with pytest.raises(ValueError, match='Invalid feature type'):
        usc_generate.generate_esc50_fold_data(str(data), 0, str(out), l3embedding_model=m, features='vggish')


def test_us8k_variants_labels_and_mp3_skip(tmp_path, caplog):
    data, out = tmp_path / 'us8k', tmp_path / 'out'
    meta = tmp_path / 'UrbanSound8K.csv'
    rows = [('100-1-0-0.wav', 1, 7), ('100-1-0-1.wav', 1, 7), ('200-3-0-0.wav', 2, 3)]
    with open(str(meta), 'w') as fh:
        w = csv.writer(fh)
        w.writerow(['slice_file_name', 'fsID', 'start', 'end', 'salience', 'fold', 'classID', 'class'])
        for name, fold, cid in rows:
            w.writerow([name, 1, 0.0, 1.0, 1, fold, cid, 'x'])
    f1 = data / 'fold1'
    os.makedirs(str(f1 / 'aug'))
    _tone_wav(f1 / '100-1-0-0.wav', 5000, 22050)
    _tone_wav(f1 / 'aug' / '100-1-0-0_pitch1.wav', 5000, 48000)       # a variant in a sub-directory
    _tone_wav(f1 / '100-1-0-1.wav', 5000, 16000)
    _tone_wav(f1 / '100-1-0-10.wav', 5000, 16000)                      # not a variant of 100-1-0-1 ([!0-9] after the stem)
    (f1 / '100-1-0-0.jams').write_text('{}')
    (f1 / '100-1-0-0_bgnoise.mp3').write_bytes(b'ID3')
    os.makedirs(str(data / 'fold2'))
    _tone_wav(data / 'fold2' / '200-3-0-0.wav', 5000, 44100)
    assert sorted(os.path.basename(p) for p in usc_generate.us8k_variants(str(f1), '100-1-0-1.wav')) == ['100-1-0-1.wav']
    m = StandInModel()
    usc_generate.generate_us8k_fold_data(str(meta), str(data), 0, str(out), l3embedding_model=m)
    names = sorted(os.listdir(str(out / 'fold1')))
    assert names == ['100-1-0-0.npz', '100-1-0-0_pitch1.npz', '100-1-0-1.npz']
    assert m.calls == [3]
    assert any('mp3' in rec.getMessage() and rec.levelname == 'ERROR' for rec in caplog.records)
    with np.load(str(out / 'fold1' / '100-1-0-0_pitch1.npz')) as z:
        assert int(z['y']) == 7 and z['X'][0, 1] == 48000
    usc_generate.generate_us8k_folds(str(meta), str(data), str(out), l3embedding_model=m)
    assert sorted(os.listdir(str(out))) == ['fold%d' % k for k in sorted(range(1, 11), key=str)]
    assert os.listdir(str(out / 'fold2')) == ['200-3-0-0.npz']


def test_same_output_name_is_written_once_first_job_wins(tmp_path, caplog):
    # two US8K variants of one name in different sub-directories map to one .npz: the reference writes the first in glob
    # order and then finds the file there for the second
    caplog.set_level(logging.INFO, logger='cls-data-generation')
    f1 = tmp_path / 'us8k' / 'fold1'
    os.makedirs(str(f1 / 'a'))
    os.makedirs(str(f1 / 'b'))
    _tone_wav(f1 / 'a' / '100-1-0-0_x.wav', 5000, 22050)
    _tone_wav(f1 / 'b' / '100-1-0-0_x.wav', 7000, 44100)
    variants = usc_generate.us8k_variants(str(f1), '100-1-0-0.wav')
    out = tmp_path / 'out.npz'
    m = StandInModel()
    written = usc_generate.embed_files([(v, str(out), 1) for v in variants], m)
    assert written == [str(out)] and m.calls == [1]
    first_n = 5000 if os.path.basename(os.path.dirname(variants[0])) == 'a' else 7000
    with np.load(str(out)) as z:
        assert z['X'][0, 0] == first_n
    assert any('already exists' in rec.getMessage() for rec in caplog.records)


def test_cli_defaults_and_refusals(capsys):
    args = cli_embedding_samples.parse_arguments(['-lmp', '/m/embedding/music/cnn_L3_melspec2/20171021/model.h5', 'esc50',
                                                  'data', 'out'])
    assert args == dict(random_state=20171021, verbose=False, features='l3',
                        l3embedding_model_path='/m/embedding/music/cnn_L3_melspec2/20171021/model.h5',
                        l3embedding_pooling_type='original', hop_size=0.1, num_random_samples=None, gpus=0, fold=None,
                        us8k_metadata_path=None, dataset_name='esc50', data_dir='data', output_dir='out')
    assert cli_embedding_samples.features_dir(args) == 'out/features/esc50/l3/original/music/cnn_L3_melspec2'
    for argv, what in ((['-f', 'vggish', '-lmp', 'x/embedding/a/b/m.h5', 'esc50', 'd', 'o'], 'vggish'),
                       (['esc50', 'd', 'o'], 'model path'),
                       (['-lmp', 'x/embedding/a/b/m.h5', 'us8k', 'd', 'o'], 'metadata')):
        with pytest.raises(SystemExit) as exc:
            cli_embedding_samples.parse_arguments(argv)
        assert exc.value.code == 2 and what in capsys.readouterr().err


def test_cli_folds_feed_classifier_train(tmp_path, monkeypatch):
    loaded = {}

    def fake_load_embedding(path, model_type, embedding_type, pooling_type, tgt_num_gpus=None):
        loaded.update(path=path, model_type=model_type, embedding_type=embedding_type, pooling=pooling_type)
        return StandInModel()

    monkeypatch.setattr(model, 'load_embedding', fake_load_embedding)
    data = tmp_path / 'esc'
    for f in range(1, 6):
        os.makedirs(str(data / ('fold%d' % f)))
        for c in range(3):
            for k in range(2):
                _tone_wav(data / ('fold%d' % f) / ('%d-%d%d-A-%d.wav' % (f, c, k, c)), 50000 + 30000 * c, 44100)
    weights = str(tmp_path / 'models' / 'embedding' / 'cnn_L3_melspec2' / 'run' / 'model.h5')
    out = cli_embedding_samples.main(['-lmp', weights, '--fold', '4', 'esc50', str(data), str(tmp_path / 'o')])
    assert loaded == dict(path=weights, model_type='cnn_L3_melspec2', embedding_type='audio', pooling='original')
    assert out == str(tmp_path / 'o' / 'features' / 'esc50' / 'l3' / 'original' / 'cnn_L3_melspec2')
    assert sorted(os.listdir(out)) == ['config_4.json', 'fold4']
    with open(os.path.join(out, 'config_4.json')) as fh:
        assert json.load(fh)['features_dir'] == out
    cli_embedding_samples.main(['-lmp', weights, 'esc50', str(data), str(tmp_path / 'o')])
    assert sorted(os.listdir(out)) == ['config_4.json', 'config_None.json'] + ['fold%d' % f for f in range(1, 6)]

    class FakeMLP(object):
        def __init__(self, D, C, batch, weight_decay=0, seed=0, device=0):
            assert D == 4 and C == 50
            self.batch, self.C = batch, C

        def set_data(self, *a):
            pass

        def epoch(self, perm, lr, t0):
            return dict(loss=1.0, acc=0.0, val_loss=1.0, val_acc=0.0)

        def get_weights(self):
            return [np.zeros(s, np.float32) for s in _lib.mlp_shapes(4, self.C)]

        def set_weights(self, w):
            pass

        def predict(self, x):
            return np.full((len(x), self.C), 1.0 / self.C, np.float32)

        def close(self):
            pass

    monkeypatch.setattr(classifier._lib, 'MLP', FakeMLP)
    run = classifier.train(out, str(tmp_path / 'cls'), 1, model_type='mlp', num_epochs=2)
    assert os.path.exists(os.path.join(run, 'results.pkl'))
