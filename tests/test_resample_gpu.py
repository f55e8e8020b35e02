"""Resampling on the GPU (resampy.resample, data/usc/features.py:25-26): the kernel against the NumPy restatement
(tests/resample_ref.py, exact output times) bit for bit, output sub-ranges and mixed-rate launches, predict_clips(rates=...)
against predict_clips on host-resampled clips, read_audio, and the 05 CLI through to the MLP classifier."""
import importlib.util
import os
import wave

import numpy as np
import pytest

from l3embedding_amd import _lib, classifier, cli_embedding_samples, features, model, resample
from oracle import l3_oracle as o
from resample_ref import resample_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
UP = [8000, 11025, 16000, 22050, 32000, 44100]
DOWN = [96000, 192000]


def _mod():
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(GOLDEN, 'make_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _clip(n, seed):
    return (0.5 * np.random.RandomState(seed).randn(n)).astype(np.float32)


@pytest.mark.parametrize('sr', UP + DOWN)
def test_kernel_matches_restatement_bit_for_bit(gpu_required, sr):
    win, nt = resample.kaiser_best()
    shortest = 1 if sr < 48000 else -(-sr // 48000)         # output length int(L * 48000 / sr) >= 1
    for k, n in enumerate([shortest, 100, 3 * sr + 7]):     # one sample, shorter than the filter, several seconds
        x = _clip(n, sr + k)
        got = resample.resample(x, sr, 48000)
        ref = resample_ref(x, sr, 48000, win, nt)
        assert got.dtype == np.float32 and got.shape == ref.shape == (int(n * (48000.0 / sr)),)
        assert np.array_equal(got, ref), (sr, n, np.abs(got - ref).max())


@pytest.mark.parametrize('sr', [22050, 44100, 96000])
def test_output_ranges_are_slices_of_the_whole_clip(gpu_required, sr):
    win, nt = resample.kaiser_best()
    x = _clip(2 * sr + 3, 7)
    whole = resample.resample(x, sr, 48000)
    m = whole.size
    for t0, t1 in ((0, 1), (0, 300), (17, 4000), (m // 2 - 5, m // 2 + 700), (m - 257, m), (m - 1, m)):
        assert np.array_equal(_lib.op_resample(x, sr, 48000, win, nt, t0, t1 - t0), whole[t0:t1]), (t0, t1)


def test_mixed_rate_launch_equals_per_clip_launches(gpu_required):
    win, nt = resample.kaiser_best()
    rates = [44100, 8000, 48000, 96000, 22050, 192000, 48000]
    clips = [_clip(n, i) for i, n in enumerate([44100 + 5, 900, 3000, 96000 * 2 + 1, 17, 800, 0])]
    x = np.concatenate(clips)
    rows, pos, dst, expect = [], 0, 3, []
    for c, r in zip(clips, rates):
        if r == 48000:
            full = c
        else:
            full = resample.resample(c, r, 48000)
        t0 = min(5, full.size)
        rows.append((pos, c.size, r, t0, full.size - t0, dst))
        expect.append((dst, full[t0:]))
        pos += c.size
        dst += full.size - t0 + 11                  # gaps stay zero
    got = _lib.op_resample_clips(x, rows, 48000, win, nt, dst, copy_equal=True)
    ref = np.zeros(dst, np.float32)
    for d, y in expect:
        ref[d:d + y.size] = y
    assert np.array_equal(got, ref)
    # without copy_equal a 48 kHz row is filtered, as resampy filters it
    one = _lib.op_resample_clips(clips[2], [(0, 3000, 48000, 0, 3000, 0)], 48000, win, nt, 3000)
    assert np.array_equal(one, resample_ref(clips[2], 48000, 48000, win, nt))


HOP = 4800
# native lengths at mixed rates: short, empty-at-48k, multi-second clips whose frames straddle engine batches of 2 and 3
NATIVE = [(44100 + 3 * 4410, 44100), (30000, 48000), (20000, 22050), (0, 48000), (2 * 96000 + 5, 96000), (500, 8000),
          (3 * 44100 + 77, 44100)]


@pytest.mark.parametrize('batch,scope', [(2, 'sample'), (3, 'sample'), (2, 'batch'), (3, 'batch')])
def test_predict_clips_rates_equals_host_resampled(gpu_required, monkeypatch, batch, scope):
    mt = 'cnn_L3_melspec2'
    P = _mod().perturbed_params(mt, 71)
    m = model.L3Model(mt, db_max_scope=scope)
    e = m._ensure_engine(batch)
    e.set_params(P)
    em = model.EmbeddingModel(m, 'audio', o.AUDIO_POOLING[mt]['original'])
    clips = [_clip(n, 40 + i) for i, (n, _) in enumerate(NATIVE)]
    rates = [r for _, r in NATIVE]
    host = [c if r == 48000 else resample.resample(c, r, 48000) for c, r in zip(clips, rates)]
    # small calls: the long clips are split across calls
    monkeypatch.setattr(model.EmbeddingModel, 'CLIP_CALL_FRAMES', 3 * batch)
    monkeypatch.setattr(model.EmbeddingModel, 'CLIP_CALL_SAMPLES', 2 * 48000)
    got = em.predict_clips(clips, HOP, rates=rates)
    ref = em.predict_clips(host, HOP)
    assert [g.shape for g in got] == [r.shape for r in ref]
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)


def test_engine_filter_tables_follow_the_window(gpu_required):
    # the engine keeps its filter tables across calls: a call with another half window must not reuse the old ones
    mt = 'cnn_L3_melspec2'
    eng = _lib.Engine(mt, 2)
    eng.set_params(_mod().perturbed_params(mt, 31))
    pool = o.AUDIO_POOLING[mt]['original']
    win, nt = resample.kaiser_best()
    for sr in (44100, 96000):
        x = _clip(sr + 2 * sr // 10, sr)
        n48 = resample.output_length(x.size, sr, 48000)
        table, _ = features.frame_table([n48], HOP)
        for w in (win, win * 0.5, win):
            got = eng.embed_audio_clips_resampled(x, [(0, x.size, sr, 0, n48, 0)], w, nt, n48, table, pool)
            ref = eng.embed_audio_frames(_lib.op_resample(x, sr, 48000, w, nt), table, pool)
            assert np.array_equal(got, ref), (sr, w[0])
    eng.close()


def _write_wav24(path, pcm24, rate):
    b = pcm24.astype('<i4').view(np.uint8).reshape(-1, 4)[:, :3]
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(pcm24.shape[1])
        w.setsampwidth(3)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(b).tobytes())


def test_read_audio_resamples_a_24bit_stereo_file(gpu_required, tmp_path):
    pcm = np.random.RandomState(3).randint(-(1 << 23), 1 << 23, size=(44100 + 99, 2))
    p = tmp_path / 'clip.wav'
    _write_wav24(p, pcm, 44100)
    x, sr = features.read_wav(str(p))
    assert sr == 44100
    win, nt = resample.kaiser_best()
    got = features.read_audio(str(p), 48000)
    assert np.array_equal(got, resample_ref(x, 44100, 48000, win, nt))
    p48 = tmp_path / 'clip48.wav'
    _write_wav24(p48, pcm, 48000)
    assert np.array_equal(features.read_audio(str(p48), 48000), features.read_wav(str(p48))[0])     # no resampling


def test_esc50_tree_through_cli_and_classifier(gpu_required, tmp_path):
    # tiny_L3 has no audio embedding layer; the smallest embedding model is used instead
    mt = 'cnn_L3_melspec2'
    m, _, _ = model.MODELS[mt]()
    m.compile(model.Adam(lr=1e-4), loss='categorical_crossentropy', metrics=['accuracy'])
    wdir = tmp_path / 'models' / 'embedding' / mt / 'run1'
    os.makedirs(str(wdir))
    weights = str(wdir / 'model.h5')
    m.save_weights(weights)
    data = tmp_path / 'ESC-50'
    r = np.random.RandomState(9)
    for f in range(1, 6):
        os.makedirs(str(data / ('fold%d' % f)))
        for c in range(2):
            for k in range(2):
                tone = np.sin(2 * np.pi * (300 + 900 * c) * np.arange(44100 + 2205) / 44100) * 0.4
                pcm = ((tone + 0.05 * r.randn(tone.size)) * 32767).astype('<i2')[:, None]
                with wave.open(str(data / ('fold%d' % f) / ('%d-%d%d-A-%d.wav' % (f, c, k, c))), 'wb') as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(44100)
                    w.writeframes(pcm.tobytes())
    out = cli_embedding_samples.main(['-lmp', weights, '-lpt', 'short', 'esc50', str(data), str(tmp_path / 'out')])
    assert out == str(tmp_path / 'out' / 'features' / 'esc50' / 'l3' / 'short' / mt)
    assert os.path.exists(os.path.join(out, 'config_None.json'))
    em = model.load_embedding(weights, mt, 'audio', 'short')
    x, sr = features.read_wav(str(data / 'fold2' / '2-11-A-1.wav'))
    with np.load(os.path.join(out, 'fold2', '2-11-A-1.npz')) as z:
        assert int(z['y']) == 1
        ref = features.get_l3_frames_uniform(resample.resample(x, sr, 48000), em)
        # another engine batch: equal up to the solo Winograd tail split's last bits (profiles/r07_clip_embedding.txt)
        assert z['X'].shape == ref.shape and np.abs(z['X'] - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    run = classifier.train(out, str(tmp_path / 'cls'), 1, model_type='mlp', num_epochs=3)
    assert os.path.exists(os.path.join(run, 'results.pkl'))
