"""Audio embeddings of whole clips on the GPU (data/usc/features.py:256-306, get_l3_frames_uniform): the frame gather
against NumPy framing, predict_clips against l3_embed_audio on host-cut frames (bit for bit), the float64 oracle, the
reference entry points end to end, and argument validation of l3_embed_audio_frames."""
import importlib.util
import os
import wave

import numpy as np
import pytest

from l3embedding_amd import _lib, features, model
from oracle import l3_oracle as o
from test_clip_frames import F, frames_from_table, ref_frames

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
HOP = 4800
# ragged clips: empty, short, exactly one second, long ones whose frame counts straddle engine batches of 2 and 3
LENGTHS = [30000, 0, F + 4 * HOP + 7, 100, F, F + 2 * HOP]


def _mod():
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(GOLDEN, 'make_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _clips(lengths, seed):
    r = np.random.RandomState(seed)
    return [(0.5 * r.randn(n)).astype(np.float32) for n in lengths]


def test_gather_frames_op_matches_numpy(gpu_required):
    clips = _clips(LENGTHS + [3 * F + 11], 1)
    table, counts = features.frame_table([len(c) for c in clips], HOP)
    samples = np.concatenate(clips)
    got = _lib.op_gather_frames(samples, table)
    ref = np.concatenate([ref_frames(c, HOP / 48000.0) for c in clips])
    assert got.shape == (counts.sum(), F)
    assert np.array_equal(got, ref)
    assert np.array_equal(got, frames_from_table(samples, table))


# At these batch sizes packing leaves the results bit-equal (measured on MI355X).  At larger batches the solo
# F(4x4,3x3) tail split sums some rows' tiles in channel slices, so packing may change the last bits (profiles/r07_clip_embedding.txt).
CASES = [   # model, pooling, engine batch, db_max_scope, dtype
    ('cnn_L3_melspec2', 'original', 2, 'sample', 'f32'),
    ('cnn_L3_melspec2', 'short', 3, 'sample', 'f32'),
    ('cnn_L3_melspec2', 'original', 3, 'batch', 'f32'),
    ('cnn_L3_melspec1', 'original', 2, 'sample', 'f32'),
    ('cnn_L3_orig', 'original', 3, 'sample', 'f32'),
    ('cnn_L3_melspec2', 'original', 3, 'sample', 'bf16'),
]


@pytest.mark.parametrize('mt,pooling,batch,scope,dtype', CASES)
def test_predict_clips_matches_embed_audio(gpu_required, mt, pooling, batch, scope, dtype):
    P = _mod().perturbed_params(mt, 71)
    m = model.L3Model(mt, db_max_scope=scope)
    m.compute_dtype = dtype
    e = m._ensure_engine(batch)
    e.set_params(P)
    pool = o.AUDIO_POOLING[mt][pooling]
    em = model.EmbeddingModel(m, 'audio', pool)
    clips = _clips(LENGTHS, 2)
    got = em.predict_clips(clips, HOP)
    assert m._engine is e
    for c, g in zip(clips, got):
        ref = e.embed_audio(ref_frames(c, HOP / 48000.0)[:, None, :], pool)
        assert g.shape == ref.shape
        assert np.array_equal(g, ref)


def test_frames_match_oracle(gpu_required):
    mt = 'cnn_L3_melspec2'
    P = _mod().perturbed_params(mt, 51)
    eng = _lib.Engine(mt, 2)
    eng.set_params(P)
    c = _clips([F + 2 * HOP + 5], 3)[0]           # three frames
    table, counts = features.frame_table([len(c)], HOP)
    assert counts.tolist() == [3]
    pool = o.AUDIO_POOLING[mt]['original']
    got = eng.embed_audio_frames(c, table, pool)
    ref = o.embed_audio(mt, P, ref_frames(c, HOP / 48000.0)[:, None, :].astype(np.float64), 'original', np.float64)
    assert got.shape == (3, 6144)
    assert np.abs(got - ref).max() < 2e-3 * max(1.0, np.abs(ref).max())
    eng.close()


def test_get_l3_frames_uniform_end_to_end(gpu_required, tmp_path):
    mt = 'cnn_L3_melspec2'
    m, inputs, out = model.MODELS[mt]()
    m.compile(model.Adam(lr=1e-4), loss='categorical_crossentropy', metrics=['accuracy'])
    v, a, l = o.synthetic_batch(2, seed=81)
    m.train_on_batch([v, a], l)
    path = str(tmp_path / 'model_latest.h5')
    m.save_weights(path)
    emb = model.load_embedding(path, mt, 'audio', 'original')
    x = _clips([120000], 4)[0]                    # 2.5 s
    got = features.get_l3_frames_uniform(x, emb, hop_size=0.1)
    assert got.shape == (16, 6144)                # 1 + 72000 // 4800
    assert np.array_equal(got, emb.predict(ref_frames(x, 0.1)[:, None, :]))
    pcm = np.random.RandomState(5).randint(-20000, 20000, size=(120000, 2)).astype('<i2')
    wav = tmp_path / 'clip.wav'
    with wave.open(str(wav), 'wb') as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(48000)
        w.writeframes(pcm.tobytes())
    got_w = features.get_l3_frames_uniform(str(wav), emb)
    xw = (pcm.astype(np.float32) / 32768).mean(-1)
    assert got_w.shape == (16, 6144)
    assert np.array_equal(got_w, emb.predict(ref_frames(xw, 0.1)[:, None, :]))


def test_embed_audio_frames_rejects_bad_input(gpu_required):
    t = np.array([[0, 0, 10]], np.int64)
    s = np.zeros(10, np.float32)
    tiny = _lib.Engine('tiny_L3', 2)
    with pytest.raises(_lib.L3Error, match='error -1: .*embedding layer'):
        tiny.embed_audio_frames(s, t, (8, 8))
    tiny.close()
    eng = _lib.Engine('cnn_L3_melspec2', 2)
    with pytest.raises(_lib.L3Error, match='error -1: .*hi > n_samples'):
        eng.embed_audio_frames(s, np.array([[0, 0, 11]], np.int64), (8, 8))
    with pytest.raises(_lib.L3Error, match='error -1: .*lo > hi'):
        eng.embed_audio_frames(s, np.array([[0, 5, 4]], np.int64), (8, 8))
    with pytest.raises(_lib.L3Error, match='error -1: .*pooling'):
        eng.embed_audio_frames(s, t, (0, 8))
    out = np.empty((1, 6144), np.float32)
    assert eng.lib.l3_embed_audio_frames(eng.h, None, 10, t.ctypes.data, 1, 8, 8, out.ctypes.data) == -1
    assert b'NULL' in eng.lib.l3_last_error(eng.h)
    eng.close()
    with pytest.raises(_lib.L3Error, match='error -1: .*hi > n_samples'):
        _lib.op_gather_frames(s, np.array([[0, 0, 11]], np.int64))
    with pytest.raises(_lib.L3Error, match='error -1: .*lo > hi'):
        _lib.op_gather_frames(s, np.array([[0, 5, 4]], np.int64))
