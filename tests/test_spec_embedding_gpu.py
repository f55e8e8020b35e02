"""The minispec front-end, spectrograms out and in, the 199-frame linear tower and the OpenL3 files on the GPU.

The front-end is compared with tests/minispec_ref.py (float64) in the power domain, relative to the second's largest value, under
the project's LIN_BOUND; its float32 NumPy restatement measures 0.6e-6 ... 2.1e-6 on noise and tones (test_spec_embedding_host).
Spectrograms out and in are bit-for-bit statements.  The distances measured on MI355X are in profiles/r31_spec_embedding.txt; every
test prints its own as `SPEC <what> <value>`.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest

import minispec_ref as R
import test_embedding_parity_gpu as E
import test_layer_parity_gpu as LP
from frontend_ref import CONTROL_MARGIN, LIN_BOUND
from l3embedding_amd import _lib, features, model, openl3
from oracle import l3_oracle as o

pytestmark = pytest.mark.gpu

SR = 48000
MODELS = ('cnn_L3_melspec2', 'cnn_L3_melspec1', 'cnn_L3_kapredbinputbn')
NAMES, AUDIO = R.signals()
EINVAL = -1                 # include/l3hip.h L3_EINVAL
DB_BOUND = 5e-3             # test_frontend's bound on the dB values of noise
_REF = {}


def _ref(mt, variant=None):
    """float64 reference of the six signals, once per (model, variant)"""
    if (mt, variant) not in _REF:
        _REF[(mt, variant)] = R.minispec(mt, AUDIO[:2] if variant else AUDIO, variant=variant)
    return _REF[(mt, variant)]


def _frontend_case(mt, mode, monkeypatch):
    if mode is None:
        monkeypatch.delenv('L3_DFT_FACTORED', raising=False)
    else:
        monkeypatch.setenv('L3_DFT_FACTORED', mode)
    got = _lib.op_frontend_form(mt, AUDIO, 'minispec')
    ref = _ref(mt)
    assert got.shape == ref.shape and got.shape[2] == 199
    d = R.lin_d(got, ref)
    for k, v in zip(NAMES, d):
        print('SPEC frontend %s path=%s %s lin %.3g' % (mt, mode, k, v))
    assert d.max() < LIN_BOUND, dict(zip(NAMES, d))
    ddb = float(np.abs(got[0] - ref[0]).max())
    print('SPEC frontend %s path=%s noise dB %.3g' % (mt, mode, ddb))
    if R.MODELS[mt][1]:             # the linear model: float32 NumPy is itself 1.5e-2 away near the -80 floor
        assert ddb < DB_BOUND
    assert np.all(got[NAMES.index('silence')] == 0.0)
    mx = got.reshape(len(NAMES), -1).max(axis=1)
    assert np.all(mx == 0.0) and got.min() >= -80.0
    # controls: the reference altered to kapre's meaning must be far from what the GPU returned
    for variant in ('kapre_pad', 'mel_of_power', 'unsquared'):
        if variant == 'mel_of_power' and not R.MODELS[mt][1]:
            continue
        dc = R.lin_d(got[:2], _ref(mt, variant))
        print('SPEC control %s path=%s %s %.3g' % (mt, mode, variant, dc.min()))
        assert dc.min() > CONTROL_MARGIN * LIN_BOUND, (variant, dc)
    return got


@pytest.mark.parametrize('mt', MODELS)
def test_minispec_frontend_against_float64(gpu_required, mt, monkeypatch):
    """The product path of each model: the one fused kernel for the mel models, the 512-point GEMM for the linear one."""
    got = _frontend_case(mt, None, monkeypatch)
    kap = _lib.op_frontend(mt, AUDIO[:2, None, :])
    assert kap.shape[2] == (199 if R.MODELS[mt][1] else 197)           # the kapre form keeps its own geometry
    assert not np.array_equal(kap[..., :197, :], got[:2, :, :197, :])


@pytest.mark.parametrize('mode', ['2', '0'])
@pytest.mark.parametrize('mt', MODELS[:2])
def test_minispec_mel_kernels_on_the_gemm_paths(gpu_required, mt, mode, monkeypatch):
    """spec_to_features in the magnitude form: behind the two-GEMM factored transform (2) and behind the full GEMM (0); both are
    other kernels than the fused one, so their bits differ from it."""
    got = _frontend_case(mt, mode, monkeypatch)
    monkeypatch.delenv('L3_DFT_FACTORED')
    fused = _lib.op_frontend_form(mt, AUDIO[:1], 'minispec')
    assert not np.array_equal(fused, got[:1])


@pytest.mark.parametrize('mt', MODELS)
def test_minispec_follows_edited_dft_kernels(gpu_required, mt):
    """A model whose stored DFT kernels were edited: the bins 100..199 doubled.  The engine must follow the kernels it holds."""
    n_fft = R.MODELS[mt][0]
    real, imag = o.stft_kernels(n_fft)
    real = real.copy()
    real[:, 100:200] *= 2.0
    ref = R.minispec(mt, AUDIO[:2], kernels=(real, imag))
    eng = _lib.Engine(mt, 2, seed=0, frontend='minispec')
    name = [n for n, _, _ in eng.param_table() if n.endswith('/real_kernels')][0]
    eng.set_param(name, real.reshape(n_fft, 1, 1, -1))
    got = eng.audio_spectrograms(AUDIO[:2].reshape(-1), features.frame_table([SR, SR], SR)[0])[..., None]
    eng.close()
    d = R.lin_d(got, ref)
    print('SPEC edited-kernels %s lin %.3g %.3g' % (mt, d[0], d[1]))
    assert d.max() < LIN_BOUND
    # the edit is visible at all: on the noise (the tones have next to nothing in the edited bins)
    assert R.lin_d(got, _ref(mt)[:2])[0] > CONTROL_MARGIN * LIN_BOUND


def _five_frames():
    """two clips back to back, five whole seconds: a full and a partial last batch at engine batches 2 and 3"""
    r = np.random.RandomState(5)
    t = np.arange(2 * SR + 100) / float(SR)
    clips = [(0.4 * np.sin(2 * np.pi * 523 * t) + 0.05 * r.randn(t.size)).astype(np.float32), r.uniform(-1, 1, 3 * SR).astype(np.float32)]
    table, counts = openl3.frame_table([c.size for c in clips])
    assert counts.tolist() == [2, 3]
    return clips, table


@pytest.mark.parametrize('B', [2, 3])
@pytest.mark.parametrize('mt', ['cnn_L3_melspec2', 'cnn_L3_kapredbinputbn'])
def test_kapre_spectrograms_out_and_in_are_bit_equal(gpu_required, mt, B):
    clips, table = _five_frames()
    x = np.concatenate(clips)
    e = _lib.Engine(mt, B, seed=4)
    F, frames = e.spectrogram_shape()
    assert (F, frames) == {'cnn_L3_melspec2': (256, 199), 'cnn_L3_kapredbinputbn': (257, 197)}[mt]
    spec = e.audio_spectrograms(x, table)
    assert spec.shape == (5, F, frames)
    fr = _lib.op_gather_frames(x, table)
    assert np.array_equal(spec[:2][..., None], _lib.op_frontend(mt, fr[:2, None, :]))
    for pool in o.AUDIO_POOLING[mt].values():
        direct = e.embed_audio_frames(x, table, pool)
        again = e.embed_audio_spec(spec, pool)
        assert np.array_equal(direct, again)
        assert np.array_equal(e.embed_audio_spec(spec[..., None], pool), direct)
        # the device form: rows 1..5 of a 7-row matrix, the canaries in rows 0 and 6 untouched
        canary = np.full((7, direct.shape[1]), -7.25, np.float32)
        dst = _lib.Features(canary)
        e.embed_audio_spec(spec, pool, dst=dst, row0=1)
        got = dst.download()
        dst.close()
        assert np.array_equal(got[1:6], direct) and np.all(got[0] == -7.25) and np.all(got[6] == -7.25)
    e.close()


@pytest.mark.parametrize('B', [2, 3])
@pytest.mark.parametrize('mt', MODELS)
def test_minispec_model_spectrograms_then_predict_equals_predict_clips(gpu_required, mt, B):
    clips, table = _five_frames()
    m = model.L3Model(mt, seed=6, frontend='minispec')
    em = model.EmbeddingModel(m, 'audio', o.AUDIO_POOLING[mt]['original'])
    rows = em.predict_clips(clips, SR, batch_size=B)
    assert m._engine.batch == B and m._engine.frontend == 'minispec'
    spec, counts = em.spectrograms(clips, SR, batch_size=B)
    assert counts.tolist() == [2, 3] and spec.shape == (5, R.MODELS[mt][1] or 257, 199, 1)
    assert np.array_equal(em.predict_spectrograms(spec, batch_size=B), np.concatenate(rows))
    assert np.array_equal(em.predict_spectrograms(spec[..., 0]), np.concatenate(rows))
    dev = em.predict_spectrograms(spec, to_device=True)
    assert np.array_equal(dev.to_host(), np.concatenate(rows))
    dev.close()
    # the spectrogram is the oracle's
    d = R.lin_d(spec, R.minispec(mt, _lib.op_gather_frames(np.concatenate(clips), table)))
    print('SPEC spectrograms %s B=%d lin %.3g' % (mt, B, d.max()))
    assert d.max() < LIN_BOUND
    m._drop_engines()


def test_geometry_of_the_three_minispec_engines(gpu_required):
    """199 frames for all three; the pooled widths stay (32, 24, 512), so l3_embed_dim and the pooling table are unchanged"""
    for mt in MODELS:
        e = _lib.Engine(mt, 1, frontend='minispec')
        k = _lib.Engine(mt, 1)
        assert e.spectrogram_shape() == (R.MODELS[mt][1] or 257, 199)
        n = C.c_int64()
        _lib.check(e.lib.l3_activation_numel(e.h, b'audio_model/audio_embedding_layer', C.byref(n)), e.h)
        h, w, c = model.AUDIO_EMBEDDING_MAP[mt]
        assert n.value == h * w * c
        for pool in o.AUDIO_POOLING[mt].values():
            assert e.lib.l3_embed_dim(e.h, 0, pool[0], pool[1]) == k.lib.l3_embed_dim(k.h, 0, pool[0], pool[1])
        assert sorted(e.lib.l3_embed_dim(e.h, 0, *p) for p in o.AUDIO_POOLING[mt].values()) == [512, 6144]
        assert [(a, tuple(b), c_) for a, b, c_ in e.param_table()] == [(a, tuple(b), c_) for a, b, c_ in k.param_table()]
        e.close()
        k.close()


def test_linear_tower_at_199_frames_against_float64(gpu_required):
    """cnn_L3_kapredbinputbn on the 257 x 199 input: minispec_ref, then the oracle's audio tower, judged by the rule and bounds of
    test_embedding_parity_gpu's other audio models, its float32 NumPy run the yardstick."""
    mt = 'cnn_L3_kapredbinputbn'
    names = ('noise', 'tone')
    P = E._mod().perturbed_params(mt, E.PARAM_SEED)
    a = np.stack([E.SIGNALS[k] for k in names])
    m64 = R.tower_embedding_map(mt, P, R.minispec(mt, a), np.float64)
    m32 = R.tower_embedding_map(mt, P, R.minispec(mt, a, np.float32), np.float32)
    assert m64.shape[1:] == (32, 24, 512)
    eng = _lib.Engine(mt, 2, frontend='minispec')
    eng.set_params(P)
    bad = []
    for pooling, pool in o.AUDIO_POOLING[mt].items():
        got = eng.embed_audio(a[:, None, :], pool)
        r64, r32 = o.pool_embedding(m64, pool), o.pool_embedding(m32, pool)
        bad += E._check('SPEC tower199 %s %-8s' % (mt, pooling), E.FP32_BOUND[mt], {k: got[i:i + 1] for i, k in enumerate(names)},
                        {k: r64[i] for i, k in enumerate(names)}, {k: r32[i] for i, k in enumerate(names)})
    eng.close()
    assert bad == []


@pytest.mark.parametrize('case', [('S.conv1a', 257, 199, 1, 64), ('S.conv1b', 257, 199, 64, 64), ('S.conv2a', 128, 99, 64, 128),
                                  ('S.conv2b', 128, 99, 128, 128)], ids=lambda c: c[0])
def test_first_two_blocks_convolutions_at_the_199_frame_geometry(gpu_required, case):
    """conv1 and conv2 of the linear spec model alone, 257 x 199 and 128 x 99, against the float64 direct convolution at
    test_layer_parity_gpu's bounds"""
    tag, h, w, ci, co = case
    x, wt, b, _ = LP._layer_data(*case)
    ref = o.conv2d_fwd(x.astype(np.float64), wt.astype(np.float64), b.astype(np.float64), 'same')
    y = _lib.op_conv2d_fwd(x, wt, b, True)
    err = LP.relerr(y, ref)
    print('SPEC conv %s %dx%d %d->%d y %.3g' % (tag, h, w, ci, co, err))
    assert err < (LP.TOL_F4 if ci >= LP.F4_MIN_CIN else LP.TOL)


# ---- refusals and compatibility ------------------------------------------------------------------------------------------------------
def _create(mt, frontend, db_max_scope=0, size=None):
    cfg = _lib.L3Config2()
    cfg.struct_size = C.sizeof(_lib.L3Config2) if size is None else size
    cfg.model_type = _lib.MODEL_IDS[mt]
    cfg.batch = 1
    cfg.db_max_scope = db_max_scope
    cfg.bn_zero_debias = 1
    cfg.frontend = frontend
    h = C.c_void_p()
    rc = _lib.load().l3_create(C.byref(cfg), 1, C.byref(h))
    msg = _lib.load().l3_last_error(None)
    return rc, h, (msg.decode() if msg else '')


def test_create_refusals_and_the_old_struct_size(gpu_required):
    lib = _lib.load()
    for mt in ('cnn_L3_orig', 'tiny_L3'):
        rc, h, msg = _create(mt, 1)
        assert rc == EINVAL and not h.value and 'L3_FRONTEND_MINISPEC' in msg and 'cnn_L3_melspec1' in msg
    rc, h, msg = _create('cnn_L3_melspec2', 1, db_max_scope=1)
    assert rc == EINVAL and not h.value and 'db_max_scope' in msg
    rc, h, msg = _create('cnn_L3_melspec2', 2)
    assert rc == EINVAL and not h.value and 'frontend' in msg
    with pytest.raises(ValueError):
        _lib.Engine('cnn_L3_melspec2', 1, frontend='librosa')
    # a caller compiled against the header before `frontend`: the struct ends where the field begins, and whatever lies behind
    # it is not read
    old = _lib.L3Config2.frontend.offset
    assert old == C.sizeof(_lib.L3Config) == C.sizeof(_lib.L3Config2) - 8
    rc, h, msg = _create('cnn_L3_kapredbinputbn', 1, size=old)
    assert rc == 0 and h.value
    r, f = C.c_int64(), C.c_int64()
    assert lib.l3_spectrogram_shape(h, C.byref(r), C.byref(f)) == 0 and (r.value, f.value) == (257, 197)
    lib.l3_destroy(h)
    rc, h, msg = _create('cnn_L3_kapredbinputbn', 0, size=old - 4)
    assert rc == EINVAL and 'struct_size' in msg


def test_a_minispec_engine_refuses_training_and_infers(gpu_required):
    mt = 'cnn_L3_melspec1'
    v, a, l = o.synthetic_batch(1, seed=3)
    e = _lib.Engine(mt, 1, frontend='minispec')
    before = e.get_params()

    def refused(fn, *args):
        with pytest.raises(_lib.L3Error) as info:
            fn(*args)
        assert 'inference' in str(info.value) and 'L3_FRONTEND_MINISPEC' in str(info.value), str(info.value)

    refused(e.train_step, v, a, l, 1e-3)
    e.upload_batch(v, a, l)
    refused(e.step_forward, True)
    refused(e.step_resident, 1e-3)
    refused(e.step_backward_bucket, 0)
    refused(e.step_update, 1e-3)
    refused(e.step_replicas, 1e-3)
    refused(e.step_dp, 1e-3)
    refused(e.tower_step, 'audio', True)
    after = e.get_params()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # inference works: forward, the activation tap, the embed calls
    probs, logits = e.forward(v, a, training=False)
    assert np.isfinite(probs).all()
    fe = e.activation('audio_model/frontend')
    assert fe.size == 128 * 199
    assert np.array_equal(fe.reshape(1, 128, 199, 1), _lib.op_frontend_form(mt, a[:, 0, :], 'minispec'))
    e.step_forward(False)
    e.close()


def test_spec_entry_argument_errors_leave_outputs_untouched(gpu_required):
    mt = 'cnn_L3_melspec1'
    e = _lib.Engine(mt, 2)
    lib, D = e.lib, 6144
    spec = np.zeros((3, 128, 199), np.float32)
    out = np.full((3, D), -7.25, np.float32)
    msg = lambda: lib.l3_last_error(e.h).decode()
    assert lib.l3_embed_audio_spec(e.h, None, 3, 4, 8, _lib._ptr(out)) == EINVAL and 'NULL' in msg()
    assert lib.l3_embed_audio_spec(e.h, _lib._ptr(spec), 3, 4, 8, None) == EINVAL and 'NULL' in msg()
    assert lib.l3_embed_audio_spec(e.h, _lib._ptr(spec), -1, 4, 8, _lib._ptr(out)) == EINVAL
    assert lib.l3_embed_audio_spec(e.h, _lib._ptr(spec), 3, 0, 8, _lib._ptr(out)) == EINVAL and 'pooling' in msg()
    assert lib.l3_embed_audio_spec(e.h, _lib._ptr(spec), 0, 4, 8, _lib._ptr(out)) == 0
    assert np.all(out == -7.25)
    dst = _lib.Features(np.full((4, D), -7.25, np.float32))
    narrow = _lib.Features(np.full((4, 512), -7.25, np.float32))
    assert lib.l3_embed_audio_spec_dev(e.h, _lib._ptr(spec), 3, 4, 8, dst.h, 2) == EINVAL and 'rows' in msg()
    assert lib.l3_embed_audio_spec_dev(e.h, _lib._ptr(spec), 3, 4, 8, dst.h, -1) == EINVAL
    assert lib.l3_embed_audio_spec_dev(e.h, _lib._ptr(spec), 3, 4, 8, narrow.h, 0) == EINVAL and 'columns' in msg()
    assert lib.l3_embed_audio_spec_dev(e.h, _lib._ptr(spec), 3, 4, 8, None, 0) == EINVAL
    assert np.all(dst.download() == -7.25) and np.all(narrow.download() == -7.25)
    dst.close()
    narrow.close()
    with pytest.raises(ValueError):
        e.embed_audio_spec(np.zeros((1, 128, 197), np.float32), (4, 8))
    # l3_audio_spectrograms: the table's validation is l3_embed_audio_frames'
    x = np.zeros(SR, np.float32)
    sp = np.full((1, 128, 199), -7.25, np.float32)
    bad = np.array([[0, 0, SR + 1]], np.int64)
    assert lib.l3_audio_spectrograms(e.h, _lib._ptr(x), SR, _lib._ptr(bad), 1, _lib._ptr(sp)) == EINVAL and 'frame 0' in msg()
    assert lib.l3_audio_spectrograms(e.h, None, SR, _lib._ptr(bad), 1, _lib._ptr(sp)) == EINVAL
    assert np.all(sp == -7.25)
    e.close()


# SHA-256 of a kapre engine's front-end output and of one embedding on a fixed seed, taken from the commit before the front-end
# form existed: the kapre form computes the same bits
KAPRE_FRONTEND_SHA256 = '3d60acea0239869c4977b0b9643678b5a020e38ab671490abda8a708ef2b6950'
KAPRE_EMBEDDING_SHA256 = '03667e571bbfc1a157a5af1f1e8b34d42bebf6d1a4a1daded3ce7ea8f05c4bd5'


def kapre_pins():
    a = o.synthetic_batch(2, seed=9)[1]
    fe = _lib.op_frontend('cnn_L3_melspec2', a)
    e = _lib.Engine('cnn_L3_melspec2', 2, seed=0)
    emb = e.embed_audio(a, (8, 8))
    e.close()
    return hashlib.sha256(np.ascontiguousarray(fe).tobytes()).hexdigest(), hashlib.sha256(np.ascontiguousarray(emb).tobytes()).hexdigest()


def test_the_kapre_form_computes_the_bits_it_computed_before(gpu_required):
    fe, emb = kapre_pins()
    print('SPEC pins', fe, emb)
    assert fe == KAPRE_FRONTEND_SHA256 and emb == KAPRE_EMBEDDING_SHA256


def test_load_embedding_with_the_minispec_frontend(gpu_required, tmp_path):
    """model.load_embedding(..., frontend='minispec'): the file's weights on an engine of the other form"""
    mt = 'cnn_L3_melspec1'
    P = E._mod().perturbed_params(mt, E.PARAM_SEED)
    src = model.L3Model(mt)
    src._assign(P)
    path = str(tmp_path / 'model_latest.h5')
    src.save_weights(path)
    clips, _ = _five_frames()
    em = model.load_embedding(path, mt, 'audio', 'short', frontend='minispec')
    assert em.base.frontend == 'minispec' and em.pool == (16, 24)
    got = np.concatenate(em.predict_clips(clips[:1], SR, batch_size=2))
    direct = model.L3Model(mt, frontend='minispec')
    direct._assign(P)
    want = np.concatenate(model.EmbeddingModel(direct, 'audio', (16, 24)).predict_clips(clips[:1], SR, batch_size=2))
    assert np.array_equal(got, want)
    kap = np.concatenate(model.load_embedding(path, mt, 'audio', 'short').predict_clips(clips[:1], SR, batch_size=2))
    assert not np.array_equal(kap, got)
    for m in (em.base, direct):
        m._drop_engines()


# ---- the OpenL3 files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mt', MODELS)
def test_extract_then_load_returns_every_tower_parameter(gpu_required, tmp_path, mt):
    P = E._mod().perturbed_params(mt, E.PARAM_SEED)
    m = model.L3Model(mt)
    m._assign(P)
    paths = openl3.extract_models(m, mt, 'music', str(tmp_path))
    r = openl3.repr_of(mt)
    fe_layer = [n for n in P if n.endswith('/real_kernels')][0].split('/')[1]
    clips, table = _five_frames()
    want = None
    for kind, frontend in (('audio', 'kapre'), ('spec', 'kapre'), ('spec', 'minispec')):
        em = openl3.load_audio_embedding(paths[kind], r, 6144, frontend=frontend)
        got = em.base._weights_dict()
        for k, v in P.items():
            if k.startswith('audio_model/') and (kind == 'audio' or k.split('/')[1] != fe_layer):
                assert np.array_equal(got[k], v), k
        assert em.pool == o.AUDIO_POOLING[mt]['original'] and em.base.frontend == frontend
        if frontend == 'kapre':         # perturbed_params leaves the constants stock, so the spec file gives the same embedding
            rows = np.concatenate(em.predict_clips(clips[:1], SR, batch_size=2))
            want = rows if want is None else want
            assert np.array_equal(rows, want)
        else:
            assert em.base._ensure_engine(1).spectrogram_shape()[1] == 199
        em.base._drop_engines()
    em = openl3.load_image_embedding(paths['image'], r, 8192)
    got = em.base._weights_dict()
    assert all(np.array_equal(got[k], v) for k, v in P.items() if k.startswith('vision_model/'))
    assert em.pool == (7, 7) and em.embedding_type == 'vision'
    em.base._drop_engines()
    with pytest.raises(ValueError):
        openl3.load_audio_embedding(paths['audio'], r, 1024)
    with pytest.raises(ValueError):
        openl3.load_audio_embedding(paths['image'], r, 512)
