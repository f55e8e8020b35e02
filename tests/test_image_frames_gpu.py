"""Image embeddings from raw frames of any size, resized on the GPU (csrc/frames.hip, l3_embed_vision_frames,
EmbeddingModel.predict_images; data/avc/sample.py:286-316, :169-193, train.py:186): the frame kernel alone against the NumPy
float64 oracle of image_ref.py, uint8 and float32 exactly equal; through the engine against l3_embed_vision on the oracle's
frames, bit for bit, to the host and into a device matrix; predict_images; and the argument errors."""
import importlib.util
import os

import numpy as np
import pytest

import image_ref
from l3embedding_amd import _lib, features, model, usc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
MT = 'cnn_L3_melspec2'
POOL = (7, 7)
SENTINEL = np.float32(-1234.5)


def _mod():
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(GOLDEN, 'make_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _engine(mt, batch, dtype='f32'):
    eng = _lib.Engine(mt, batch, dtype=dtype)
    eng.set_params(_mod().perturbed_params(mt, 71))
    return eng


def _embedding(mt, batch, dtype='f32'):
    m = model.L3Model(mt)
    m.compute_dtype = dtype
    m._ensure_engine(batch).set_params(_mod().perturbed_params(mt, 71))
    return model.EmbeddingModel(m, 'vision', POOL)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------
def test_kernel_equals_the_oracle_exactly(gpu_required):
    frames, pixels, table, want_u8, want_f32 = image_ref.kernel_case()
    assert (table[1:, 0] % 2 == 1).any()          # unaligned frames
    u8, f32 = _lib.op_image_frames(pixels, table)
    for i, ((shape, resize, crop), row) in enumerate(zip(image_ref.KERNEL_CASES, table)):
        du = int((u8[i] != want_u8[i]).sum())
        df = int((f32[i] != want_f32[i]).sum())
        print('frame %d %s -> %s at %s: %d uint8 and %d float32 values differ' % (i, shape, tuple(row[3:5].tolist()), tuple(row[5:7].tolist()), du, df))
    assert np.array_equal(u8, want_u8)
    assert np.array_equal(f32, want_f32)
    i = [c[0] for c in image_ref.KERNEL_CASES].index((256, 341))          # the identity: the source bytes
    y0, x0 = table[i, 5:7]
    assert np.array_equal(u8[i], frames[i][y0:y0 + 224, x0:x0 + 224])
    assert np.all(u8[12] == 0) and np.all(f32[12] == -1.0) and np.all(u8[13] == 255) and np.all(f32[13] == 1.0)
    # either output alone
    only_u8, none = _lib.op_image_frames(pixels[:table[2, 0]], table[:2], want_f32=False)
    assert none is None and np.array_equal(only_u8, want_u8[:2])
    none, only_f32 = _lib.op_image_frames(pixels[:table[2, 0]], table[:2], want_u8=False)
    assert none is None and np.array_equal(only_f32, want_f32[:2])


# ---- 2. through the engine --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mt,batch,dtype', [(MT, 2, 'f32'), (MT, 3, 'f32'), ('cnn_L3_orig', 3, 'f32'), (MT, 3, 'bf16')])
def test_engine_rows_equal_embed_vision_on_the_oracles_frames(gpu_required, mt, batch, dtype):
    _, pixels, table, frames_f32 = image_ref.engine_case()
    n = len(table)
    assert n % batch != 0          # a partial last batch
    eng = _engine(mt, batch, dtype)
    want = eng.embed_vision(frames_f32, POOL)
    assert want.shape == (n, 8192) and np.isfinite(want).all() and len(np.unique(want)) > 100
    got = eng.embed_vision_frames(pixels, table, POOL)
    assert np.array_equal(got, want)
    # ... and into a device matrix: the same bits, nothing outside [row0, row0 + n)
    total, row0 = n + 2 * batch + 5, batch + 2
    dst = _lib.Features(np.full((total, want.shape[1]), SENTINEL, np.float32))
    assert eng.embed_vision_frames(pixels, table, POOL, dst=dst, row0=row0) is dst
    rows = dst.download()
    assert np.array_equal(rows[row0:row0 + n], want)
    assert np.all(rows[:row0] == SENTINEL) and np.all(rows[row0 + n:] == SENTINEL)
    dst.close()
    eng.close()


def test_predict_images(gpu_required):
    frames, pixels, table, frames_f32 = image_ref.engine_case()
    em = _embedding(MT, 2)
    want = em.predict(frames_f32)
    got = em.predict_images(frames)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    dev = em.predict_images(frames, to_device=True)
    assert isinstance(dev, usc.DeviceFeatures) and dev.shape == want.shape
    assert np.array_equal(dev.to_host(), want)
    dev.close()
    # calls split at engine-batch boundaries give the same rows
    em.IMAGE_CALL_FRAMES = 2
    assert np.array_equal(em.predict_images(frames), want)
    em.IMAGE_CALL_FRAMES, em.IMAGE_CALL_BYTES = 4096, 1000
    assert np.array_equal(em.predict_images(frames), want)
    # a (T, H, W, 3) array is the list of its frames; explicit crops and no resize reach the table
    clip = np.stack([image_ref.random_frame(230, 250, 300 + i) for i in range(3)])
    crops = [(0, 0), (6, 26), (3, 13)]
    a = em.predict_images(clip, resize=None, crop=crops)
    b = em.predict_images([f for f in clip], resize=None, crop=crops)
    c = em.predict(np.stack([image_ref.to_f32(f[y:y + 224, x:x + 224]) for f, (y, x) in zip(clip, crops)]))
    assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- 3. argument errors -----------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_destination_alone(gpu_required):
    eng = _lib.Engine(MT, 2)
    px = np.zeros(3 * 300 * 300, np.uint8)
    good = [0, 300, 300, 256, 256, 16, 16]
    D = 8192
    dst = _lib.Features(np.full((4, D), SENTINEL, np.float32))
    out = np.full((2, D), SENTINEL, np.float32)
    for col, value, why in ((1, 0, 'H and W'), (1, 8193, 'H and W'), (2, 0, 'H and W'), (2, 8193, 'H and W'),
                            (3, 223, 'Ho and Wo'), (3, 8193, 'Ho and Wo'), (4, 223, 'Ho and Wo'), (4, 8193, 'Ho and Wo'),
                            (5, -1, 'crop'), (5, 33, 'crop'), (6, -1, 'crop'), (6, 33, 'crop'),
                            (0, -1, 'offset < 0'), (0, 1, 'n_bytes')):
        t = np.array([good, good], np.int64)
        t[1, col] = value
        with pytest.raises(_lib.L3Error, match='error -1: l3_embed_vision_frames: frame 1: .*' + why):
            eng.embed_vision_frames(px, t, POOL, out=out)
        with pytest.raises(_lib.L3Error, match='error -1: l3_embed_vision_frames_dev: frame 1: .*' + why):
            eng.embed_vision_frames(px, t, POOL, dst=dst, row0=1)
    with pytest.raises(_lib.L3Error, match='error -1: l3_embed_vision_frames: frame 0: .*n_bytes'):
        eng.embed_vision_frames(px[:-1], np.array([good], np.int64), POOL, out=out[:1])
    with pytest.raises(_lib.L3Error, match='bad pooling size'):
        eng.embed_vision_frames(px, np.array([good], np.int64), (0, 7))
    assert np.all(out == SENTINEL) and np.all(dst.download() == SENTINEL)
    dst.close()
    # the destination: width, rows, and (where there is a second GPU to hold one) device
    t = np.array([good, good], np.int64)
    if eng.lib.l3_device_count() >= 2:
        other = _lib.Features(np.full((4, D), SENTINEL, np.float32), device=1)
        with pytest.raises(_lib.L3Error, match='error -1: l3_embed_vision_frames_dev: dst is on device 1'):
            eng.embed_vision_frames(px, t, POOL, dst=other)
        assert np.all(other.download() == SENTINEL)
        other.close()
    for width, row0, why in ((D + 4, 0, 'columns'), (D, -1, 'outside'), (D, 3, 'outside')):
        bad = _lib.Features(np.full((4, width), SENTINEL, np.float32))
        with pytest.raises(_lib.L3Error, match='error -1: l3_embed_vision_frames_dev: .*' + why):
            eng.embed_vision_frames(px, t, POOL, dst=bad, row0=row0)
        assert np.all(bad.download() == SENTINEL)
        bad.close()
    assert eng.lib.l3_embed_vision_frames_dev(eng.h, px.ctypes.data, px.size, t.ctypes.data, 2, 7, 7, None, 0) == -1
    assert b'dst must not be NULL' in eng.lib.l3_last_error(eng.h)
    assert eng.lib.l3_embed_vision_frames(eng.h, None, px.size, t.ctypes.data, 2, 7, 7, out.ctypes.data) == -1
    assert b'must not be NULL' in eng.lib.l3_last_error(eng.h)
    # no frames: L3_OK and nothing written, in both forms
    ok = _lib.Features(np.full((4, D), SENTINEL, np.float32))
    assert eng.lib.l3_embed_vision_frames(eng.h, px.ctypes.data, px.size, t.ctypes.data, 0, 7, 7, out.ctypes.data) == 0
    assert eng.lib.l3_embed_vision_frames_dev(eng.h, px.ctypes.data, px.size, t.ctypes.data, 0, 7, 7, ok.h, 4) == 0
    assert eng.embed_vision_frames(px[:0], t[:0], POOL).shape == (0, D)
    assert np.all(out == SENTINEL) and np.all(ok.download() == SENTINEL)
    ok.close()
    tiny = _lib.Engine('tiny_L3', 2)
    with pytest.raises(_lib.L3Error, match='no embedding layer'):
        tiny.embed_vision_frames(px, t, POOL)
    tiny.close()
    eng.close()
