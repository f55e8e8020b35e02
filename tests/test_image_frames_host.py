"""Image embeddings from raw frames, the parts that need no GPU: features.image_table's rule (data/avc/sample.py:303-305 and the
centre crop) on known answers, the NumPy oracle of csrc/frames.hip (image_ref.py) against torch's antialiased bilinear
interpolation in float64 and against the identity, the argument errors of EmbeddingModel.predict_images (raised before an engine
is made: there is no GPU here), and the table errors of the C entry point, which precede any device call."""
import numpy as np
import pytest

import image_ref
from l3embedding_amd import _lib, features, model


def test_image_table_known_answers():
    # 480 x 640: scaling 256 / 480, Wo = ceil(341.33) = 342; crop ((256 - 224) // 2, (342 - 224) // 2) = (16, 59)
    # 300 x 257: scaling 256 / 257, Ho = ceil(298.83) = 299, Wo = 256
    t, offs = features.image_table([(480, 640), (300, 257)])
    assert t.dtype == np.int64 and t.shape == (2, 7)
    assert t[0].tolist() == [0, 480, 640, 256, 342, 16, 59]
    assert t[1].tolist() == [3 * 480 * 640, 300, 257, 299, 256, 37, 16]
    assert offs.tolist() == [0, 3 * 480 * 640]
    t, _ = features.image_table([(224, 224)], resize=None)
    assert t[0].tolist() == [0, 224, 224, 224, 224, 0, 0]
    t, _ = features.image_table([(480, 640), (300, 257)], crop=[(32, 118), (0, 0)])
    assert t[:, 5:7].tolist() == [[32, 118], [0, 0]]
    t, offs = features.image_table(np.zeros((0, 2)))
    assert t.shape == (0, 7) and offs.shape == (0,)


def test_image_table_refuses_what_cannot_be_cropped():
    for shape in ((223, 224), (224, 223)):
        with pytest.raises(ValueError, match='frame 1 is %d x %d' % shape):
            features.image_table([(224, 224), shape], resize=None)
    with pytest.raises(ValueError, match='outside'):
        features.image_table([(480, 640)], crop=[(33, 0)])
    with pytest.raises(ValueError, match='outside'):
        features.image_table([(480, 640)], crop=[(0, -1)])
    with pytest.raises(ValueError, match='one .* per frame'):
        features.image_table([(480, 640)], crop=[(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="'center'"):
        features.image_table([(480, 640)], crop='random')
    with pytest.raises(ValueError, match='resize'):
        features.image_table([(480, 640)], resize=223)
    with pytest.raises(ValueError, match='>= 1'):
        features.image_table([(0, 640)])


@pytest.mark.parametrize('shape', [(5, 7), (97, 131), (224, 224), (300, 257), (360, 640), (720, 1280)])
def test_oracle_is_torchs_antialiased_bilinear(shape):
    import torch
    import torch.nn.functional as F
    img = image_ref.random_frame(shape[0], shape[1], 7)
    t, _ = features.image_table([shape])
    _, _, _, Ho, Wo, y0, x0 = t[0].tolist()
    got = image_ref.resize_window(img, Ho, Wo, y0, x0)
    x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    want = F.interpolate(x, size=(Ho, Wo), mode='bilinear', antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    assert np.abs(got - want[y0:y0 + 224, x0:x0 + 224]).max() <= 1e-9


def test_oracle_is_the_identity_at_equal_sizes():
    img = image_ref.random_frame(256, 341, 8)
    lo, cnt, w = image_ref.axis_taps(341, 341, 58)
    assert set(np.unique(w).tolist()) <= {0.0, 1.0} and np.all(w.sum(axis=1) == 1.0)
    v = image_ref.resize_window(img, 256, 341, 16, 58)
    assert np.array_equal(v, img[16:240, 58:282].astype(np.float64))
    u8, f32 = image_ref.frame_ref(img, [0, 256, 341, 256, 341, 16, 58])
    assert np.array_equal(u8, img[16:240, 58:282])
    assert f32.dtype == np.float32 and f32.min() >= -1.0 and f32.max() <= 1.0


def test_predict_images_argument_errors():
    audio = model.EmbeddingModel(model.L3Model('cnn_L3_melspec2'), 'audio', (32, 24))
    with pytest.raises(TypeError, match='vision'):
        audio.predict_images([np.zeros((300, 300, 3), np.uint8)])
    vision = model.EmbeddingModel(model.L3Model('cnn_L3_melspec2'), 'vision', (7, 7))
    with pytest.raises(ValueError, match='uint8'):
        vision.predict_images([np.zeros((300, 300, 3), np.float32)])
    with pytest.raises(ValueError, match='uint8'):
        vision.predict_images(np.zeros((2, 300, 300, 3), np.float32))
    for shape in ((300, 300), (300, 300, 4), (300, 0, 3)):
        with pytest.raises(ValueError, match=r'\(H, W, 3\)'):
            vision.predict_images([np.zeros(shape, np.uint8)])
    with pytest.raises(ValueError, match='shape'):
        vision.predict_images(np.zeros((300, 300, 3), np.uint8))          # one frame is not a sequence of frames
    with pytest.raises(ValueError, match='frame 0 is 223 x 300'):
        vision.predict_images([np.zeros((223, 300, 3), np.uint8)], resize=None)
    with pytest.raises(ValueError, match='outside'):
        vision.predict_images([np.zeros((300, 300, 3), np.uint8)], crop=[(0, 33)])
    assert vision.base._engine is None and audio.base._engine is None          # nothing reached the device


def test_table_errors_precede_the_device():
    lib = _lib.load()
    px = np.zeros(3 * 300 * 300, np.uint8)
    good = [0, 300, 300, 256, 256, 16, 16]

    def rc(row, n_bytes=px.size):
        t = np.array([good, row], np.int64)
        return lib.l3_op_image_frames(0, px.ctypes.data, n_bytes, t.ctypes.data, 2, None, None)

    for col, value, why in ((1, 0, b'H and W'), (2, 8193, b'H and W'), (3, 223, b'Ho and Wo'), (4, 8193, b'Ho and Wo'),
                            (5, -1, b'crop'), (5, 33, b'crop'), (6, 33, b'crop'), (0, -1, b'offset < 0'), (0, 1, b'n_bytes')):
        row = list(good)
        row[col] = value
        assert rc(row) == -1
        msg = lib.l3_last_error(None)
        assert b'l3_op_image_frames: frame 1: ' in msg and why in msg, msg
    assert rc(good, px.size - 1) == -1 and b'frame 0: ' in lib.l3_last_error(None)
    assert lib.l3_op_image_frames(0, None, 0, None, 0, None, None) == -1 and b'NULL' in lib.l3_last_error(None)
    t = np.array([good], np.int64)
    assert lib.l3_op_image_frames(0, px.ctypes.data, px.size, t.ctypes.data, 0, None, None) == 0          # no frames: nothing to do
