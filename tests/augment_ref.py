"""float64 NumPy yardstick of the augmentation tests: what data/avc/sample.py computes for one sample once the frame and the
second have been chosen, with skimage's rgb2hsv / hsv2rgb / img_as_float / img_as_ubyte restated (skimage is not installed
here; nothing below is its text).  Deliberately the LONG way round -- hue, sector, the three hsv2rgb blends -- not the closed
form the kernel uses, so that the closed form is what gets tested.

Shared by tests/test_augment_host.py and tests/test_augment_gpu.py; not a test module itself."""
import numpy as np

CROP = 224


def img_as_float(u8):
    return np.asarray(u8, np.uint8).astype(np.float64) / 255.0


def img_as_ubyte(x):
    """float image in [0, 1] -> uint8: scale, round half to even (np.rint), clip."""
    return np.clip(np.rint(np.asarray(x, np.float64) * 255.0), 0, 255).astype(np.uint8)


def rgb2hsv(rgb):
    rgb = np.asarray(rgb, np.float64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    v = rgb.max(-1)
    delta = v - rgb.min(-1)
    grey = delta == 0
    safe_d = np.where(grey, 1.0, delta)
    s = np.where(grey, 0.0, delta / np.where(v == 0, 1.0, v))
    # the channel holding the maximum names the sector pair; where several do, blue wins over green wins over red
    h = (g - b) / safe_d
    h = np.where(g == v, 2.0 + (b - r) / safe_d, h)
    h = np.where(b == v, 4.0 + (r - g) / safe_d, h)
    h = np.where(grey, 0.0, (h / 6.0) % 1.0)
    return np.stack([h, s, v], -1)


def hsv2rgb(hsv):
    hsv = np.asarray(hsv, np.float64)
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    sector = np.floor(h * 6.0)
    f = h * 6.0 - sector
    p = v * (1.0 - s)
    q = v * (1.0 - f * s)
    t = v * (1.0 - (1.0 - f) * s)
    sector = sector.astype(np.uint8) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.empty(hsv.shape, np.float64)
    for c in range(3):
        out[..., c] = np.choose(sector, [row[c] for row in table])
    return out


def adjust_saturation(rgb, factor):
    """sample.py:24-38 with dtype_limits(float image, clip_negative=True) = (0, 1)."""
    hsv = rgb2hsv(rgb)
    hsv[..., 1] = np.clip(hsv[..., 1] * factor, 0.0, 1.0)
    return hsv2rgb(hsv)


def adjust_brightness(rgb, delta):
    """sample.py:41-56: the float32 delta widened to the image's float64, limits (0, 1)."""
    return np.clip(rgb + np.float64(delta), 0.0, 1.0)


def augment_frame(frame_u8, p):
    """One frame (H, W, 3) uint8 and one parameter row -> (224, 224, 3) uint8: sample.py:169-193, 237-281."""
    x0, y0 = int(p['start_x']), int(p['start_y'])
    x = np.asarray(frame_u8)[x0:x0 + CROP, y0:y0 + CROP, :]
    assert x.shape == (CROP, CROP, 3), x.shape
    x = img_as_float(x)
    if p['flip']:
        x = x[:, ::-1, :]
    if p['sat_first']:
        x = adjust_brightness(adjust_saturation(x, p['saturation']), p['brightness'])
    else:
        x = adjust_saturation(adjust_brightness(x, p['brightness']), p['saturation'])
    return img_as_ubyte(x)


def augment_video(frames_u8, params):
    return np.stack([augment_frame(f, p) for f, p in zip(frames_u8, params)])


def audio_gain(row_i16, u):
    """sample.py:148-156 with random.uniform(a, b) = a + (b - a) * random() spelled out; u = that random()."""
    x = np.asarray(row_i16).astype(float)
    peak = np.abs(x).max()
    max_gain = min(0.1, 32768 / peak - 1) if peak else 0.1
    a, b = -0.1, max_gain
    return 1 + (a + (b - a) * float(u))


def augment_audio(rows_i16, u):
    """(N, T) int16, u (N,) -> (augmented int16 rows, gains): sample.py:146-162."""
    rows_i16 = np.asarray(rows_i16)
    gains = np.array([audio_gain(r, ui) for r, ui in zip(rows_i16, u)], np.float64)
    out = np.empty_like(rows_i16)
    for i, r in enumerate(rows_i16):
        y = r.astype(float)
        y *= gains[i]
        out[i] = y.astype(rows_i16.dtype)
    return out, gains
