"""NumPy float64 oracle of csrc/frames.hip, in the contract's order of operations: per axis the tap ranges and weights of the
antialiased bilinear resize, the horizontal sums first (ascending tap, multiply then add), then the vertical ones, rounding half
up to uint8, and 2 * float32(u / 255) - 1.  Loops run over taps; rows, columns and channels are vectorised (NumPy multiplies and
adds in separate passes, so nothing is fused).  Also the frames the image tests share and their packing into one byte buffer."""
import functools

import numpy as np

from l3embedding_amd import features

SIDE = 224


def axis_taps(n_in, n_out, first, count=SIDE):
    """lo (count,), cnt (count,), w (count, max cnt) float64 (zero past cnt) for outputs [first, first + count) of n_in -> n_out"""
    r = float(n_in) / float(n_out)
    s = max(r, 1.0)
    lo, rows = [], []
    for i in range(first, first + count):
        c = r * (i + 0.5)
        a = max(0, int(c - s + 0.5))
        b = min(n_in, int(c + s + 0.5))
        t = [max(0.0, 1.0 - abs((j - c + 0.5) / s)) for j in range(a, b)]
        total = 0.0
        for v in t:
            total += v
        lo.append(a)
        rows.append([v / total for v in t])
    cnt = np.array([len(x) for x in rows])
    w = np.zeros((count, int(cnt.max())), np.float64)
    for i, x in enumerate(rows):
        w[i, :len(x)] = x
    return np.array(lo), cnt, w


def resize_window(img, Ho, Wo, y0, x0, side=SIDE):
    """Rows [y0, y0 + side) x [x0, x0 + side) of img (H, W, 3) resized to Ho x Wo, before rounding: (side, side, 3) float64"""
    H, W, _ = img.shape
    p = img.astype(np.float64)
    xlo, xcnt, wx = axis_taps(W, Wo, x0, side)
    ylo, ycnt, wy = axis_taps(H, Ho, y0, side)
    h = np.zeros((H, side, 3), np.float64)
    for j in range(wx.shape[1]):
        m = j < xcnt
        prod = wx[m, j][None, :, None] * p[:, xlo[m] + j, :]
        h[:, m, :] = h[:, m, :] + prod
    v = np.zeros((side, side, 3), np.float64)
    for k in range(wy.shape[1]):
        m = k < ycnt
        prod = wy[m, k][:, None, None] * h[ylo[m] + k, :, :]
        v[m] = v[m] + prod
    return v


def to_u8(v):
    return np.clip(np.floor(v + 0.5), 0.0, 255.0).astype(np.uint8)


def to_f32(u8):
    f = (u8.astype(np.float64) / 255.0).astype(np.float32)
    return np.float32(2.0) * f - np.float32(1.0)


def frame_ref(img, row):
    """(u8, f32), each (224, 224, 3), of one frame under its table row {offset, H, W, Ho, Wo, y0, x0}"""
    u8 = to_u8(resize_window(img, int(row[3]), int(row[4]), int(row[5]), int(row[6])))
    return u8, to_f32(u8)


def pack(frames, specs):
    """frames back to back in one uint8 buffer and their table; specs: one (resize, crop) per frame, crop 'center', (y0, x0), or
    'far' for the corner (Ho - 224, Wo - 224)"""
    rows = []
    for f, (resize, crop) in zip(frames, specs):
        t, _ = features.image_table([f.shape[:2]], resize=resize)
        if crop == 'far':
            t[0, 5:7] = t[0, 3:5] - SIDE
        elif crop != 'center':
            t[0, 5:7] = crop
        rows.append(t[0])
    table = np.array(rows, np.int64).reshape(-1, 7)
    sizes = np.array([f.size for f in frames], np.int64)
    table[:, 0] = np.cumsum(sizes) - sizes
    pixels = np.concatenate([f.reshape(-1) for f in frames]) if frames else np.zeros(0, np.uint8)
    return pixels, table


def random_frame(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# The kernel test's frames: (H, W), resize, crop.  Packed back to back the first frame's three bytes make every later offset odd.
KERNEL_CASES = [
    ((1, 1), 256, 'center'),
    ((5, 7), 256, 'center'),
    ((97, 131), 256, 'center'),                  # upscale
    ((224, 224), None, 'center'),
    ((224, 224), 256, 'center'),                 # the half-way cases
    ((256, 341), 256, 'center'),                 # pure crop: the identity returns the source bytes
    ((300, 257), 256, 'center'),                 # scale just above 1
    ((480, 640), 256, 'center'),
    ((720, 1280), 256, 'center'),                # about 10 taps per axis
    ((480, 640), 256, (0, 0)),
    ((720, 1280), 256, 'far'),                   # taps clamped at the border
    ((5, 7), 256, 'far'),
    ((33, 47), 256, 'center'),                   # all 0
    ((300, 257), 256, 'far'),                    # all 255
]


@functools.lru_cache(maxsize=None)
def kernel_case():
    """(frames, pixels, table, want_u8, want_f32) of KERNEL_CASES, computed once per process; callers must not write to them"""
    frames = [random_frame(h, w, 100 + i) for i, ((h, w), _, _) in enumerate(KERNEL_CASES)]
    frames[12][:] = 0
    frames[13][:] = 255
    pixels, table = pack(frames, [(r, c) for _, r, c in KERNEL_CASES])
    refs = [frame_ref(f, row) for f, row in zip(frames, table)]
    out = (frames, pixels, table, np.stack([u for u, _ in refs]), np.stack([f for _, f in refs]))
    for a in out[1:]:
        a.setflags(write=False)
    return out


ENGINE_SHAPES = [(5, 7), (224, 224), (300, 257), (480, 640), (97, 131)]


@functools.lru_cache(maxsize=None)
def engine_case():
    """Five mixed-size frames under the default rule: (frames, pixels, table, want_f32 (5, 224, 224, 3))"""
    frames = [random_frame(h, w, 200 + i) for i, (h, w) in enumerate(ENGINE_SHAPES)]
    pixels, table = pack(frames, [(256, 'center')] * len(frames))
    want = np.stack([frame_ref(f, row)[1] for f, row in zip(frames, table)])
    for a in (pixels, table, want):
        a.setflags(write=False)
    return frames, pixels, table, want
