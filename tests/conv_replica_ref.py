"""The yardstick of the full-chip convolution screen (test_conv_full_chip_gpu.py, test_conv_full_chip_host.py): a batch large enough
to occupy every CU for several rounds of workgroups whose WHOLE output can be checked without a float64 oracle of the whole batch.

The batch is made of scaled copies of three base samples:

    x[r] = 2^k(r) * xb[r % 3],    dy[r] = 2^-k(r) * dyb[r % 3],    k(r) = SCALE_EXPONENTS[r % 7],    bias = 0

3 and 7 are coprime, so the batch holds 21 distinct (base, scale) pairs and no two neighbouring samples hold equal numbers.
Multiplying by a power of two commutes with every rounding of the convolution kernels (bfloat16 operand rounding, fp32
accumulation, the Winograd transforms, the bfloat16 store) as long as nothing overflows or goes denormal -- the ranges here stay
30 binades away from either -- so

    y[r]  == 2^(k(r) - k(r % 3)) * y[r % 3]      bit for bit, every element (forward)
    dx[r] == 2^(k(r % 3) - k(r)) * dx[r % 3]     bit for bit, every element (data gradient)

and only the first three samples need the oracle.  In the weight gradient the scales cancel (x[r] (x) dy[r] = xb (x) dyb), so its
float64 reference is sum_j count_j * dw_j with dw_j the single-sample weight gradient of base j; the bias gradient is the float64
column sum of the dy actually sent.

A failing comparison names where the first difference lies: sample, row, column, channel, and -- given the tiling of the kernel
that wrote the tensor -- the block (patch, flat tile or tile block) and the workgroup it belongs to.  Pure NumPy."""
import collections

import numpy as np

SCALE_EXPONENTS = (0, 2, -3, 1, -2, 3, -1)        # the seven values -3 .. 3, scrambled: neighbours differ by at least 3


def scale_exponents(n):
    """k(r) for r = 0 .. n - 1."""
    return np.array([SCALE_EXPONENTS[r % 7] for r in range(n)], np.int64)


def replica_counts(n):
    """How many of the n samples are copies of base 0, 1, 2."""
    return [len(range(j, n, 3)) for j in range(3)]


def replicate(base, n, sign):
    """(n, ...) from the three bases (3, ...): sample r = 2^(sign * k(r)) * base[r % 3], exact in base's dtype."""
    assert base.shape[0] == 3 and sign in (1, -1)
    out = np.empty((n,) + base.shape[1:], base.dtype)
    k = scale_exponents(n)
    for r in range(n):
        np.multiply(base[r % 3], base.dtype.type(2.0 ** (sign * int(k[r]))), out=out[r])
    return out


def make_batch(xb, dyb, n):
    """x (scales 2^k) and dy (scales 2^-k) of the n-sample batch from the bases xb (3, H, W, Cin) and dyb (3, H, W, Cout)."""
    return replicate(xb, n, 1), replicate(dyb, n, -1)


# A kernel's decomposition of an (N, H, W, C) output into workgroups: tiles of ph x pw pixels in (n, tile row, tile column) order --
# every image padded to whole tiles --, `group` consecutive tiles to a block, a block's channels cut into slices of `bn`:
#   2-D patches of the bf16 halo kernel      Tiling(8, 32, 1, 128 or 64) / Tiling(16, 16, 1, 128 or 64)   block = patch
#   its flat tiles (256 consecutive pixels)  Tiling(1, 1, 256, 128)                                        block = flat tile
#   F(4x4,3x3) (32 tiles of 4 x 4 pixels)    Tiling(4, 4, 32, 64)                                          block = tile block
# workgroup = block * (C / bn) + channel slice: the kernels' logical index, before their remap over the XCDs.
Tiling = collections.namedtuple('Tiling', 'ph pw group bn')


def tiling_blocks(t, n, h, w):
    """Blocks (patches / flat tiles / tile blocks) of an n x h x w output under tiling t."""
    return (n * (-(-h // t.ph)) * (-(-w // t.pw)) + t.group - 1) // t.group


def locate(t, shape, r, row, col, ch):
    """(block, workgroup) of element (r, row, col, ch) of a tensor of `shape` written under tiling t."""
    _, h, w, c = shape
    ty, tx = -(-h // t.ph), -(-w // t.pw)
    block = ((r * ty + row // t.ph) * tx + col // t.pw) // t.group
    return block, block * (c // t.bn) + ch // t.bn


def _first_difference(got, want, first_sample=0, step=1):
    """None if got == want everywhere (NaN counts as a difference), else (count, sample, row, column, channel, got, expected) of
    the first differing element.  got / want: samples first_sample, first_sample + step, ... of an (N, H, W, C) tensor."""
    bad = got != want
    bad |= np.isnan(got) | np.isnan(want)
    count = int(bad.sum())
    if count == 0:
        return None
    i, row, col, ch = (int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
    return count, first_sample + i * step, row, col, ch, float(got[i, row, col, ch]), float(want[i, row, col, ch])


def _report(name, size, shape, diff, tiling):
    count, r, row, col, ch, g, w = diff
    msg = '%s: %d of %d elements differ; first at sample %d row %d column %d channel %d: got %r, expected %r' % (
        name, count, size, r, row, col, ch, g, w)
    if tiling is not None:
        block, wg = locate(tiling, shape, r, row, col, ch)
        msg += ' -- block %d (%dx%d-pixel tiles, %d per block), workgroup %d (%d-channel slices)' % (
            block, tiling.ph, tiling.pw, tiling.group, wg, tiling.bn)
    return msg


def describe_difference(name, got, want, tiling=None):
    """None if the (N, H, W, C) tensors agree in every element, else the failure report: the output's name, how many elements
    differ, and for the first one its sample, row, column, channel, both values, block and workgroup."""
    diff = _first_difference(got, want)
    return None if diff is None else _report(name, got.size, got.shape, diff, tiling)


def replica_difference(name, out, sign, tiling=None):
    """The scaled-replica comparison of an (N, H, W, C) output whose sample r must be 2^(sign * (k(r) - k(r % 3))) times sample
    r % 3, bit for bit: None, or the report of the first difference (as describe_difference) over the whole tensor."""
    n = out.shape[0]
    k = scale_exponents(n)
    diffs = []
    for j in range(min(3, n)):
        rs = np.arange(j, n, 3)
        scale = (2.0 ** (sign * (k[rs] - k[j]))).astype(out.dtype).reshape(-1, 1, 1, 1)
        diff = _first_difference(out[j::3], out[j][None] * scale, first_sample=j, step=3)
        if diff is not None:
            diffs.append(diff)
    if not diffs:
        return None
    first = min(diffs, key=lambda d: d[1:5])
    return _report(name, out.size, out.shape, (sum(d[0] for d in diffs),) + first[1:], tiling)


def unscaled(out, r, sign):
    """Sample r of an output brought back to the scale of sample r % 3 (exact: a power of two), for the every-sample oracle check:
    the same comparison as the replica one with the float64 result of base r % 3 in place of the GPU's."""
    k = SCALE_EXPONENTS[r % 7] - SCALE_EXPONENTS[(r % 3) % 7]
    return out[r] * out.dtype.type(2.0 ** (-sign * k))


def wgrad_reference(dw_single, n):
    """sum_j count_j * dw_j: the float64 weight gradient of the n-sample batch from the single-sample gradients of the bases."""
    counts = replica_counts(n)
    return sum(float(counts[j]) * np.asarray(dw_single[j], np.float64) for j in range(3))


def bias_grad_reference(dy):
    """Float64 column sum of the dy actually sent."""
    return dy.reshape(-1, dy.shape[-1]).sum(axis=0, dtype=np.float64)


# ---- the index arithmetic the flat tiles rest on (conv_bf16_halo.hip fdiv) ---------------------------------------------------------
FDIV_GUARD = 1 << 22          # flat_halo_pixels() refuses flat tiles from this many pixels on


def fdiv(a, b):
    """conv_bf16_halo.hip: int(((float)a + 0.5f) * inv), inv = 1.0f / (float)b -- in float32, truncated."""
    inv = np.float32(1.0) / np.float32(b)
    return ((np.asarray(a).astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


def fdiv_first_failure(b, lo, hi, chunk=1 << 22):
    """Smallest a in [lo, hi) with fdiv(a, b) != a // b, or None."""
    for start in range(lo, hi, chunk):
        a = np.arange(start, min(start + chunk, hi), dtype=np.int32)
        bad = fdiv(a, b) != a // b
        if bad.any():
            return int(a[int(np.argmax(bad))])
    return None


# ---- restated split-K plans of the weight-gradient kernels (what each case prints beside its errors) -------------------------------
def wgrad9_plan(n, h, w, cin, cout, target=512):
    """conv.hip wgrad9_plan + conv_wgrad_bf16.hip conv_wgrad_bf16_tr_launch (bf16-stored operands): split-K slices from the 4x4-pixel
    patch count, then the transpose-read kernel's own 4x16 or 8x8 patches dealt over them.  A stage = one patch of 64 pixels; the
    plan keeps >= 16 4x4 patches = 256 pixels = 4 stages per split."""
    tiles = (cin // 64) * (cout // 64)
    npatch4 = n * ((h + 3) // 4) * ((w + 3) // 4)
    want = -(-target // tiles)
    splits = max(1, min(want, (npatch4 + 15) // 16))
    per4 = -(-npatch4 // splits)
    splits = -(-npatch4 // per4)
    pad4 = ((h + 3) // 4 * 4) * ((w + 15) // 16 * 16)
    pad8 = ((h + 7) // 8 * 8) * ((w + 7) // 8 * 8)
    sq = pad8 < pad4
    npatch = n * (((h + 7) // 8) * ((w + 7) // 8) if sq else ((h + 3) // 4) * ((w + 15) // 16))
    return dict(kernel='wgrad_bf16_tr', patch='8x8' if sq else '4x16', tiles=tiles, splits=splits, blocks=tiles * splits,
                target=target, stages_per_split=-(-npatch // splits), min_stages=4, at_target=want <= (npatch4 + 15) // 16)


def wgw_plan(n, h, w, cin, cout, target=256):
    """conv_wgrad_wino.hip wgw_plan (fp32 operands): units of 8 F(3x3,2x2) tiles (1x8, 2x4 or 4x2, the least padded; ties: the widest),
    one unit per stage, >= 32 stages per split."""
    ty, tx = (h + 1) // 2, (w + 1) // 2
    best, uc = None, 8
    for c in (8, 4, 2):
        ur = 8 // c
        padded = (-(-ty // ur) * ur) * (-(-tx // c) * c)
        if best is None or padded < best:
            best, uc = padded, c
    ur = 8 // uc
    units = n * (-(-ty // ur)) * (-(-tx // uc))
    tiles = (cin // 64) * (cout // 64)
    want = -(-target // tiles)
    splits = max(1, min(want, (units + 31) // 32))
    per = -(-units // splits)
    splits = -(-units // per)
    return dict(kernel='wgrad_wino', patch='%dx%d tiles' % (ur, uc), tiles=tiles, splits=splits, blocks=tiles * splits, target=target,
                stages_per_split=per, min_stages=32, at_target=want <= (units + 31) // 32)


def plan_is_full(p):
    """The kernel splits as far as its block target asks (the cap of its minimum stages per split does not bind; dealing whole
    stages may then leave the grid a few blocks short of the target) and every split runs at least three times that minimum."""
    return p['at_target'] and p['stages_per_split'] >= 3 * p['min_stages']
