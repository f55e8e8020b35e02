"""The yardstick of the audio front-end's kernels one by one (test_frontend_stages_gpu.py, test_frontend_stages_host.py): the
float64 reference of every stage of csrc/frontend.hip, the cases, the bounds and the controls.

  frame_audio / frame_audio_folded / dft_pack_frames   frames_of(), folded32(), packed32(): float32 NumPy, bit for bit -- a copy, one
                                                       add or subtract, one multiply by the library's window
  dft_twiddle                                          twiddle_ratios(): float64 arithmetic on the float32 y and table
  the 2048-point transform                             staged_dft(): the factorisation the kernels use, written out in float64 --
        n = 64 n1 + n2;  Y[n2][k1] = sum_n1 xw[n] W32^(n1 k1);  Z[k1][n2] = Y[n2][k1] exp(-2 pi i n2 k1 / 2048);
        X[k1 + 32 k2] = sum_n2 Z[k1][n2] W64^(n2 k2), k2 < 32;  X[1024] = sum_n2 (-1)^n2 Y[n2][0]
  spec_to_features                                     spec_layout(), power_of(), features(): mel product, sqrt, dB, log
  dft_fused                                            fused64(): float64 rfft of the float32 frame times the float32 window
  db_normalize                                         db_normalize32(): float32 NumPy maximum(x - max, -80), bit for bit

Every criterion is an error / bound ratio (<= 1 passes), printed as `FESTAGE <kernel> <case> <criterion> <error / bound>`;
profiles/r30_frontend_stage_bounds.txt keeps the worst of each.  The bounds:

  tables           2^-24 absolute: half an ulp at 1 (every entry is a cosine, a sine or a Hann weight) with room for the cast
  dft_twiddle      a2: 2^-23 (|yr co| + |yi si|) -- a product rounded, then a fused multiply-add rounded;
                   nyq: 8 x 2^-24 sum |Y[n2][0]| -- one add per lane and six shuffle levels
  linear features  (mel_len + 3) 2^-24 ref: re^2 + im^2 is two roundings, every tap of the band one more, and all terms are >= 0
  flags            the project's yardstick (test_embedding_parity_gpu.py): d = max |got - ref64| / max |ref64| over the case at most
                   K_D32 times d32, the same distance of the float32 NumPy restatement, with a floor of one fp32 ulp (2^-23) of the result
  dft_fused        d = max |got - ref| / max ref per row <= LIN_BOUND, the project's linear-domain bound of the front-end
  engine           2e-5 of the peak in the linear domain, test_frontend's tone bound
A control alters the REFERENCE; the case named for it must put the GPU more than CONTROL_MARGIN bounds away from the altered one.
"""
import functools

import numpy as np

from oracle import l3_oracle as o

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
N, N1, N2, NB = 2048, 32, 64, 1025
LIN_BOUND = 6e-6            # test_embedding_parity_gpu.LIN_BOUND.  dft_fused measured on MI355X: 1.55e-6 on the tone sweep (the float32
                            # GEMM restatement in NumPy: 1.07e-6), 9.1e-7 beyond one trip, 7.2e-7 / 6.8e-7 / 3.1e-7 with the 256- / 128- /
                            # 70-filter banks, <= 4.7e-7 on the padded edges and the ragged workgroups
K_D32 = 7.0                 # test_embedding_parity_gpu.K_D32.  Measured d / d32: sqrt_out 6.4e-8 / 8.5e-8, db 1.2e-7 / 7.6e-8,
                            # loglambda 1.7e-7 / 7.1e-8, sqrt_out + db 1.7e-7 / 9.5e-8: at most 0.20 of the rule (the floor decides)
ULP32 = 2.0 ** -23          # the floor of the K_D32 rule: one fp32 ulp of the result
CONTROL_MARGIN = 10.0
ENGINE_BOUND = 2e-5         # test_parity_gpu.test_frontend: tones, of the peak, linear domain.  Measured: 1.1e-6 (fused), 1.0e-6 (two
                            # GEMMs), 1.5e-6 (full GEMM); fused against the full GEMM 1.8e-6
TABLE_BOUND = U24           # measured: 0.4999 of it (tw), i.e. every entry is the correctly rounded float
LN10_32 = F32(2.302585092994046)
DB_FLOOR32 = F32(-100.0)                           # 10 log10(1e-10)
LOG_FLOOR32 = F32(np.log(F64(F32(1e-12)))) / F32(5)   # log(1e-12) / 5, each step rounded to float32

# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (B, T, n_dft, hop, pad_left, frames)
FRAME_CASES = [
    (2, 3000, 2048, 242, 976, 13),        # 'same' padding
    (3, 500, 2048, 242, 1016, 3),         # left and right padding inside one frame
    (1, 1, 2048, 242, 1023, 1),           # a single sample
    (2, 1500, 512, 242, 0, 5),            # 'valid' framing
    (2, 2600, 512, 240, 0, 9),            # the tiny model's hop
    (1, 6000, 512, 700, 0, 8),            # hop > n_dft
    (1, 19632, 2048, 16, 0, 1100),        # past the 8192-block cap of the grid-stride kernels
]
EDGE_CASES = FRAME_CASES[:3]              # the 2048-point ones with padding: dft_fused's clamped loads
# (T, n_dft, hop, same) of frontend_cfg against oracle.tf_same_pad / frame_signal: the models' and the cases above that are either
CFG_CASES = [(48000, 2048, 242, True), (48000, 512, 242, False), (48000, 512, 240, False), (3000, 2048, 242, True),
             (500, 2048, 242, True), (1, 2048, 242, True), (1500, 512, 242, False), (2600, 512, 240, False), (6000, 512, 700, False),
             (19632, 2048, 16, False), (2048, 2048, 16, True), (4097, 512, 512, True)]
TWIDDLE_FRAMES = (1, 3, 300)
SPEC_ROWS = (1, 3, 13)
FLAG_SETS = [dict(sqrt_out=True), dict(db=True), dict(loglambda=True), dict(sqrt_out=True, db=True)]
# (B, per_sample) of db_normalize; (300, 3500) is more than 4096 x 256 elements and B > 256 for batch_max
DB_CASES = [(1, 1), (3, 255), (2, 257), (300, 3500)]


def tag(case):
    return 'x'.join(map(str, case))


def flag_tag(fl):
    return '+'.join(k for k in ('sqrt_out', 'db', 'loglambda') if fl.get(k)) or 'linear'


def rng_of(*key):
    return np.random.default_rng([20240911] + [int(k) for k in key])


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _ratio(err, bound):
    """max err / bound, an exact 0 / 0 counting as 0."""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- tables ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables64():
    """win (2048), b1 (32, 64), b2 (128, 64), tw (64, 32, 2) in float64, laid out as the library's."""
    n = np.arange(N, dtype=F64)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / N)
    a1 = 2 * np.pi * np.outer(np.arange(N1), np.arange(N1)) / N1
    b1 = np.concatenate([np.cos(a1), -np.sin(a1)], axis=1)
    a2 = 2 * np.pi * np.outer(np.arange(N2), np.arange(N2 // 2)) / N2
    b2 = np.concatenate([np.concatenate([np.cos(a2), -np.sin(a2)], axis=1), np.concatenate([np.sin(a2), np.cos(a2)], axis=1)], axis=0)
    at = 2 * np.pi * np.outer(np.arange(N2), np.arange(N1)) / N
    tw = np.stack([np.cos(at), np.sin(at)], axis=-1)
    return dict(win=_ro(win), b1=_ro(b1), b2=_ro(b2), tw=_ro(tw))


def window64(n_dft):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_dft, dtype=F64) / n_dft)


def pack_bands(fb):
    """The first-to-last-nonzero packing of fb (nb, F): start, len, off (int32) and the weights (fb's dtype)."""
    fb = np.asarray(fb)
    st, ln, of, w = [], [], [], []
    for q in range(fb.shape[1]):
        nz = np.flatnonzero(fb[:, q])
        s, l = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        st.append(s), ln.append(l), of.append(sum(ln[:-1]))
        w.append(fb[s:s + l, q])
    return np.array(st, np.int32), np.array(ln, np.int32), np.array(of, np.int32), np.concatenate(w) if w else np.zeros(0, fb.dtype)


def banded_product(pw, bands):
    """pw (rows, nb) times the packed bands, tap by tap in band order: (rows, F)."""
    st, ln, of, w = bands
    out = np.zeros((pw.shape[0], len(st)), pw.dtype)
    for q in range(len(st)):
        for i in range(int(ln[q])):
            out[:, q] += pw[:, st[q] + i] * w[of[q] + i]
    return out


@functools.lru_cache(maxsize=None)
def stock_bank(n_mels, n_dft=N):
    """kapre's freq2mel (nb, n_mels) in float32, as oracle.frontend_constants holds it."""
    return _ro(np.ascontiguousarray(o.mel_basis(48000, n_dft, n_mels, 0.0, None, True, 1).T.astype(F32)))


@functools.lru_cache(maxsize=None)
def bank70():
    """70 filters (no multiple of 64) over the 1025 bins, what the stock bank never has: 0 a single tap on bin 0; 1 a band ending on
    bin 1024; 2 an empty filter; 3 a filter with interior zeros; 4 a dense filter over all 1025 bins; the rest random bands, two of
    them touching the two edge bins again."""
    r = rng_of(70)
    fb = np.zeros((NB, 70), F32)
    fb[0, 0] = 0.75
    fb[1000:1025, 1] = r.uniform(0.1, 1.0, 25)
    fb[[40, 41, 45, 52], 3] = [0.5, 0.25, 1.0, 0.125]
    fb[:, 4] = r.uniform(0.001, 0.01, NB)
    for q in range(5, 70):
        s, l = int(r.integers(0, 1000)), int(r.integers(1, 40))
        fb[s:min(s + l, NB), q] = r.uniform(0.01, 1.0, min(s + l, NB) - s)
    fb[0:7, 68] = r.uniform(0.1, 1.0, 7)
    fb[1020:1025, 69] = r.uniform(0.1, 1.0, 5)
    return _ro(fb)


BANK70_EMPTY = (2,)


def identity_bank():
    return np.eye(NB, dtype=F32)


def edge_bank(n_mels=256):
    """The engine-level case's freq2mel: the stock bank with filter 0 replaced by a tap on bin 0 and the last filter by a band ending
    on bin 1024, both heavy enough to be the loudest outputs of edge_signal()."""
    fb = np.array(stock_bank(n_mels))
    fb[:, 0] = 0
    fb[0, 0] = 1.0
    fb[:, n_mels - 1] = 0
    fb[1017:1025, n_mels - 1] = np.linspace(0.125, 1.0, 8, dtype=F32)
    return fb


def edge_signal(t=48000, seed=3):
    """Alternating +-0.3 (the Nyquist bin) plus a 0.2 offset (the DC bin) plus noise."""
    n = np.arange(t)
    return (np.where(n % 2 == 0, 0.3, -0.3) + 0.2 + 0.01 * rng_of(seed, t).standard_normal(t)).astype(F32)


# ---- framing -----------------------------------------------------------------------------------------------------------------------
def audio_case(case):
    """Noise plus a constant 1.0 (a clamped sample in place of a zero pad is then a gross error): (B, T) float32."""
    b, t = case[0], case[1]
    return (rng_of(*case).standard_normal((b, t)) * 0.25 + 1.0).astype(F32)


def frames_of(x, n_dft, hop, pad_left, n_frames, edge=False):
    """x (B, T) -> (B, n_frames, n_dft) in x's dtype: sample f hop - pad_left + k, zero outside [0, T) (edge: the nearest sample)."""
    t = x.shape[1]
    idx = np.arange(n_frames)[:, None] * hop - pad_left + np.arange(n_dft)[None, :]
    inside = (idx >= 0) & (idx < t)
    fr = x[:, np.clip(idx, 0, t - 1)]
    return fr if edge else np.where(inside[None], fr, x.dtype.type(0))


def folded32(fr, ke, ko):
    """frame_audio_folded in float32: fe[j] = x[j] + x[N - j] (x[0], x[N / 2] alone), fo[j] = x[j + 1] - x[N - j - 1], zero padded."""
    fr = np.asarray(fr, F32)
    n = fr.shape[-1]
    h = n // 2
    fe = np.zeros(fr.shape[:-1] + (ke,), F32)
    fo = np.zeros(fr.shape[:-1] + (ko,), F32)
    fe[..., 0], fe[..., h] = fr[..., 0], fr[..., h]
    fe[..., 1:h] = fr[..., 1:h] + fr[..., :h:-1]
    fo[..., :h - 1] = fr[..., 1:h] - fr[..., :h:-1]
    return fe, fo


def packed32(fr, win32):
    """dft_pack_frames in float32: a1[n2][n1] = frame[64 n1 + n2] win[64 n1 + n2]."""
    xw = np.asarray(fr, F32) * np.asarray(win32, F32)
    return np.ascontiguousarray(np.swapaxes(xw.reshape(fr.shape[:-1] + (N1, N2)), -1, -2))


# ---- the transform -----------------------------------------------------------------------------------------------------------------
def staged_dft(xw, order='k1+32k2'):
    """The factored 2048-point transform of xw (rows, 2048) in float64, stage by stage: dict of Y (rows, 64, 32) complex [n2][k1],
    Z (rows, 32, 64) [k1][n2], X (rows, 1025) and nyq (rows).  order 'k2+32k1' is the control with the bins mis-ordered."""
    xw = np.asarray(xw, F64)
    rows = xw.shape[0]
    x = xw.reshape(rows, N1, N2)                                                  # [n1][n2]
    w32 = np.exp(-2j * np.pi * np.outer(np.arange(N1), np.arange(N1)) / N1)       # [n1][k1]
    Y = np.einsum('rab,ak->rbk', x, w32)                                          # [n2][k1]
    t = np.exp(-2j * np.pi * np.outer(np.arange(N2), np.arange(N1)) / N)          # [n2][k1]
    Z = np.swapaxes(Y * t, 1, 2)                                                  # [k1][n2]
    w64 = np.exp(-2j * np.pi * np.outer(np.arange(N2), np.arange(N2 // 2)) / N2)  # [n2][k2]
    X2 = Z @ w64                                                                  # [k1][k2]
    nyq = (Y[:, :, 0].real * np.where(np.arange(N2) % 2, -1.0, 1.0)).sum(1)
    X = np.empty((rows, NB), np.complex128)
    if order == 'k1+32k2':
        X[:, :N // 2] = np.swapaxes(X2, 1, 2).reshape(rows, -1)                   # k = k1 + 32 k2
    else:
        X[:, :N // 2] = X2.reshape(rows, -1)                                      # k = k2 + 32 k1: wrong
    X[:, N // 2] = nyq
    return dict(Y=Y, Z=Z, X=X, nyq=nyq)


def fused64(x32, hop, pad_left, n_frames, win32, edge=False, order=None):
    """The power spectrum dft_fused has before its mel product, in float64 from the float32 audio and window: (B n_frames, 1025)."""
    fr = frames_of(np.asarray(x32, F32), N, hop, pad_left, n_frames, edge).astype(F64).reshape(-1, N)
    xw = fr * np.asarray(win32, F64)
    X = np.fft.rfft(xw, axis=1) if order is None else staged_dft(xw, order)['X']
    return X.real ** 2 + X.imag ** 2


def tone_sweep():
    """1025 one-frame rows: row k = 0.5 cos(2 pi k n / 2048 + phi_k), phi = 0 for k = 0 and 1024 (else the tone would vanish)."""
    phi = rng_of(1025).uniform(0, 2 * np.pi, NB)
    phi[0] = phi[N // 2] = 0.0
    n = np.arange(N, dtype=F64)
    return (0.5 * np.cos(2 * np.pi * np.arange(NB)[:, None] * n[None, :] / N + phi[:, None])).astype(F32)


def row_d(got, ref):
    """d = max |got - ref| / max ref per row, the largest over the rows."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float((np.abs(got - ref).max(1) / ref.max(1)).max())


def rows_of(out):
    """An operator's (B, F, n_frames) as (B n_frames, F)."""
    out = np.asarray(out)
    return np.ascontiguousarray(np.swapaxes(out, 1, 2)).reshape(-1, out.shape[1])


# ---- dft_twiddle -------------------------------------------------------------------------------------------------------------------
def twiddle_input(frames):
    return rng_of(7, frames).standard_normal((frames, N2, 2 * N1)).astype(F32)


def twiddle_ratios(y32, tw32, a2, nyq):
    """a2 and nyq against float64 arithmetic on the float32 y (frames, 64, [re k1 | im k1]) and table."""
    y, tw = np.asarray(y32, F64), np.asarray(tw32, F64)
    yr, yi = np.swapaxes(y[:, :, :N1], 1, 2), np.swapaxes(y[:, :, N1:], 1, 2)          # [k1][n2]
    co, si = tw[:, :, 0].T[None], tw[:, :, 1].T[None]
    re, im = yr * co + yi * si, yi * co - yr * si
    ref = np.concatenate([re, im], axis=2)
    mag = np.abs(yr * co) + np.abs(yi * si)
    mag_i = np.abs(yi * co) + np.abs(yr * si)
    bound = 2 * U24 * np.concatenate([mag, mag_i], axis=2)
    y0 = y[:, :, 0]
    nref = (y0 * np.where(np.arange(N2) % 2, -1.0, 1.0)).sum(1)
    # measured: a2 0.94 of the bound (300 frames), nyq 0.071
    return {'a2': _ratio(np.abs(np.asarray(a2, F64) - ref), bound),
            'nyq': _ratio(np.abs(np.asarray(nyq, F64) - nref), 8 * U24 * np.abs(y0).sum(1))}


# ---- spec_to_features --------------------------------------------------------------------------------------------------------------
def spec_input(rows, n_dft, quiet_rows=0, seed=0):
    """A transform to feed spec_to_features: re, im (rows, nb) float32 (the Nyquist bin real).  The last `quiet_rows` rows are 0, tiny
    or just under the floors' thresholds, so that the amin branches run."""
    nb = n_dft // 2 + 1
    r = rng_of(11, rows, n_dft, seed)
    re, im = r.standard_normal((rows, nb)).astype(F32), r.standard_normal((rows, nb)).astype(F32)
    im[:, nb - 1] = 0
    for i, scale in zip(range(rows - quiet_rows, rows), (0.0, 1e-12, 2e-7, 4e-6)):
        re[i] *= F32(scale)
        im[i] *= F32(scale)
    return _ro(re, im)


def spec_layout(layout, re, im, cfg):
    """re, im (rows, nb) as spec_to_features reads them: (spec, nyq or None)."""
    rows, nb = re.shape
    if layout == 'unfolded':
        s = np.zeros((rows, cfg['ncols_pad']), F32)
        s[:, :nb], s[:, nb:2 * nb] = re, im
        return s, None
    if layout == 'folded':
        s = np.zeros((2 * rows, cfg['nc']), F32)
        s[:rows, :nb], s[rows:, :nb] = re, im
        return s, None
    assert nb == NB
    s = np.empty((rows, N1, N2), F32)                                               # [k1][re k2 | im k2], k = k1 + 32 k2
    s[:, :, :N2 // 2] = np.swapaxes(re[:, :N // 2].reshape(rows, N2 // 2, N1), 1, 2)
    s[:, :, N2 // 2:] = np.swapaxes(im[:, :N // 2].reshape(rows, N2 // 2, N1), 1, 2)
    return s, np.ascontiguousarray(re[:, N // 2])


def features(pw, fb, sqrt_out=False, db=False, loglambda=False, dtype=F64, amin=1e-10, power_scale=1.0):
    """spec_to_features' arithmetic after the power spectrum pw (rows, nb) in `dtype`: (rows, F).  amin and power_scale are the
    controls' handles."""
    t = np.dtype(dtype).type
    v = np.asarray(pw, dtype) * t(power_scale)
    if fb is not None:
        v = v @ np.asarray(fb, dtype)
    if sqrt_out:
        v = np.sqrt(v)
    if db:
        v = t(10) * np.log(np.maximum(v, t(amin))) / (LN10_32 if dtype == F32 else t(np.log(10.0)))
    if loglambda:
        v = np.log(np.maximum(v, t(1e-12))) / t(5)
    return v.astype(dtype)


def power_of(re, im, dtype=F64):
    re, im = np.asarray(re, dtype), np.asarray(im, dtype)
    return re * re + im * im


def linear_ratio(got, re, im, fb):
    """Flags off: |got - ref| <= (mel_len + 3) 2^-24 ref per element (3 2^-24 ref without mels); an empty filter exactly 0.
    Measured: 0.58 of the bound without mels (n_dft 512), 0.39 with the 128-mel bank, 0.37 / 0.40 / 0.34 factored with the 256-mel,
    the 70-filter and the identity bank."""
    pw = power_of(re, im)
    if fb is None:
        return _ratio(np.abs(np.asarray(got, F64) - pw), 3 * U24 * pw)
    ref = pw @ np.asarray(fb, F64)
    ln = pack_bands(fb)[1].astype(F64)
    r = _ratio(np.abs(np.asarray(got, F64) - ref), (ln[None, :] + 3) * U24 * ref)
    empty = ln == 0
    return r if np.all(np.asarray(got)[:, empty] == 0) else np.inf


def d_of(got, ref):
    ref = np.asarray(ref, F64)
    return float(np.abs(np.asarray(got, F64) - ref).max() / np.abs(ref).max())


def flag_ratios(got, re, im, fb, fl):
    """One flag set: (ratios, d, d32).  'k_d32': d / (K_D32 max(d32, ULP32)); 'floor': the values under amin bit-equal to the float32
    floor expression."""
    pw64 = power_of(re, im)
    ref = features(pw64, fb, dtype=F64, **fl)
    ref32 = features(power_of(re, im, F32), fb, dtype=F32, **fl)
    d, d32 = d_of(got, ref), d_of(ref32, ref)
    lin = features(pw64, fb, sqrt_out=fl.get('sqrt_out', False))
    # far enough under the threshold that no rounding of the value itself decides the branch
    under = lin < (1e-12 if fl.get('loglambda') else 1e-10) * (1 - 1e-3)
    res = {'k_d32': d / (K_D32 * max(d32, ULP32))}
    if fl.get('db') or fl.get('loglambda'):
        floor = LOG_FLOOR32 if fl.get('loglambda') else DB_FLOOR32
        assert under.any()
        res['floor'] = 0.0 if np.all(np.asarray(got, F32)[under] == floor) else np.inf
    return res, d, d32


# ---- db_normalize ------------------------------------------------------------------------------------------------------------------
def db_input(b, per, kind='plain'):
    """dB-like values in [-100, 30].  'floor_row': sample 1 (0 where B = 1) is entirely -100; 'last_max': the batch maximum is the
    last value of the last sample."""
    x = rng_of(13, b, per).uniform(-100, 30, (b, per)).astype(F32)
    if kind == 'floor_row':
        x[min(1, b - 1)] = -100
    if kind == 'last_max':
        x[b - 1, per - 1] = 31
    return x


def db_normalize32(x, scope):
    x = np.asarray(x, F32)
    mx = x.max(axis=1, keepdims=True) if scope == 'sample' else x.max()
    return np.maximum(x - mx, F32(-80))


def lines(kernel, case, res):
    return ['FESTAGE %s %s %s %.4g' % (kernel, case, k, v) for k, v in sorted(res.items())]
