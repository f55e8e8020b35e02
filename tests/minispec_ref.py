"""NumPy oracle of the 'minispec' front-end: the spectrogram the deployed pipeline computes for every second of
audio, restated from its arithmetic.

    x (48000 samples) -> n_fft / 2 zeros on both sides -> 199 frames of n_fft samples at hop 242 -> periodic Hann window -> DFT,
    bins 0 .. n_fft / 2 -> magnitude |X| -> (mel models) the htk, norm-1 filterbank of oracle.l3_oracle.mel_basis applied to the
    MAGNITUDE -> v^2 -> 10 log10(max(v^2, 1e-10)) -> minus the second's maximum -> clipped at -80.

float64 is the reference.  The float32 restatement (a float32 windowed DFT matrix, float32 products and sums) is the yardstick:
what the same steps cost in the GPU's number format.  `variant` alters the REFERENCE for the tests' controls:
    'kapre_pad'    the zeros kapre's framing puts in front (982 for n_fft 2048 under 'same'; none for 512 under 'valid'), the rest
                   behind, 199 frames all the same
    'mel_of_power' the filterbank on |X|^2, then the square root, then the square again: kapre's order of the two steps
    'unsquared'    10 log10 of v instead of v^2: kapre's dB scale, half of this one
"""
import numpy as np

from oracle import l3_oracle as o

SR = 48000
HOP = 242
N_FRAMES = 1 + SR // HOP                  # 199
MODELS = {'cnn_L3_kapredbinputbn': (512, 0), 'cnn_L3_melspec1': (2048, 128), 'cnn_L3_melspec2': (2048, 256)}     # n_fft, n_mels
AMIN = 1e-10
VARIANTS = (None, 'kapre_pad', 'mel_of_power', 'unsquared')


def window(n_fft, dtype=np.float64):
    n = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).astype(dtype)


def frames(audio, n_fft, pad_left=None):
    """audio (B, 48000) -> (B, 199, n_fft): frame f holds the samples f * 242 - pad_left ..., zeros outside the second."""
    audio = np.asarray(audio)
    pad_left = n_fft // 2 if pad_left is None else pad_left
    need = (N_FRAMES - 1) * HOP + n_fft
    x = np.zeros((audio.shape[0], need), audio.dtype)
    x[:, pad_left:pad_left + SR] = audio[:, :need - pad_left]
    idx = np.arange(N_FRAMES)[:, None] * HOP + np.arange(n_fft)[None, :]
    return x[:, idx]


def dft_matrix(n_fft, dtype):
    """(n_fft, n_fft / 2 + 1) windowed cos and -sin, computed in float64 and rounded once to dtype"""
    n = np.arange(n_fft, dtype=np.float64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.float64)[None, :]
    ang = 2.0 * np.pi * ((n * k) % n_fft) / n_fft
    w = window(n_fft)[:, None]
    return (w * np.cos(ang)).astype(dtype), (-w * np.sin(ang)).astype(dtype)


def magnitudes(audio, n_fft, dtype=np.float64, pad_left=None, squared=False, kernels=None):
    """|X| (or |X|^2) of every frame: (B, 199, n_fft / 2 + 1) in dtype.  kernels: (real, imag), each (n_fft, n_fft / 2 + 1), in
    place of the windowed DFT matrix (a model whose stored DFT kernels were edited)."""
    fr = frames(np.asarray(audio, dtype), n_fft, pad_left)
    b = fr.shape[0]
    re_m, im_m = dft_matrix(n_fft, dtype) if kernels is None else (np.asarray(k, dtype).reshape(n_fft, -1) for k in kernels)
    fr2 = fr.reshape(b * N_FRAMES, n_fft)
    re, im = fr2 @ re_m, fr2 @ im_m
    p = (re * re + im * im).reshape(b, N_FRAMES, -1)
    return p if squared else np.sqrt(p)


def kapre_pad(n_fft):
    return o.tf_same_pad(SR, n_fft, HOP)[1] if n_fft == 2048 else 0


def power(model_type, audio, dtype=np.float64, variant=None, kernels=None):
    """v^2 before the dB: (B, F, 199) in dtype.  The linear model's |X|^2 is formed without a square root in between."""
    assert variant in VARIANTS
    n_fft, n_mels = MODELS[model_type]
    pad = kapre_pad(n_fft) if variant == 'kapre_pad' else None
    if not n_mels:
        return np.transpose(magnitudes(audio, n_fft, dtype, pad, squared=True, kernels=kernels), (0, 2, 1))
    fb = o.mel_basis(SR, n_fft, n_mels).T.astype(np.float32).astype(dtype)       # (n_freq, n_mels), float32 values as the model stores them
    if variant == 'mel_of_power':
        v2 = magnitudes(audio, n_fft, dtype, pad, squared=True, kernels=kernels) @ fb
    else:
        v = magnitudes(audio, n_fft, dtype, pad, kernels=kernels) @ fb
        v2 = v * v
    return np.transpose(v2, (0, 2, 1))


def to_db(p, dtype=np.float64, unsquared=False):
    """10 log10(max(p, 1e-10)) - the second's maximum, clipped at -80; p (B, F, 199)"""
    p = np.asarray(p, dtype)
    if unsquared:
        p = np.sqrt(p)
    db = (10 * np.log(np.maximum(p, np.asarray(AMIN, dtype))) / np.asarray(np.log(10.0), dtype)).astype(dtype)
    db = db - db.reshape(db.shape[0], -1).max(axis=1)[:, None, None]
    return np.maximum(db, np.asarray(-80.0, dtype))


def minispec(model_type, audio, dtype=np.float64, variant=None, kernels=None):
    """audio (B, 48000) -> (B, F, 199, 1) dB in dtype"""
    p = power(model_type, audio, dtype, variant, kernels)
    return to_db(p, dtype, unsquared=variant == 'unsquared')[..., None]


def lin(db):
    """the dB values back in the power domain, relative to the second's largest value (which is 1)"""
    return 10.0 ** (np.asarray(db, np.float64) / 10.0)


def lin_d(got_db, ref_db):
    """per second: max |lin(got) - lin(ref)| / max lin(ref), the distance test_frontend_of_the_signals_in_the_linear_domain takes"""
    g, r = lin(got_db), lin(ref_db)
    g, r = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
    return np.abs(g - r).max(axis=1) / r.max(axis=1)


def signals():
    """(names, audio (6, 48000) float32): noise, test_frontend's two tones, silence, an impulse at sample 0, one at sample 47999
    and an alternating +-0.3 signal with its energy on the Nyquist bin"""
    t = np.arange(SR) / float(SR)
    r = np.random.RandomState(9)
    s = [('noise', r.uniform(-1, 1, SR)),
         ('tones', 0.5 * np.sin(2 * np.pi * 440 * t) + 0.05 * np.sin(2 * np.pi * 5000 * t)),
         ('silence', np.zeros(SR)),
         ('impulse0', np.eye(1, SR, 0)[0]),
         ('impulse47999', np.eye(1, SR, SR - 1)[0]),
         ('nyquist', np.where(np.arange(SR) % 2 == 0, 0.3, -0.3) * (1 + 0.1 * np.sin(2 * np.pi * 3 * t)))]
    return tuple(k for k, _ in s), np.stack([v for _, v in s]).astype(np.float32)


def tower_embedding_map(model_type, P, spec, dtype=np.float64):
    """The oracle's audio tower on spectrograms (n, F, frames, 1) of any width, up to the embedding layer's convolution, one row at
    a time: (n, h, w, 512)"""
    ops = o.model_spec(model_type)['audio']
    ops = ops[:[k for k, op in enumerate(ops) if op[0] == 'conv' and op[1] == 'audio_embedding_layer'][0] + 1]
    maps = []
    for i in range(spec.shape[0]):
        taps = {}
        o._tower_forward('audio_model', ops, np.asarray(spec[i:i + 1], dtype), P, False, taps)
        maps.append(taps['audio_embedding_layer'])
    return np.concatenate(maps)
