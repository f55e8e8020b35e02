"""Restatement of the VGGish feature path in NumPy, written from the formulae the project documents (DESIGN.md section 8d;
data/usc/features.py:166-240 and data/usc/vggish/*.py are the lines it restates).  Every function takes the dtype it computes
in: float64 is the yardstick of the tests, float32 the same formulae at the kernels' precision (what the tests' bounds are
derived from).  Nothing here is used by the product.
"""
import numpy as np

SR, WIN, HOP, NFFT, BINS, MELS, ROWS = 16000, 400, 160, 512, 257, 64, 96
MIN_SAMPLES = 15600
LAYERS = (('conv1', 1, 64, True), ('conv2', 64, 128, True), ('conv3/conv3_1', 128, 256, False), ('conv3/conv3_2', 256, 256, True),
          ('conv4/conv4_1', 256, 512, False), ('conv4/conv4_2', 512, 512, True))
DENSE = (('fc1/fc1_1', 12288, 4096), ('fc1/fc1_2', 4096, 4096), ('fc2', 4096, 128))


def hann_periodic(n, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2 * np.pi / n * np.arange(n))).astype(dtype)


def mel_matrix(dtype=np.float64):
    """257 x 64: triangles in HTK mel (1127 ln(1 + f / 700)) between 125 and 7500 Hz over the bins of a 512-point DFT at 16 kHz;
    the DC bin zeroed"""
    def mel(f):
        return 1127.0 * np.log(1.0 + f / 700.0)
    bins = mel(np.linspace(0.0, SR / 2.0, BINS))
    edges = np.linspace(mel(125.0), mel(7500.0), MELS + 2)
    m = np.empty((BINS, MELS))
    for i in range(MELS):
        lo, c, hi = edges[i:i + 3]
        m[:, i] = np.maximum(0.0, np.minimum((bins - lo) / (c - lo), (hi - bins) / (hi - c)))
    m[0, :] = 0.0
    return m.astype(dtype)


def frame_count(n):
    return 0 if n < WIN else 1 + (n - WIN) // HOP


def log_mel(x, dtype=np.float64, dft='rfft'):
    """(frames, 64): log(|DFT_512(frame x hann)| . mel + 0.01), frames of 400 at hop 160, the tail dropped.  dft='matrix' sums the
    transform as a matrix product (the kernel's form) instead of np.fft.rfft."""
    x = np.asarray(x, dtype)
    f = frame_count(x.size)
    idx = np.arange(f)[:, None] * HOP + np.arange(WIN)[None, :]
    frames = x[idx] * hann_periodic(WIN, dtype)
    if dft == 'rfft':
        spec = np.fft.rfft(frames.astype(np.float64 if dtype == np.float64 else np.float32), NFFT)
        mag = np.abs(spec).astype(dtype)
    else:
        ph = 2 * np.pi * ((np.arange(WIN)[:, None] * np.arange(BINS)[None, :]) % NFFT) / NFFT
        re, im = frames @ np.cos(ph).astype(dtype), frames @ np.sin(ph).astype(dtype)
        mag = np.sqrt(re * re + im * im)
    return np.log(mag @ mel_matrix(dtype) + dtype(0.01)).astype(dtype)


def example_hop(hop_size):
    return int(round(hop_size * (1.0 / 0.010)))


def example_count(n_samples, hop_size):
    f = frame_count(max(n_samples, MIN_SAMPLES))
    return 1 + (f - ROWS) // example_hop(hop_size)


def pad_clip(x):
    x = np.asarray(x)
    if x.size >= MIN_SAMPLES:
        return x
    pad = MIN_SAMPLES - x.size
    return np.pad(x, (pad // 2, pad - pad // 2), mode='constant')


def examples(lm, hop_size):
    hop = example_hop(hop_size)
    n = 1 + (lm.shape[0] - ROWS) // hop
    return np.stack([lm[k * hop:k * hop + ROWS] for k in range(n)]) if n > 0 else np.zeros((0, ROWS, MELS), lm.dtype)


def conv3x3_same(x, w, b):
    """x (n, H, W, Cin), w (3, 3, Cin, Cout), zero padding of 1: sum over the nine taps of shifted products"""
    n, H, W, _ = x.shape
    xp = np.zeros((n, H + 2, W + 2, x.shape[3]), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    y = np.zeros((n, H, W, w.shape[3]), x.dtype)
    for kh in range(3):
        for kw in range(3):
            y += xp[:, kh:kh + H, kw:kw + W] @ w[kh, kw]
    return y + b


def pool2(x):
    n, H, W, C = x.shape
    return x.reshape(n, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def he_weights(seed):
    """He-normal kernels and small biases from a seed, float32, under the TF variable names.  The reference initialises with a
    truncated normal of standard deviation 0.01 (vggish_params INIT_STDDEV), under which the activations shrink by orders of
    magnitude per layer and the embedding of an untrained network is numerically nothing; He-normal keeps every layer's output at
    the scale of its input, so a parity test sees every layer."""
    rng = np.random.RandomState(seed)
    w = {}
    for name, cin, cout, _ in LAYERS:
        w['vggish/%s/weights' % name] = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        w['vggish/%s/biases' % name] = (rng.standard_normal(cout) * 0.05).astype(np.float32)
    for name, cin, cout in DENSE:
        w['vggish/%s/weights' % name] = (rng.standard_normal((cin, cout)) * np.sqrt(2.0 / cin)).astype(np.float32)
        w['vggish/%s/biases' % name] = (rng.standard_normal(cout) * 0.05).astype(np.float32)
    return w


def network(ex, weights, dtype=np.float64):
    """ex (n, 96, 64) -> (n, 128): the embedding after fc2's ReLU"""
    x = np.asarray(ex, dtype)[..., None]
    for name, _, _, pool in LAYERS:
        x = np.maximum(conv3x3_same(x, weights['vggish/%s/weights' % name].astype(dtype), weights['vggish/%s/biases' % name].astype(dtype)), 0)
        if pool:
            x = pool2(x)
    x = x.reshape(x.shape[0], -1)
    for name, _, _ in DENSE:
        x = np.maximum(x @ weights['vggish/%s/weights' % name].astype(dtype) + weights['vggish/%s/biases' % name].astype(dtype), 0)
    return x


def pca_clip(emb, pca, means, dtype=np.float64):
    """clip(pca (e - means), -2, 2)"""
    e = np.asarray(emb, dtype)
    return np.clip((np.asarray(pca, dtype) @ (e.T - np.asarray(means, dtype).reshape(-1, 1))).T, -2.0, 2.0)


def prequant(clipped):
    """the value the quantiser truncates: (x + 2) * (255 / 4)"""
    return (clipped - (-2.0)) * (255.0 / (2.0 - (-2.0)))


def postprocess(emb, pca, means, quantize=True, dtype=np.float64):
    c = pca_clip(emb, pca, means, dtype)
    return prequant(c).astype(np.uint8) if quantize else c


def seeded_pca(emb, seed):
    """A PCA matrix and means for embeddings `emb` (float64) under which the postprocessed output uses the whole quantiser: rows of
    a random orthogonal matrix scaled so that each output coordinate has standard deviation 1.4 over `emb` (a normal variable then
    clips at -2 / +2 about 8 % of the time each side), means = the embeddings' mean."""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.standard_normal((128, 128)))
    means = emb.mean(axis=0)
    proj = (emb - means) @ q.T
    q = q / (proj.std(axis=0)[:, None] / 1.4 + 1e-12)
    return q.astype(np.float32), means.astype(np.float32)


def network_torch32(ex, weights):
    """the same network in float32 on torch-CPU (conv2d / max_pool2d / linear): what a float32 implementation with another
    summation order gives -- the tests' bounds are multiples of its distance from float64"""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(ex, np.float32))[:, None]                  # NCHW
        for name, _, _, pool in LAYERS:
            w = torch.from_numpy(weights['vggish/%s/weights' % name]).permute(3, 2, 0, 1).contiguous()
            x = F.relu(F.conv2d(x, w, torch.from_numpy(weights['vggish/%s/biases' % name]), padding=1))
            if pool:
                x = F.max_pool2d(x, 2, 2)
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)                                      # NHWC flatten
        for name, _, _ in DENSE:
            x = F.relu(F.linear(x, torch.from_numpy(weights['vggish/%s/weights' % name]).t().contiguous(),
                                torch.from_numpy(weights['vggish/%s/biases' % name])))
        return x.numpy()


def chain(clips16, hop_size, weights, dtype):
    """clips at 16 kHz -> embeddings of all their examples (n, 128): pad, log-mel, examples, network, in `dtype` (float64: NumPy;
    float32: NumPy log-mel through rfft and the torch-CPU network)"""
    ex = np.concatenate([examples(log_mel(pad_clip(np.asarray(c, dtype)), dtype), hop_size) for c in clips16])
    return network(ex, weights, np.float64) if dtype == np.float64 else network_torch32(ex, weights)


def pca_unclipped(emb, pca, means):
    return (np.asarray(pca, np.float64) @ (np.asarray(emb, np.float64).T - np.asarray(means, np.float64).reshape(-1, 1))).T


def quantised_agreement(got_q, unclipped64, delta):
    """(fraction of entries left out, mismatches outside them).  u = (x + 2) * 63.75 of the float64 value x BEFORE the clip: the
    quantiser's steps are the integers 1..255 inside (0, 255) and the two clip edges; an entry is left out when u lies within delta
    of one of them (beyond an edge by more than delta the result is 0 or 255 whatever the rounding)."""
    u = prequant(unclipped64)
    inside = (u > 0) & (u < 255)
    near = np.where(inside, np.abs(u - np.round(u)) <= delta, np.minimum(np.abs(u), np.abs(u - 255)) <= delta)
    want = np.clip(u, 0, 255).astype(np.uint8).astype(np.float32)
    return float(near.mean()), int((np.asarray(got_q) != want)[~near].sum())


def quantiser_coverage(q64):
    """(share at 0, share at 255, share strictly between, distinct values) of a float64-path quantised output"""
    return float((q64 == 0).mean()), float((q64 == 255).mean()), float(((q64 > 0) & (q64 < 255)).mean()), int(np.unique(q64).size)


def varied_clips(seed, lengths):
    """float32 clips of different kinds in turn -- noise at three levels, tones over noise, a chirp, hard-clipped noise -- so that
    their embeddings spread (a PCA fitted to near-identical embeddings would only magnify rounding)"""
    rng = np.random.RandomState(seed)
    out = []
    for i, n in enumerate(lengths):
        t = np.arange(n) / 16000.0
        kind = i % 6
        if kind < 3:
            x = (0.01, 0.1, 0.7)[kind] * rng.standard_normal(n)
        elif kind == 3:
            x = 0.4 * np.sin(2 * np.pi * rng.uniform(200, 3000) * t) + 0.2 * np.sin(2 * np.pi * rng.uniform(3000, 7000) * t) \
                + 0.003 * rng.standard_normal(n)
        elif kind == 4:
            x = 0.5 * np.sin(2 * np.pi * (300 * t + 900 * t * t)) * np.exp(-t) + 0.001 * rng.standard_normal(n)
        else:
            x = np.clip(3.0 * rng.standard_normal(n), -1, 1)
        out.append(x.astype(np.float32))
    return out
