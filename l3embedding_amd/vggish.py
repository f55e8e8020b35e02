"""VGGish baseline features on the GPU -- data/usc/features.py:166-240 (extract_vggish_embedding, get_vggish_frames_uniform) with
vggish/vggish_input.py, mel_features.py, vggish_slim.py and vggish_postprocess.py.

The framing rule lives here and only here: `example_table` turns 16 kHz clip lengths into the pad of each clip and the first
log-mel row of each example; the C side (l3_vggish_embed_clips_resampled, csrc/vggish.hip) follows the table on the GPU.  The
weights come from two files in `resources_dir`: vggish_pca_params.npz, the reference's own file (pca_eigen_vectors, pca_means),
and vggish_model.npz, the variables of the released TF checkpoint under their TF names (DESIGN.md section 8d gives the lines that
dump it where TensorFlow exists; reading the .ckpt itself is not built).
"""
import os

import numpy as np

SAMPLE_RATE = 16000
MIN_SAMPLES = int(np.ceil(SAMPLE_RATE * max(0.96, 0.975)))      # 15600, features.py:175
STFT_WIN, STFT_HOP = 400, 160                                    # 25 ms / 10 ms at 16 kHz
EXAMPLE_ROWS = 96                                                # frame_win_sec 0.96 at 100 rows per second
EMBEDDING_SIZE = 128

# TF variable name -> shape (vggish_slim.py:66-99; HWIO convolutions, (in, out) dense layers)
WEIGHT_SHAPES = {}
for _scope, _cin, _cout in (('conv1', 1, 64), ('conv2', 64, 128), ('conv3/conv3_1', 128, 256), ('conv3/conv3_2', 256, 256),
                            ('conv4/conv4_1', 256, 512), ('conv4/conv4_2', 512, 512)):
    WEIGHT_SHAPES['vggish/%s/weights' % _scope] = (3, 3, _cin, _cout)
    WEIGHT_SHAPES['vggish/%s/biases' % _scope] = (_cout,)
for _scope, _cin, _cout in (('fc1/fc1_1', 12288, 4096), ('fc1/fc1_2', 4096, 4096), ('fc2', 4096, 128)):
    WEIGHT_SHAPES['vggish/%s/weights' % _scope] = (_cin, _cout)
    WEIGHT_SHAPES['vggish/%s/biases' % _scope] = (_cout,)

# parameters of extract_vggish_embedding's **params that this build fixes, with the reference's defaults (vggish_input.py:25-29,
# vggish_postprocess.py:33-34, features.py:170-171)
FIXED_PARAMS = dict(target_sample_rate=16000, stft_win_len_sec=0.025, stft_hop_len_sec=0.010, num_mel_bins=64, mel_min_hz=125,
                    mel_max_hz=7500, frame_win_sec=0.96, embedding_size=128)

# examples per device call: the log-mel of the clips they come from is computed once per call
CALL_EXAMPLES = 8192
CALL_SAMPLES = 1 << 25


def example_hop_rows(hop_size):
    """vggish_input.py:65-69: the hop between examples in log-mel rows"""
    hop = int(round(hop_size * (1.0 / 0.010)))
    if hop < 1:
        raise ValueError('hop_size %r is below one log-mel row (10 ms)' % (hop_size,))
    return hop


def example_table(lengths_16k, hop_size=0.1):
    """Examples of clips of these lengths at 16 kHz, as extract_vggish_embedding cuts them:

    - a clip shorter than 15600 samples is zero-padded to 15600, pad // 2 in front and the rest behind (features.py:175-181);
    - the padded clip of n samples has F = 1 + (n - 400) // 160 log-mel rows (mel_features.py:42) and 1 + (F - 96) // hop examples,
      hop = int(round(hop_size * 100)) rows, the tail dropped (vggish_input.py:64-75).

    Returns (pads, rows, counts): pads (n_clips, 2) int64 {left pad, padded length}; rows (n_examples,) int64, the first log-mel
    row of each example when the clips' log-mel rows lie back to back in clip order; counts (n_clips,) int64 examples per clip."""
    hop = example_hop_rows(hop_size)
    L = np.asarray(lengths_16k, dtype=np.int64).reshape(-1)
    if (L < 0).any():
        raise ValueError('clip lengths must be >= 0')
    padded = np.maximum(L, MIN_SAMPLES)
    pads = np.stack([(padded - L) // 2, padded], axis=1).astype(np.int64)
    frames = 1 + (padded - STFT_WIN) // STFT_HOP
    counts = (1 + (frames - EXAMPLE_ROWS) // hop).astype(np.int64)
    row0 = np.concatenate([[0], np.cumsum(frames)[:-1]]) if L.size else np.zeros(0, np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]) if L.size else np.zeros(0, np.int64)
    k = np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(first, counts)
    rows = np.repeat(row0, counts) + k * hop
    return pads, rows.astype(np.int64), counts


def load_weights(resources_dir):
    """(weights, pca_matrix, pca_means) from vggish_model.npz and vggish_pca_params.npz; ValueError names what is missing or
    mis-shaped"""
    model_path = os.path.join(resources_dir, 'vggish_model.npz')
    pca_path = os.path.join(resources_dir, 'vggish_pca_params.npz')
    for p in (model_path, pca_path):
        if not os.path.exists(p):
            raise ValueError('%s not found (the VGGish resources directory holds vggish_model.npz and vggish_pca_params.npz)' % p)
    weights = {}
    with np.load(model_path) as z:
        for name, shape in WEIGHT_SHAPES.items():
            key = name if name in z.files else name + ':0' if name + ':0' in z.files else None
            if key is None:
                raise ValueError('%s: tensor %s is missing' % (model_path, name))
            a = z[key]
            if a.shape != shape:
                raise ValueError('%s: tensor %s has shape %s, expected %s' % (model_path, name, a.shape, shape))
            weights[name] = np.ascontiguousarray(a, np.float32)
    with np.load(pca_path) as z:
        for key in ('pca_eigen_vectors', 'pca_means'):
            if key not in z.files:
                raise ValueError('%s: tensor %s is missing' % (pca_path, key))
        pca, means = z['pca_eigen_vectors'], z['pca_means']
    if pca.shape != (EMBEDDING_SIZE, EMBEDDING_SIZE):
        raise ValueError('%s: tensor pca_eigen_vectors has shape %s, expected (128, 128)' % (pca_path, pca.shape))
    if means.size != EMBEDDING_SIZE:
        raise ValueError('%s: tensor pca_means has shape %s, expected 128 values' % (pca_path, means.shape))
    return weights, np.ascontiguousarray(pca, np.float32), np.ascontiguousarray(means.reshape(-1), np.float32)


class VGGishModel(object):
    """The VGGish network with its postprocessor on one GPU.  VGGishModel(resources_dir) reads the two .npz files;
    VGGishModel(weights=..., pca_matrix=..., pca_means=...) takes arrays (tests draw them from a seed)."""

    def __init__(self, resources_dir=None, weights=None, pca_matrix=None, pca_means=None, batch=0, device=0, conv=None):
        # conv: 'direct' (the default when None), 'f4x4' or 'f2x2' -- l3_vggish_set_conv
        from . import _lib
        if resources_dir is not None:
            weights, pca_matrix, pca_means = load_weights(resources_dir)
        if weights is None:
            raise ValueError('VGGishModel needs resources_dir or weights')
        for name, shape in WEIGHT_SHAPES.items():
            if name not in weights:
                raise ValueError('tensor %s is missing' % name)
            if tuple(np.shape(weights[name])) != shape:
                raise ValueError('tensor %s has shape %s, expected %s' % (name, np.shape(weights[name]), shape))
        self.net = _lib.VGGish(batch=batch, device=device)
        if conv is not None:
            self.net.set_conv(conv)
        for name in WEIGHT_SHAPES:
            self.net.set_weight(name, weights[name])
        self.has_pca = pca_matrix is not None
        if self.has_pca:
            self.net.set_pca(pca_matrix, pca_means)

    def close(self):
        self.net.close()

    def predict_clips(self, clips, rates, hop_size=0.1, quantize=True, postprocess=True):
        """extract_vggish_embedding for many files per call: clips are 1-D float32 arrays (channel mean taken), rates their
        sample rates in whole Hz.  Each clip is resampled to 16 kHz (resampy 'kaiser_best'; a 16 kHz clip is taken as it is),
        padded and framed as example_table says, all on the device.  Returns one (n_i, 128) float32 array per clip: quantised
        (values 0..255), clipped PCA output (quantize=False), or the raw embedding (postprocess=False)."""
        from .resample import check_rates, get_filter, output_length
        clips = [np.asarray(c, dtype=np.float32) for c in clips]
        for c in clips:
            if c.ndim != 1:
                raise ValueError('every clip must be a 1-D array (got shape %s)' % (c.shape,))
        rates = [check_rates(r, SAMPLE_RATE)[0] for r in np.asarray(rates).reshape(-1).tolist()]
        if len(rates) != len(clips):
            raise ValueError('rates must give one rate per clip (%d rates, %d clips)' % (len(rates), len(clips)))
        if not clips:
            return []
        mode = 'raw' if not postprocess else 'quantized' if quantize else 'pca'
        if mode != 'raw' and not self.has_pca:
            raise ValueError('this model was built without PCA parameters: only postprocess=False is available')
        win, num_table = get_filter('kaiser_best')
        native = np.array([c.size for c in clips], np.int64)
        L16 = np.array([n if r == SAMPLE_RATE else output_length(int(n), r, SAMPLE_RATE) for n, r in zip(native.tolist(), rates)],
                       np.int64)
        pads, rows, counts = example_table(L16, hop_size)
        frames = 1 + (pads[:, 1] - STFT_WIN) // STFT_HOP
        out, i, n = [], 0, len(clips)
        while i < n:
            j, ex, smp = i, 0, 0
            while j < n and (j == i or (ex + counts[j] <= CALL_EXAMPLES and smp + native[j] + pads[j, 1] <= CALL_SAMPLES)):
                ex += int(counts[j])
                smp += int(native[j] + pads[j, 1])
                j += 1
            x_off = np.concatenate([[0], np.cumsum(native[i:j])[:-1]])
            y_off = np.concatenate([[0], np.cumsum(pads[i:j, 1])[:-1]])
            table = np.stack([x_off, native[i:j], np.array(rates[i:j], np.int64), np.zeros(j - i, np.int64), L16[i:j],
                              y_off + pads[i:j, 0]], axis=1)
            table = table[L16[i:j] > 0]                       # an empty clip is all padding
            segments = np.stack([y_off, pads[i:j, 1]], axis=1)
            e0, e1 = int(counts[:i].sum()), int(counts[:j].sum())
            ex_rows = rows[e0:e1] - int(frames[:i].sum())
            x = np.concatenate(clips[i:j]) if native[i:j].sum() else np.zeros(1, np.float32)
            emb = self.net.embed_clips_resampled(x, table, win, num_table, int(pads[i:j, 1].sum()), segments, ex_rows, mode)
            for c in np.split(emb, np.cumsum(counts[i:j])[:-1]):
                out.append(c)
            i = j
        return out


_model_cache = {}


def _cached_model(resources_dir):
    key = os.path.abspath(resources_dir)
    if key not in _model_cache:
        _model_cache[key] = VGGishModel(key)
    return _model_cache[key]


def extract_vggish_embedding(audio_path, input_op_name='vggish/input_features', output_op_name='vggish/embedding',
                             resources_dir=None, vggish_model=None, **params):
    """features.py:166-221 on the GPU: (n_examples, 128) float32 of one audio file.  Honours frame_hop_sec (default 0.96, as
    waveform_to_examples) and quantize (default True); a parameter this build fixes (FIXED_PARAMS) raises ValueError with its name
    if given another value.  The model of a resources directory is kept between calls (the reference reloads it every time)."""
    from .features import read_wav
    for name, fixed in FIXED_PARAMS.items():
        if name in params and params[name] != fixed:
            raise ValueError('%s=%r: this build fixes %s at %r' % (name, params[name], name, fixed))
    if input_op_name != 'vggish/input_features' or output_op_name != 'vggish/embedding':
        raise ValueError('input_op_name / output_op_name: this build fixes the tensors at vggish/input_features and vggish/embedding')
    if vggish_model is None:
        if not resources_dir:
            resources_dir = os.path.join(os.path.dirname(__file__), '..', 'resources', 'vggish')
        vggish_model = _cached_model(resources_dir)
    data, sr = read_wav(audio_path)
    return vggish_model.predict_clips([data], [sr], hop_size=params.get('frame_hop_sec', 0.96),
                                      quantize=params.get('quantize', True))[0]
