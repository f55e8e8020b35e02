"""VGGish feature path on the GPU against float64 (tests/vggish_ref.py) and against fixtures the reference's NumPy code wrote.

Bounds.  Log-mel and whole chain: 4 x the distance of a float32 run of the same formulae (NumPy rfft log-mel, torch-CPU network) from
float64 on the same inputs -- the kernels are float32 with another summation order.  Single operators: the kernel's own error
model, rounding x (sqrt(K) + 2) x sum |terms| per output (K products summed in float32 in some order, as test_svm_parity_gpu.py
bounds its kernels).  Weights are He-normal from a seed: under the reference's initialiser (truncated normal, sigma 0.01) the
activations of an untrained VGGish shrink layer by layer and the embedding collapses to nothing, so no layer would be tested.
Every figure is printed before it is asserted; profiles/r12_vggish.txt holds the figures of the runs made so far.
"""
import os

import numpy as np
import pytest

import vggish_ref as ref
from resample_ref import resample_ref
from l3embedding_amd import _lib, resample, vggish

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = 2.0 ** -24


def _logmel_inputs():
    rng = np.random.RandomState(1)
    n = 16000 * 3 + 77
    t = np.arange(n) / 16000.0
    broadband = (0.3 * rng.standard_normal(n)).astype(np.float32)
    tonal = (0.5 * np.sin(2 * np.pi * 440 * t) + 0.25 * np.sin(2 * np.pi * 2500 * t)).astype(np.float32)
    clipped = np.clip(4.0 * rng.standard_normal(n), -1, 1).astype(np.float32)
    return [('broadband', broadband), ('tonal', tonal), ('silent', np.zeros(n, np.float32)), ('clipped', clipped),
            ('400 samples', broadband[1000:1400]), ('401 samples', broadband[2000:2401])]


def test_logmel_matches_float64_within_4x_float32_numpy(gpu_required):
    """Per input: max |kernel - float64| <= 4 x max |float32 NumPy - float64| on the same input."""
    for name, x in _logmel_inputs():
        want = ref.log_mel(x.astype(np.float64))
        f32 = float(np.abs(ref.log_mel(x, np.float32) - want).max())
        got = _lib.op_vggish_logmel(x)
        err = float(np.abs(got - want).max())
        bound = 4 * f32
        print('logmel %-12s rows %4d  kernel-f64 %.3e  numpy32-f64 %.3e  bound %.3e' % (name, got.shape[0], err, f32, bound))
        assert got.shape == want.shape == (ref.frame_count(x.size), 64)
        assert err <= bound
    assert _lib.op_vggish_logmel(np.zeros(399, np.float32)).shape == (0, 64)


def test_logmel_matches_reference_fixture_and_segments(gpu_required):
    with np.load(os.path.join(GOLDEN, 'vggish_logmel.npz')) as z:
        x, want = z['audio'], z['log_mel']
    f32 = float(np.abs(ref.log_mel(x, np.float32) - want).max())
    got = _lib.op_vggish_logmel(x)
    print('logmel fixture: kernel-reference %.3e  numpy32-reference %.3e' % (np.abs(got - want).max(), f32))
    assert np.abs(got - want).max() <= 4 * f32
    # segments of one buffer: each as if alone, rows back to back; 33 frames = one full block and one frame
    segs = [[0, 400 + 160 * 32], [7000, 15600], [30000, 401]]
    both = _lib.op_vggish_logmel(x, segs)
    alone = np.concatenate([_lib.op_vggish_logmel(x[o:o + n]) for o, n in segs])
    assert both.shape == (33 + 96 + 1, 64) and np.array_equal(both, alone)


@pytest.mark.parametrize('n', [37, 2])
def test_conv1_gather_matches_float64(gpu_required, n):
    rng = np.random.RandomState(n)
    lm = (rng.standard_normal((96 + 10 * (n - 1) + 5, 64)) * 2 - 1).astype(np.float32)
    rows = np.arange(n, dtype=np.int64) * 10
    rows[-1] += 5                                                   # the last 96 rows of the buffer
    w = (rng.standard_normal((3, 3, 1, 64)) * 0.5).astype(np.float32)
    b = (rng.standard_normal(64) * 0.1).astype(np.float32)
    got = _lib.op_vggish_conv1(lm, rows, w, b)
    ex = np.stack([lm[r:r + 96] for r in rows]).astype(np.float64)[..., None]
    pre = ref.conv3x3_same(ex, w.astype(np.float64), b.astype(np.float64))
    want = ref.pool2(np.maximum(pre, 0))
    mag = ref.conv3x3_same(np.abs(ex), np.abs(w).astype(np.float64), np.abs(b).astype(np.float64))
    bound = EPS * (np.sqrt(9) + 2) * ref.pool2(mag)
    err = np.abs(got - want)
    print('conv1 n=%d: max err %.3e, max err / bound %.3f' % (n, err.max(), (err / bound).max()))
    assert got.shape == (n, 48, 32, 64) and (err <= bound).all()


@pytest.mark.parametrize('h,w,c,pool', [(48, 32, 128, 1), (24, 16, 256, 0), (24, 16, 256, 1), (12, 8, 512, 0), (12, 8, 512, 1)])
def test_bias_relu_tail_matches_float64(gpu_required, h, w, c, pool):
    rng = np.random.RandomState(h + c + pool)
    x = rng.standard_normal((37, h, w, c)).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    got = _lib.op_vggish_bias_relu(x, b, pool)
    y = np.maximum(x.astype(np.float64) + b.astype(np.float64), 0)
    mag = np.abs(x).astype(np.float64) + np.abs(b)
    want, bound = (ref.pool2(y), EPS * ref.pool2(mag)) if pool else (y, EPS * mag)          # one rounding: the addition
    err = np.abs(got - want)
    print('bias_relu %dx%dx%d pool %d: max err %.3e, max err / bound %.3f' % (h, w, c, pool, err.max(), (err / bound).max()))
    assert got.shape == want.shape and (err <= bound).all()


ALGOS = ['f4x4', 'f2x2', 'direct']


@pytest.mark.parametrize('algo', ALGOS)
@pytest.mark.parametrize('h,w,cin,cout,pool', [(48, 32, 64, 128, 1), (24, 16, 128, 256, 0), (24, 16, 256, 256, 1), (12, 8, 256, 512, 0),
                                               (12, 8, 512, 512, 1)])
def test_wide_convolutions_match_float64_at_vggish_geometry(gpu_required, h, w, cin, cout, pool, algo):
    """conv2 .. conv4_2 as the handle runs them (convolution, then the bias + ReLU (+ pool) tail), 37 examples: 37 x 3 x 2 = 222
    tiles of a 12 x 8 map do not fill whole blocks of 32.  Bound: K = 9 Cin products per output summed in float32."""
    rng = np.random.RandomState(h + cin + cout)
    x = np.maximum(rng.standard_normal((37, h, w, cin)), 0).astype(np.float32)            # what a ReLU hands the next layer
    k = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.05).astype(np.float32)
    got = _lib.op_vggish_conv(x, k, b, pool, algo)
    pre = ref.conv3x3_same(x.astype(np.float64), k.astype(np.float64), b.astype(np.float64))
    mag = ref.conv3x3_same(np.abs(x).astype(np.float64), np.abs(k).astype(np.float64), np.abs(b).astype(np.float64))
    want, bound = np.maximum(pre, 0), EPS * (np.sqrt(9 * cin) + 2) * mag
    if pool:
        want, bound = ref.pool2(want), ref.pool2(bound)
    err = np.abs(got - want)
    print('conv %s %dx%dx%d->%d pool %d: max err %.3e (%.2e of the range), max err / bound %.3f'
          % (algo, h, w, cin, cout, pool, err.max(), err.max() / (want.max() - want.min()), (err / bound).max()))
    assert got.shape == want.shape and (err <= bound).all()


@pytest.mark.parametrize('K,N', [(12288, 4096), (4096, 4096), (4096, 128)])
def test_dense_layers_match_float64_at_vggish_geometry(gpu_required, K, N):
    rng = np.random.RandomState(K + N)
    x = np.maximum(rng.standard_normal((37, K)), 0).astype(np.float32)
    w = (rng.standard_normal((K, N)) * np.sqrt(2.0 / K)).astype(np.float32)
    b = (rng.standard_normal(N) * 0.05).astype(np.float32)
    got = _lib.op_mlp_dense_fwd(x, w, b, relu=True)
    want = np.maximum(x.astype(np.float64) @ w.astype(np.float64) + b, 0)
    bound = EPS * (np.sqrt(K) + 2) * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64) + np.abs(b))
    err = np.abs(got - want)
    print('dense %dx%d rows 37: max err %.3e, max err / bound %.3f' % (K, N, err.max(), (err / bound).max()))
    assert (err <= bound).all()


def test_postprocess_matches_float64_and_reference_fixture(gpu_required):
    with np.load(os.path.join(GOLDEN, 'vggish_postprocess.npz')) as p:
        emb, pca, means, q_ref, c_ref = (p[k] for k in ('embeddings', 'pca_eigen_vectors', 'pca_means', 'quantized', 'clipped'))
    pca32, means32 = pca.astype(np.float32), means.astype(np.float32)
    emb = emb[:37]                                                  # a count that no tile size divides
    u64 = ref.pca_unclipped(emb, pca32, means32)
    got = _lib.op_vggish_postprocess(emb, pca32, means32, quantize=False)
    d = np.abs(emb.astype(np.float64)[:, None, :] - means32.astype(np.float64)[None, None, :])
    bound = EPS * (np.sqrt(128) + 3) * (d * np.abs(pca32).astype(np.float64)[None]).sum(axis=2)
    err = np.abs(got - np.clip(u64, -2, 2))
    print('postprocess: max err %.3e, max err / bound %.3f' % (err.max(), (err / bound).max()))
    assert (err <= bound).all()
    q = _lib.op_vggish_postprocess(emb, pca32, means32, quantize=True)
    left_out, mismatches = ref.quantised_agreement(q, u64, float(bound.max()) * 63.75)
    print('postprocess quantised: left out %.4f, mismatches %d' % (left_out, mismatches))
    assert mismatches == 0 and left_out <= 0.05
    # against the reference's own output (float64 arithmetic on the float64 parameters): the same, up to the float32 parameters
    left_out, mismatches = ref.quantised_agreement(q, ref.pca_unclipped(emb, pca, means), (float(bound.max()) + 4 * EPS * 128) * 63.75)
    assert mismatches == 0 and left_out <= 0.05


# ---- whole chain ---------------------------------------------------------------------------------------------------------------
RATES = (8000, 16000, 22050, 44100)


def _chain_clips():
    """(clips at their rates, rates): shorter than 0.975 s, exactly 15600 samples at 16 kHz, and up to 10 s, over four rates"""
    seconds = (0.4, 0.975, 1.7, 3.1, 0.9, 5.0, 2.2, 10.0)
    rates = [RATES[i % 4] for i in range(len(seconds))]
    lengths = [15600 if (r == 16000 and s == 0.975) else int(s * r) for s, r in zip(seconds, rates)]
    return ref.varied_clips(9, lengths), rates


def _to_16k(clips, rates, dtype):
    win, nt = resample.kaiser_best()
    return [np.asarray(c if r == 16000 else resample_ref(c, r, 16000, win, nt), dtype) for c, r in zip(clips, rates)]


_CHAIN_REF = {}          # the float64 and float32 references: computed once


@pytest.fixture(scope='module', params=ALGOS)
def chain_case(gpu_required, request):
    if not _CHAIN_REF:
        weights = ref.he_weights(3)
        clips, rates = _chain_clips()
        c64 = _to_16k(clips, rates, np.float64)
        c32 = [c.astype(np.float32) for c in c64]
        _CHAIN_REF.update(weights=weights, clips=clips, rates=rates, e64={}, e32={})
        for hop in (0.96, 0.1, 0.37):
            _CHAIN_REF['e64'][hop] = ref.chain(c64, hop, weights, np.float64)
            _CHAIN_REF['e32'][hop] = ref.chain(c32, hop, weights, np.float32)
        _CHAIN_REF['pca'], _CHAIN_REF['means'] = ref.seeded_pca(_CHAIN_REF['e64'][0.1], 11)
    case = dict(_CHAIN_REF, algo=request.param)
    weights = case['weights']
    case['model'] = vggish.VGGishModel(weights=weights, pca_matrix=case['pca'], pca_means=case['means'], batch=32, conv=request.param)
    yield case
    case['model'].close()


@pytest.mark.parametrize('hop', [0.96, 0.1, 0.37])
def test_chain_unquantised_matches_float64(chain_case, hop):
    c = chain_case
    e64, e32 = c['e64'][hop], c['e32'][hop]
    raw = np.concatenate(c['model'].predict_clips(c['clips'], c['rates'], hop_size=hop, postprocess=False))
    bound = 4 * float(np.abs(e32 - e64).max())
    err = float(np.abs(raw - e64).max())
    print('chain ' + c['algo'] + ' hop %.2f: %d examples (batch 32), |emb| max %.2f, kernel-f64 %.3e, torch32-f64 %.3e, bound %.3e'
          % (hop, e64.shape[0], np.abs(e64).max(), err, bound / 4, bound))
    assert raw.shape == e64.shape and e64.shape[0] == sum(ref.example_count(int(n * 16000.0 / r), hop) for n, r in
                                                           zip([x.size for x in c['clips']], c['rates']))
    assert hop != 0.1 or e64.shape[0] > 32                       # more examples than one batch
    assert err <= bound
    p64, p32 = ref.pca_clip(e64, c['pca'], c['means']), ref.pca_clip(e32, c['pca'], c['means'], np.float32)
    got = np.concatenate(c['model'].predict_clips(c['clips'], c['rates'], hop_size=hop, quantize=False))
    pbound = 4 * float(np.abs(p32 - p64).max())
    perr = float(np.abs(got - p64).max())
    print('chain ' + c['algo'] + ' hop %.2f pca: kernel-f64 %.3e, torch32-f64 %.3e, bound %.3e' % (hop, perr, pbound / 4, pbound))
    assert perr <= pbound


def test_chain_quantised_matches_float64_outside_delta(chain_case):
    c = chain_case
    hop = 0.1
    e64, e32 = c['e64'][hop], c['e32'][hop]
    p64 = ref.pca_clip(e64, c['pca'], c['means'])
    at0, at255, between, distinct = ref.quantiser_coverage(ref.prequant(p64).astype(np.uint8))
    print('quantiser coverage of the float64 output: %.3f at 0, %.3f at 255, %.3f between, %d distinct' % (at0, at255, between, distinct))
    assert at0 >= 0.05 and at255 >= 0.05 and between >= 0.5 and distinct >= 100
    delta = 4 * float(np.abs(ref.pca_clip(e32, c['pca'], c['means'], np.float32) - p64).max()) * 63.75
    q = np.concatenate(c['model'].predict_clips(c['clips'], c['rates'], hop_size=hop, quantize=True))
    left_out, mismatches = ref.quantised_agreement(q, ref.pca_unclipped(e64, c['pca'], c['means']), delta)
    print('chain ' + c['algo'] + ' quantised: delta %.3e, left out %.4f, mismatches outside %d of %d' % (delta, left_out, mismatches, q.size))
    assert q.dtype == np.float32 and q.min() >= 0 and q.max() <= 255 and np.array_equal(q, np.trunc(q))
    assert mismatches == 0 and left_out <= 0.05


def test_many_files_equal_file_by_file_and_runs_are_bit_identical(chain_case, tmp_path):
    import struct
    c = chain_case
    hop = 0.37
    bound = 4 * float(np.abs(c['e32'][hop] - c['e64'][hop]).max())
    paths = []
    for i, (x, r) in enumerate(zip(c['clips'], c['rates'])):
        path = str(tmp_path / ('clip%d.wav' % i))
        data = x.astype('<f4').tobytes()                           # IEEE-float WAV: the samples as they are
        with open(path, 'wb') as fh:
            fh.write(b'RIFF' + struct.pack('<I', 36 + len(data)) + b'WAVEfmt ' + struct.pack('<IHHIIHH', 16, 3, 1, r, 4 * r, 4, 32)
                     + b'data' + struct.pack('<I', len(data)) + data)
        paths.append(path)
    many = c['model'].predict_clips(c['clips'], c['rates'], hop_size=hop, quantize=False)
    again = c['model'].predict_clips(c['clips'], c['rates'], hop_size=hop, quantize=False)
    assert all(np.array_equal(a, b) for a, b in zip(many, again))
    worst = 0.0
    for path, m in zip(paths, many):
        one = vggish.extract_vggish_embedding(path, vggish_model=c['model'], frame_hop_sec=hop, quantize=False)
        assert one.shape == m.shape
        worst = max(worst, float(np.abs(one - m).max()))
    print('many files vs file by file: max difference %.3e (bound %.3e)' % (worst, bound))
    assert worst <= bound


def test_missing_weight_is_an_error_not_a_fallback(gpu_required):
    net = _lib.VGGish(batch=4)
    win, nt = resample.kaiser_best()
    with pytest.raises(_lib.L3Error, match='vggish/conv1/weights was never set'):
        net.embed_clips_resampled(np.zeros(15600, np.float32), [[0, 15600, 16000, 0, 15600, 0]], win, nt, 15600, [[0, 15600]], [0],
                                  'raw')
    with pytest.raises(_lib.L3Error, match='no VGGish variable named'):
        net.set_weight('vggish/conv9/weights', np.zeros(4, np.float32))
    net.close()


def test_handle_filter_tables_follow_the_window_and_the_buffers(gpu_required):
    # the handle keeps its filter tables and its per-call buffers across calls: another half window must not meet the old
    # tables, and a buffer reallocated for a longer call (or for one more table) must not pass for an uploaded one
    weights = _CHAIN_REF.get('weights') or ref.he_weights(3)
    win, nt = resample.kaiser_best()
    short, long_, other = ref.varied_clips(21, [int(1.2 * 44100), 3 * int(1.2 * 44100), int(1.2 * 22050)])

    def embed(net, x, sr, w):
        n16 = resample.output_length(x.size, sr, 16000)
        pads, rows, _ = vggish.example_table([n16], 0.96)
        return net.embed_clips_resampled(x, [[0, x.size, sr, 0, n16, int(pads[0, 0])]], w, nt, int(pads[0, 1]), [[0, int(pads[0, 1])]],
                                         rows, 'raw')

    kept = vggish.VGGishModel(weights=weights, batch=4)
    calls = [(short, 44100, win), (short, 44100, 0.5 * win), (short, 44100, win),
             (long_, 44100, win),               # three times as long: every per-call buffer is reallocated
             (other, 22050, win),               # one more window scale: the table buffer grows
             (short, 44100, win)]
    got = []
    for x, sr, w in calls:
        fresh = vggish.VGGishModel(weights=weights, batch=4)
        got.append(embed(kept.net, x, sr, w))
        want = embed(fresh.net, x, sr, w)
        fresh.close()
        assert got[-1].shape[0] >= 1 and np.array_equal(got[-1], want), (x.size, sr, float(w[0]))
    kept.close()
    assert not np.array_equal(got[0], got[1])              # the window matters to the output: stale tables would show
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[0], got[5])
    assert got[3].shape[0] > got[0].shape[0]
