"""VGGish feature path, host side (no GPU): the float64 restatement against fixtures the reference's own NumPy code wrote
(tests/golden/make_vggish_fixtures.py), the framing table, the .npz loader, the fixed parameters, the fold walkers and the CLI."""
import json
import os
import wave

import numpy as np
import pytest

import vggish_ref as ref
from l3embedding_amd import classifier, cli_embedding_samples, features, usc_generate, vggish

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_restatement_reproduces_reference_logmel_and_examples():
    with np.load(os.path.join(GOLDEN, 'vggish_logmel.npz')) as z, np.load(os.path.join(GOLDEN, 'vggish_examples.npz')) as e:
        lm = ref.log_mel(z['audio'].astype(np.float64))
        assert lm.shape == z['log_mel'].shape and np.abs(lm - z['log_mel']).max() <= 1e-12
        assert np.abs(ref.mel_matrix() - z['mel_matrix']).max() <= 1e-12
        for hop in (0.96, 0.1, 0.37):
            want = e['examples_hop_%s' % hop]
            got = ref.examples(lm, hop)
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
            assert ref.example_count(z['audio'].size, hop) == want.shape[0]


def test_restatement_reproduces_reference_postprocessor_exactly():
    with np.load(os.path.join(GOLDEN, 'vggish_postprocess.npz')) as p:
        q = ref.postprocess(p['embeddings'], p['pca_eigen_vectors'], p['pca_means'])
        assert q.dtype == np.uint8 and np.array_equal(q, p['quantized'])
        assert np.array_equal(ref.postprocess(p['embeddings'], p['pca_eigen_vectors'], p['pca_means'], quantize=False), p['clipped'])


def _boundary_length(hop_size, k):
    """the shortest 16 kHz length with k examples at this hop"""
    return 400 + 160 * (96 + (k - 1) * ref.example_hop(hop_size) - 1)


@pytest.mark.parametrize('hop_size', [0.96, 0.1, 0.37])
def test_example_table_counts_and_pads(hop_size):
    lengths = [1, 15599, 15600, 15601, 16000, 160000, _boundary_length(hop_size, 3) - 1, _boundary_length(hop_size, 3)]
    pads, rows, counts = vggish.example_table(lengths, hop_size)
    assert counts.tolist() == [ref.example_count(n, hop_size) for n in lengths]
    assert counts[-2] == 2 and counts[-1] == 3
    with np.load(os.path.join(GOLDEN, 'vggish_examples.npz')) as e:                     # the reference's own count
        assert vggish.example_table([32000], hop_size)[2][0] == e['examples_hop_%s' % hop_size].shape[0]
    for n, (left, padded) in zip(lengths, pads.tolist()):
        x = ref.pad_clip(np.ones(n))
        assert padded == x.size and left == (int(np.argmax(x)) if n < 15600 else 0)
        assert padded - n - left == (15600 - n) - (15600 - n) // 2 if n < 15600 else left == 0
    # rows: example k of clip i starts k * hop rows into the clip's log-mel, the clips' log-mels back to back
    frames = [ref.frame_count(max(n, 15600)) for n in lengths]
    want = [sum(frames[:i]) + k * ref.example_hop(hop_size) for i in range(len(lengths)) for k in range(counts[i])]
    assert rows.tolist() == want
    assert all(r + 96 <= sum(frames[:i + 1]) for i in range(len(lengths)) for r in rows[sum(counts[:i]):sum(counts[:i + 1])])


def _write_resources(d, drop=None, reshape=None):
    rng = np.random.RandomState(0)
    w = {k: np.zeros(s, np.float32) for k, s in vggish.WEIGHT_SHAPES.items()}
    if drop:
        del w[drop]
    if reshape:
        w[reshape] = w[reshape].reshape(-1)
    np.savez(os.path.join(str(d), 'vggish_model.npz'), **w)
    np.savez(os.path.join(str(d), 'vggish_pca_params.npz'), pca_eigen_vectors=rng.standard_normal((128, 128)),
             pca_means=rng.standard_normal((128, 1)))


def test_loader_names_missing_and_misshaped_tensors(tmp_path):
    with pytest.raises(ValueError, match='vggish_model.npz'):
        vggish.load_weights(str(tmp_path))
    _write_resources(tmp_path)
    w, pca, means = vggish.load_weights(str(tmp_path))
    assert set(w) == set(vggish.WEIGHT_SHAPES) and pca.shape == (128, 128) and means.shape == (128,) and pca.dtype == np.float32
    _write_resources(tmp_path, drop='vggish/conv3/conv3_2/biases')
    with pytest.raises(ValueError, match='vggish/conv3/conv3_2/biases is missing'):
        vggish.load_weights(str(tmp_path))
    _write_resources(tmp_path, reshape='vggish/fc1/fc1_1/weights')
    with pytest.raises(ValueError, match=r'vggish/fc1/fc1_1/weights has shape'):
        vggish.load_weights(str(tmp_path))
    _write_resources(tmp_path)
    np.savez(os.path.join(str(tmp_path), 'vggish_pca_params.npz'), pca_eigen_vectors=np.zeros((128, 64)), pca_means=np.zeros(128))
    with pytest.raises(ValueError, match='pca_eigen_vectors has shape'):
        vggish.load_weights(str(tmp_path))


@pytest.mark.parametrize('name,value', [('target_sample_rate', 8000), ('stft_win_len_sec', 0.05), ('stft_hop_len_sec', 0.02),
                                        ('num_mel_bins', 128), ('mel_min_hz', 0), ('mel_max_hz', 8000), ('frame_win_sec', 1.0),
                                        ('embedding_size', 64)])
def test_fixed_parameters_raise_with_their_name(name, value):
    with pytest.raises(ValueError, match=name):
        vggish.extract_vggish_embedding('nothing.wav', vggish_model=object(), **{name: value})


class StandInVGGish(object):
    """predict_clips(clips, rates, hop_size, quantize): one row per example, [clip length, rate, hop, index] + zeros"""
    def __init__(self):
        self.calls = []

    def predict_clips(self, clips, rates, hop_size=0.1, quantize=True, postprocess=True):
        self.calls.append((len(clips), hop_size, quantize))
        out = []
        for c, r in zip(clips, rates):
            n = int(vggish.example_table([int(c.size * (16000.0 / r))], hop_size)[2][0])
            out.append(np.array([[c.size, r, hop_size, k] for k in range(n)], np.float32))
        return out


def _tone_wav(path, n, rate):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.arange(n) % 200 * 100).astype('<i2').tobytes())


def test_extract_honours_hop_and_quantize_and_features_branches(tmp_path):
    _tone_wav(tmp_path / 'a.wav', 44100, 44100)
    m = StandInVGGish()
    X = vggish.extract_vggish_embedding(str(tmp_path / 'a.wav'), vggish_model=m, frame_hop_sec=0.37, quantize=False)
    assert m.calls == [(1, 0.37, False)] and X.shape[0] == ref.example_count(16000, 0.37)
    assert vggish.extract_vggish_embedding(str(tmp_path / 'a.wav'), vggish_model=m).shape[0] == 1 and m.calls[-1] == (1, 0.96, True)
    X = features.get_vggish_frames_uniform(str(tmp_path / 'a.wav'), hop_size=0.1, vggish_model=m)
    assert m.calls[-1] == (1, 0.1, True) and X.shape[0] == ref.example_count(16000, 0.1)
    X2 = features.compute_file_features(str(tmp_path / 'a.wav'), 'vggish', hop_size=0.1, vggish_model=m)
    assert np.array_equal(X, X2)
    with pytest.raises(ValueError, match='Must provide L3 embedding model to use l3 features'):
        features.compute_file_features(str(tmp_path / 'a.wav'), 'l3')
    with pytest.raises(ValueError, match='Invalid feature type: mfcc'):
        features.compute_file_features(str(tmp_path / 'a.wav'), 'mfcc')


def test_walkers_write_vggish_folds_and_still_refuse_without_a_model(tmp_path):
    data, out = tmp_path / 'esc', tmp_path / 'out'
    for f in range(1, 6):
        os.makedirs(str(data / ('fold%d' % f)))
        for c in (3, 17):
            _tone_wav(data / ('fold%d' % f) / ('%d-1000%d-A-%d.wav' % (f, c, c)), 44100 + f, 44100)
    m = StandInVGGish()
    usc_generate.generate_esc50_folds(str(data), str(out), features='vggish', vggish_model=m, hop_size=0.37)
    assert m.calls == [(2, 0.37, True)] * 5
    with np.load(str(out / 'fold3' / '3-100017-A-17.npz')) as z:
        assert int(z['y']) == 17 and z['X'][0].tolist() == [44103, 44100, np.float32(0.37), 0]
    with pytest.raises(ValueError, match='Invalid feature type'):
        usc_generate.generate_esc50_fold_data(str(data), 0, str(out), features='vggish')
    with pytest.raises(ValueError, match='Invalid feature type'):
        usc_generate.generate_dcase2013_fold_data(str(data), 0, str(out), l3embedding_model=m, features='vggish')


def test_cli_vggish_tree_feeds_classifier_train(tmp_path, monkeypatch, capsys):
    with pytest.raises(SystemExit) as exc:
        cli_embedding_samples.parse_arguments(['-f', 'vggish', 'esc50', 'd', 'o'])
    assert exc.value.code == 2 and 'vggish' in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        cli_embedding_samples.parse_arguments(['esc50', 'd', 'o'])
    assert exc.value.code == 2 and 'model path' in capsys.readouterr().err
    args = cli_embedding_samples.parse_arguments(['-f', 'vggish', '-vrd', 'res', 'esc50', 'd', 'o'])          # no -lmp asked for
    assert args['vggish_resources_dir'] == 'res' and cli_embedding_samples.features_dir(args) == 'o/features/esc50/vggish'

    made = {}

    def fake_model(resources_dir):
        made['dir'] = resources_dir
        return StandInVGGish()

    monkeypatch.setattr(vggish, 'VGGishModel', fake_model)
    data = tmp_path / 'esc'
    for f in range(1, 6):
        os.makedirs(str(data / ('fold%d' % f)))
        for c in range(3):
            for k in range(2):
                _tone_wav(data / ('fold%d' % f) / ('%d-%d%d-A-%d.wav' % (f, c, k, c)), 50000 + 30000 * c, 44100)
    out = cli_embedding_samples.main(['-f', 'vggish', '-vrd', str(tmp_path / 'res'), 'esc50', str(data), str(tmp_path / 'o')])
    assert made['dir'] == str(tmp_path / 'res')
    assert out == str(tmp_path / 'o' / 'features' / 'esc50' / 'vggish')
    assert sorted(os.listdir(out)) == ['config_None.json'] + ['fold%d' % f for f in range(1, 6)]
    with open(os.path.join(out, 'config_None.json')) as fh:
        assert json.load(fh)['features_dir'] == out
    assert len(os.listdir(os.path.join(out, 'fold2'))) == 6

    class FakeMLP(object):
        def __init__(self, D, C, batch, weight_decay=0, seed=0, device=0):
            assert D == 4 and C == 50
            self.batch, self.C = batch, C

        def set_data(self, *a):
            pass

        def epoch(self, perm, lr, t0):
            return dict(loss=1.0, acc=0.0, val_loss=1.0, val_acc=0.0)

        def get_weights(self):
            return [np.zeros(s, np.float32) for s in classifier._lib.mlp_shapes(4, self.C)]

        def set_weights(self, w):
            pass

        def predict(self, x):
            return np.full((len(x), self.C), 1.0 / self.C, np.float32)

        def close(self):
            pass

    monkeypatch.setattr(classifier._lib, 'MLP', FakeMLP)
    run = classifier.train(out, str(tmp_path / 'cls'), 1, model_type='mlp', num_epochs=2)
    assert os.path.exists(os.path.join(run, 'results.pkl'))


def test_float32_path_quantises_like_float64_inside_the_cap():
    """The check the GPU test makes of the kernels, made here of the float32 torch-CPU chain: with the seeded PCA the float64 output
    covers the quantiser, and float32 differs from it only where float64 lies within delta of a truncation step."""
    w = ref.he_weights(3)
    clips = ref.varied_clips(5, (15600, 17200, 16400, 18000, 20000, 16000))
    e64 = ref.chain(clips, 0.1, w, np.float64)
    e32 = ref.chain(clips, 0.1, w, np.float32)
    pca, means = ref.seeded_pca(e64, 11)
    c64, c32 = ref.pca_clip(e64, pca, means), ref.pca_clip(e32, pca, means, np.float32)
    bound = 4 * np.abs(c32 - c64).max()
    at0, at255, between, distinct = ref.quantiser_coverage(ref.prequant(c64).astype(np.uint8))
    assert at0 >= 0.05 and at255 >= 0.05 and between >= 0.5 and distinct >= 100
    q32 = np.trunc(ref.prequant(c32).astype(np.float32))
    left_out, mismatches = ref.quantised_agreement(q32, ref.pca_unclipped(e64, pca, means), bound * 63.75)
    print('float32 chain: pca bound %.3e, delta %.3e, left out %.4f, mismatches %d' % (bound, bound * 63.75, left_out, mismatches))
    assert left_out <= 0.05 and mismatches == 0
