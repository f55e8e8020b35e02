"""The minispec oracle's known answers, the deployed pipeline's framing and the OpenL3 model files, without a GPU
(tests/minispec_ref.py)."""
import bz2
import gzip
import os

import numpy as np
import pytest

import minispec_ref as R
from l3embedding_amd import h5lite, kerasfile, model, openl3

SR = R.SR


def _direct_bin(x, start, n_fft, k):
    """sum over the samples of the frame that lie inside the second: x[n] w[n - start] exp(-2 pi i k (n - start) / n_fft)"""
    n = np.arange(max(start, 0), min(start + n_fft, SR))
    j = (n - start).astype(np.float64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * j / n_fft)
    return np.sum(x[n] * w * np.exp(-2j * np.pi * k * j / n_fft))


def test_impulse_at_sample_0_pins_the_padding():
    """With n_fft / 2 zeros in front, the impulse sits at index 1024 - 242 f of frame f: a flat magnitude equal to the window there
    for f <= 4, nothing from frame 5 on.  Under kapre's 982 zeros it would sit at 982 - 242 f: other window values."""
    x = np.zeros((1, SR))
    x[0, 0] = 1.0
    mag = R.magnitudes(x, 2048)[0]
    w = R.window(2048)
    for f in range(5):
        assert np.abs(mag[f] - w[1024 - 242 * f]).max() < 1e-12, f
        assert abs(w[1024 - 242 * f] - w[982 - 242 * f]) > 1e-3           # the two paddings are told apart
    assert np.abs(mag[5:]).max() == 0.0
    kap = R.magnitudes(x, 2048, pad_left=R.kapre_pad(2048))[0]
    assert R.kapre_pad(2048) == 982 and np.abs(kap[0] - w[982]).max() < 1e-12
    # the linear model: 256 zeros, frames 0 and 1
    mag = R.magnitudes(x, 512)[0]
    w = R.window(512)
    assert np.abs(mag[0] - w[256]).max() < 1e-12 and np.abs(mag[1] - w[14]).max() < 1e-12 and np.abs(mag[2:]).max() == 0.0


@pytest.mark.parametrize('mt', sorted(R.MODELS))
def test_silence_is_all_zeros(mt):
    out = R.minispec(mt, np.zeros((1, SR)))
    assert out.shape == (1, R.MODELS[mt][1] or R.MODELS[mt][0] // 2 + 1, 199, 1)
    assert np.all(out == 0.0)
    assert np.all(R.minispec(mt, np.zeros((1, SR), np.float32), np.float32) == 0.0)


@pytest.mark.parametrize('n_fft', [2048, 512])
def test_edge_frames_of_a_constant_signal_against_the_direct_sum(n_fft):
    x = np.full((1, SR), 0.25)
    mag = R.magnitudes(x, n_fft)[0]
    for f in (0, 1, 2, 3, 4, 195, 196, 197, 198):
        start = f * R.HOP - n_fft // 2
        for k in (0, 1, 7, n_fft // 4, n_fft // 2):
            ref = abs(_direct_bin(x[0], start, n_fft, k))
            assert abs(mag[f, k] - ref) < 1e-9, (f, k)
    assert R.N_FRAMES == 199 and mag.shape == (199, n_fft // 2 + 1)


def test_db_rule_floor_maximum_and_clip():
    p = np.array([[[1.0, 1e-3, 1e-12, 0.0]]])
    db = R.to_db(p)
    assert np.allclose(db[0, 0], [0.0, -30.0, -80.0, -80.0])
    p = np.array([[[1e-9, 1e-12]]])                      # the floor: 10 log10(1e-10) = -100, 10 below the maximum of -90
    assert np.allclose(R.to_db(p)[0, 0], [0.0, -10.0])
    out = R.minispec('cnn_L3_melspec1', R.signals()[1][:2])
    assert out.max() == 0.0 and out.min() >= -80.0


@pytest.mark.parametrize('mt', sorted(R.MODELS))
def test_float32_restatement_and_controls(mt):
    """The float32 restatement stays within the project's front-end bound on noise and tones; every altered reference lies more
    than (CONTROL_MARGIN + 1) bounds from the true one, so a GPU result within the bound is more than CONTROL_MARGIN bounds from it."""
    import frontend_ref as F
    names, a = R.signals()
    a = a[:2]
    ref = R.minispec(mt, a)
    d32 = R.lin_d(R.minispec(mt, a, np.float32), ref)
    print('%s float32 restatement: noise %.2e tones %.2e' % (mt, d32[0], d32[1]))
    assert d32.max() < F.LIN_BOUND
    for variant in ('kapre_pad', 'mel_of_power', 'unsquared'):
        if variant == 'mel_of_power' and not R.MODELS[mt][1]:
            continue                                     # the linear model has no filterbank
        d = R.lin_d(R.minispec(mt, a, variant=variant), ref)
        print('%s control %s: %.2e %.2e' % (mt, variant, d[0], d[1]))
        assert d.max() > (F.CONTROL_MARGIN + 1) * F.LIN_BOUND, (variant, d)


def test_frame_table_rule():
    L = [48000, 48000 * 3 + 17, 95999, 96000]
    table, counts = openl3.frame_table(L)
    assert counts.tolist() == [1, 3, 1, 2]
    off = np.concatenate([[0], np.cumsum(L)[:-1]])
    rows = [(off[i] + k * 48000, off[i], off[i] + L[i]) for i in range(len(L)) for k in range(L[i] // 48000)]
    assert table.tolist() == [list(map(int, r)) for r in rows]
    assert (table[:, 0] + 48000 <= table[:, 2]).all()               # every frame lies inside its clip: nothing is padded
    with pytest.raises(ValueError, match='less than one second'):
        openl3.frame_table([48000, 47999])
    t, c = openl3.frame_table([])
    assert t.shape == (0, 3) and c.size == 0


def test_maps():
    assert dict(openl3.INPUT_REPRS) == {'linear': 'cnn_L3_kapredbinputbn', 'mel128': 'cnn_L3_melspec1', 'mel256': 'cnn_L3_melspec2'}
    for r, mt in openl3.INPUT_REPRS.items():
        h, w, c = model.AUDIO_EMBEDDING_MAP[mt]
        for size, pool in openl3.AUDIO_POOLINGS[r].items():
            assert -(-h // pool[0]) * -(-w // pool[1]) * c == size
        assert set(openl3.AUDIO_POOLINGS[r].values()) == set(model.AUDIO_POOLING[mt].values())
    assert {s: -(-28 // p[0]) * -(-28 // p[1]) * 512 for s, p in openl3.IMAGE_POOLINGS.items()} == {8192: 8192, 512: 512}
    with pytest.raises(ValueError):
        openl3.repr_of('tiny_L3')
    with pytest.raises(ValueError):
        openl3.model_type_of('mel64')


def _host_model(mt, seed=3):
    rng = np.random.RandomState(seed)
    m = model.L3Model(mt)
    W = {n: rng.randn(*s).astype(np.float32) for n, s, _ in m.param_table()}
    m._assign(W)
    return m, W


@pytest.mark.parametrize('mt', sorted(R.MODELS))
def test_extracted_files_structure(tmp_path, mt):
    m, W = _host_model(mt)
    table = m.param_table()
    paths = openl3.extract_models(m, mt, 'env', str(tmp_path))
    r = openl3.repr_of(mt)
    assert {k: os.path.basename(p) for k, p in paths.items()} == {
        'audio': 'openl3_audio_%s_env.h5' % r, 'image': 'openl3_image_%s_env.h5' % r, 'spec': 'openl3_audio_%s_env_spec.h5' % r}
    groups = kerasfile.keras_groups(table, mt)
    flat = {}
    for kind, tower in (('audio', 'audio_model'), ('image', 'vision_model'), ('spec', 'audio_model')):
        root = h5lite.read_file(paths[kind])
        names = [n.decode() for n in root.attrs['layer_names']]
        order = []
        for n, _, _ in table:                                      # the tower's layers in get_weights order
            if n.startswith(tower + '/') and n.split('/')[1] not in order:
                order.append(n.split('/')[1])
        fe = order[0] if tower == 'audio_model' else None
        assert names == (order[1:] if kind == 'spec' else order)
        assert list(root.children) == names or sorted(root.children) == sorted(names)
        flat[kind] = []
        for ln in names:
            wn = [w.decode() for w in root[ln].attrs['weight_names']]
            want = [kerasfile._tf_name(p) for p in groups[tower] if p.split('/')[1] == ln]
            assert wn == want, ln
            for w in wn:
                p = tower + '/' + w[:-2].replace('/Variable', '/freq2mel')
                assert np.array_equal(root[ln + '/' + w], W[p])
            flat[kind] += [ln + '/' + w for w in wn]
        if kind == 'audio':
            n_const = 3 if R.MODELS[mt][1] else 2
            assert names[0] == fe and fe.endswith('spectrogram_1')
            assert [w.split('/')[-1] for w in flat[kind][:n_const]] == ['real_kernels:0', 'imag_kernels:0', 'Variable:0'][:n_const]
        if kind == 'spec':
            assert not any('spectrogram' in w or 'kernels' in w for w in flat[kind])
    n_const = 3 if R.MODELS[mt][1] else 2           # the linear model's Spectrogram layer holds two constants, the mel models' three
    assert flat['spec'] == flat['audio'][n_const:]
    assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(p) for p in paths.values())       # no copies unasked
    # read back by layer and weight name, also from below model_weights/
    for src in (paths['audio'], paths['spec']):
        got = openl3._tower_weights(src, table, mt, 'audio_model', optional=(fe,))
        assert all(np.array_equal(v, W[k]) for k, v in got.items())
        assert len(got) == len(flat['spec' if '_spec' in src else 'audio'])
    root = h5lite.read_file(paths['image'])
    outer = h5lite.Group()
    outer.children['model_weights'] = root
    saved = str(tmp_path / 'saved_model.h5')
    h5lite.write_file(saved, outer)
    got = openl3._tower_weights(saved, table, mt, 'vision_model')
    assert len(got) == len(flat['image']) and all(np.array_equal(v, W[k]) for k, v in got.items())
    with pytest.raises(ValueError):
        openl3._tower_weights(paths['image'], table, mt, 'audio_model', optional=(fe,))


def test_compressed_copies_are_written_and_read(tmp_path, monkeypatch):
    """gzip and bz2 copies beside every file when `compress` asks for them, byte for byte the file, and read like it.  The towers
    are cut down to their first weighted layers here: compressing three whole models takes half a minute."""
    mt = 'cnn_L3_kapredbinputbn'
    m, W = _host_model(mt)
    full = openl3.tower_layers
    monkeypatch.setattr(openl3, 'tower_layers', lambda *a: type(full(*a))(list(full(*a).items())[:3]))
    paths = openl3.extract_models(m, mt, 'music', str(tmp_path), compress=('gzip', 'bz2'))
    assert len(os.listdir(str(tmp_path))) == 9
    for p in paths.values():
        raw = open(p, 'rb').read()
        assert gzip.open(p + '.gz').read() == raw and bz2.BZ2File(p + '.bz2').read() == raw
        for suffix in ('.gz', '.bz2'):
            got, want = openl3.read_flat(p + suffix), openl3.read_flat(p)
            assert list(got) == list(want) and all(np.array_equal(got[ln][w], want[ln][w]) for ln in want for w in want[ln])


def test_extract_refuses_other_models(tmp_path):
    with pytest.raises(ValueError):
        openl3.extract_models(model.L3Model('cnn_L3_orig'), 'cnn_L3_orig', 'env', str(tmp_path))
    m, _ = _host_model('cnn_L3_melspec1')
    with pytest.raises(ValueError):
        openl3.extract_models(m, 'cnn_L3_melspec2', 'env', str(tmp_path))
    with pytest.raises(ValueError):
        openl3.extract_models(m, 'cnn_L3_melspec1', 'env', str(tmp_path), compress=('zip',))


def test_config_struct_grows_at_its_end():
    """`frontend` is the last field of l3_config; the struct before it is the old struct, byte for byte"""
    import ctypes
    from l3embedding_amd import _lib
    assert _lib.L3Config2.frontend.offset == ctypes.sizeof(_lib.L3Config) == 48 and ctypes.sizeof(_lib.L3Config2) == 56
    assert all(getattr(_lib.L3Config2, n).offset == getattr(_lib.L3Config, n).offset for n, _ in _lib.L3Config._fields_)
    assert _lib.FRONTENDS == {'kapre': 0, 'minispec': 1}


def test_python_options_are_checked_without_an_engine():
    with pytest.raises(ValueError):
        model.L3Model('cnn_L3_melspec2', frontend='librosa')
    m = model.L3Model('cnn_L3_melspec2', frontend='minispec')
    assert m.frontend == 'minispec'
    m.set_frontend('kapre')
    assert m.frontend == 'kapre'
    from l3embedding_amd import cli_classify
    args = cli_classify.build_parser().parse_args(['--model-dir', 'd', '--weights', 'w', '--model-type', 'cnn_L3_melspec2',
                                                   '--frontend', 'minispec', 'a.wav'])
    assert args.frontend == 'minispec'
    assert cli_classify.build_parser().parse_args(['--model-dir', 'd', '--weights', 'w', '--model-type', 'x', 'a.wav']).frontend == 'kapre'
