"""The sound classifier's host side (l3embedding_amd/sound.py): SoundClassifier.from_run's reading of a run directory for the three
model types, the unfitted min-max scaler, the width check that runs before anything else, the NumPy reference of the per-file mean
against hand-worked values, and the bindings of the new library entries.  No GPU is touched."""
import json
import os
import pickle

import numpy as np
import pytest

import sound_ref
from l3embedding_amd import _lib, classifier, forest, model, sound, svm, usc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 512


def _embedding(pooling='short', mt='cnn_L3_melspec2'):
    return model.EmbeddingModel(model.L3Model(mt), 'audio', model.AUDIO_POOLING[mt][pooling])


def _scalers(width, min_max=True, seed=0):
    r = np.random.RandomState(seed)
    mm = usc.MinMaxScaler()
    if min_max:
        mm.fit(r.randn(5, D).astype(np.float32))
    return mm, usc.StandardScaler().fit(r.randn(5, width).astype(np.float32))


def _fitted_stub(kind, width, n_classes=3):
    """a model with the attributes a fit leaves that from_run and the width check read; it never predicts here"""
    if kind == 'svm':
        clf = svm.SVC(probability=True)
        clf.support_, clf.shape_fit_, clf.classes_ = np.zeros(1, np.int64), (60, width), np.arange(n_classes)
    else:
        clf = forest.RandomForestClassifier(n_estimators=2)
        clf.estimators_, clf.n_features_, clf.classes_, clf.n_classes_ = [], width, np.arange(n_classes), n_classes
    return clf


def _run_dir(path, kind, width, min_max=True, **config):
    os.makedirs(str(path), exist_ok=True)
    cfg = dict(model_type=kind, feature_mode='framewise', non_overlap=False, non_overlap_chunk_size=10)
    cfg.update(config)
    with open(os.path.join(str(path), 'config.json'), 'w') as fh:
        json.dump(cfg, fh)
    for name, scaler in zip(('min_max_scaler.pkl', 'stdizer.pkl'), _scalers(width, min_max)):
        with open(os.path.join(str(path), name), 'wb') as fh:
            pickle.dump(scaler, fh)
    if kind == 'mlp':
        m = classifier.MLPModel(width, num_classes=7, seed=3)
        r = np.random.RandomState(4)
        m.set_weights([r.randn(*s).astype(np.float32) for s in _lib.mlp_shapes(width, 7)])
        m.save_weights(os.path.join(str(path), 'model.h5'))
    else:
        with open(os.path.join(str(path), 'model.pkl'), 'wb') as fh:
            pickle.dump(_fitted_stub(kind, width), fh)
    return str(path)


@pytest.mark.parametrize('kind', ['mlp', 'svm', 'rf'])
def test_from_run_reads_the_three_model_types(tmp_path, kind):
    sc = sound.SoundClassifier.from_run(_embedding(), _run_dir(tmp_path / kind, kind, D, non_overlap=True, non_overlap_chunk_size=3),
                                        hop_size=0.5)
    assert sc.kind == kind and sc.feature_mode == 'framewise'
    assert sc.non_overlap is True and sc.non_overlap_chunk_size == 3 and sc.hop_length == 24000
    assert sc.min_max_scaler is not None and sc.min_max_scaler.scale_.shape == (D,)
    assert sc.stdizer.mean_.shape == (D,)
    want = {'mlp': classifier.MLPModel, 'svm': svm.SVC, 'rf': forest.RandomForestClassifier}[kind]
    assert isinstance(sc.classifier, want) and sc.device == 0
    if kind == 'mlp':
        assert sc.classifier.input_dim == D and sc.classifier.num_classes == 7
        r = np.random.RandomState(4)
        for got, shp in zip(sc.classifier.get_weights(), _lib.mlp_shapes(D, 7)):
            assert np.array_equal(got, r.randn(*shp).astype(np.float32))


def test_from_run_stats_mode_takes_seven_blocks(tmp_path):
    sc = sound.SoundClassifier.from_run(_embedding(), _run_dir(tmp_path / 'run', 'svm', 7 * D, feature_mode='stats'))
    assert sc.feature_mode == 'stats' and sc.stdizer.scale_.shape == (7 * D,)


def test_from_run_leaves_an_unfitted_min_max_scaler_out(tmp_path):
    sc = sound.SoundClassifier.from_run(_embedding(), _run_dir(tmp_path / 'run', 'mlp', D, min_max=False))
    assert sc.min_max_scaler is None
    assert sound.SoundClassifier(_embedding(), sc.classifier, sc.stdizer, min_max_scaler=usc.MinMaxScaler()).min_max_scaler is None


def test_from_run_refuses_an_unknown_model_type(tmp_path):
    with pytest.raises(ValueError, match='model_type'):
        sound.SoundClassifier.from_run(_embedding(), _run_dir(tmp_path / 'run', 'svm', D, model_type='knn'))


def test_width_mismatch_is_refused_before_anything_runs(tmp_path):
    mm, std = _scalers(D)
    wide = _embedding('original')                 # 6144 columns
    assert wide.embedding_dim() == 6144 and _embedding().embedding_dim() == D
    assert _embedding('original', 'cnn_L3_melspec1').embedding_dim() == 6144
    with pytest.raises(ValueError, match='takes 512 features per row; the embedding gives 6144'):
        sound.SoundClassifier(wide, classifier.MLPModel(D, num_classes=10), std)
    with pytest.raises(ValueError, match=r'takes 512 features per row; the embedding gives 3584 \(7 statistics of 512\)'):
        sound.SoundClassifier(_embedding(), _fitted_stub('svm', D), std, feature_mode='stats')
    with pytest.raises(ValueError, match='takes 512 features per row; the embedding gives 6144'):
        sound.SoundClassifier.from_run(wide, _run_dir(tmp_path / 'run', 'rf', D))
    with pytest.raises(ValueError, match='stdizer was fitted on'):
        sound.SoundClassifier(_embedding(), classifier.MLPModel(D), _scalers(D + 1)[1])
    with pytest.raises(ValueError, match='feature_mode'):
        sound.SoundClassifier(_embedding(), classifier.MLPModel(D), std, feature_mode='mean')
    with pytest.raises(ValueError, match='probability=False'):
        stub = _fitted_stub('svm', D)
        stub.probability = False
        sound.SoundClassifier(_embedding(), stub, std)
    with pytest.raises(TypeError, match='audio embedding'):
        sound.SoundClassifier(object(), classifier.MLPModel(D), std)
    # nothing above made an engine or a device handle
    assert wide.base._engine is None


def test_sound_ref_against_hand_worked_means():
    probs = np.array([[0.25, 0.75], [0.5, 0.5], [1.0, 0.0], [0.125, 0.875]], np.float32)
    mean, pred = sound_ref.file_mean(probs, [[0, 2], [2, 3], [0, 4], [1, 2]])
    assert mean.dtype == np.float32
    assert np.array_equal(mean, np.array([[0.375, 0.625], [1.0, 0.0], [0.46875, 0.53125], [0.5, 0.5]], np.float32))
    assert pred.tolist() == [1, 0, 1, 0]          # the last file ties: the lower class
    # a float32 sum in row order, not a wider or a pairwise one: 2^24 + 1 + 1 stays 2^24 in float32
    big = np.array([[16777216.0], [1.0], [1.0]], np.float32)
    assert sound_ref.file_mean(big, [[0, 3]])[0][0, 0] == np.float32(16777216.0) / np.float32(3)


@pytest.mark.parametrize('C', [2, 3, 10, 50, 64])
def test_sound_ref_is_numpys_mean_and_its_case_ties(C):
    probs, files = sound_ref.file_mean_case(C)
    assert probs.dtype == np.float32 and files[:, 1].max() == probs.shape[0]
    assert sorted((files[:, 1] - files[:, 0]).tolist()) == [1, 2, 2, 63, 64, 65, 1000]
    mean, pred = sound_ref.file_mean(probs, files)
    for (s, e), m, p in zip(files, mean, pred):
        assert np.array_equal(probs[s:e].mean(axis=0), m)
        assert probs[s:e].mean(axis=0).argmax() == p
    top = np.sort(mean[-1])[-2:]
    assert top[0] == top[1] and pred[-1] == np.flatnonzero(mean[-1] == top[1])[0] < np.flatnonzero(mean[-1] == top[1])[1]
    assert np.array_equal(pred, classifier._file_predictions(probs, files))


def test_the_new_entries_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, 'include', 'l3hip.h')) as fh:
        header = fh.read()
    lib = _lib.load()
    for entry in ('l3_feat_alloc', 'l3_embed_audio_frames_dev', 'l3_embed_audio_clips_resampled_dev', 'l3_mlp_predict_files_dev',
                  'l3_op_file_mean'):
        assert entry in _lib.SIGNATURES and entry + '(' in header, entry
        args = header[header.index(entry + '('):].split(';', 1)[0]
        assert len(args.split(',')) == len(_lib.SIGNATURES[entry][1]), entry
        assert getattr(lib, entry).argtypes == _lib.SIGNATURES[entry][1]
    # the _dev twins take their host twins' arguments with (dst, row0) in place of out
    for host in ('l3_embed_audio_frames', 'l3_embed_audio_clips_resampled'):
        assert _lib.SIGNATURES[host + '_dev'][1][:-2] == _lib.SIGNATURES[host][1][:-1]
