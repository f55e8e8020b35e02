"""Audio clips classified end to end on the GPU from resident embeddings (l3embedding_amd/sound.py; notebooks/pimodel.ipynb,
data/usc/features.py:256-306): pooled rows written into a device matrix against the host form's rows (bit for bit, nothing outside
the row range), the per-file mean kernel against NumPy, MLPModel.predict_files, and SoundClassifier against the existing pieces run
on host rows, framewise and in stats mode, from a run directory and from the command line."""
import importlib.util
import io
import json
import os
import pickle
import wave

import numpy as np
import pytest

import sound_ref
from l3embedding_amd import _lib, classifier, cli_classify, features, forest, model, resample, sound, svm, usc
from sound_ref import HOP, LENGTHS, F

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
MT = 'cnn_L3_melspec2'
SENTINEL = np.float32(-1234.5)


def _mod():
    spec = importlib.util.spec_from_file_location('make_golden', os.path.join(GOLDEN, 'make_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _embedding(mt, pooling, batch, scope='sample', dtype='f32'):
    m = model.L3Model(mt, db_max_scope=scope)
    m.compute_dtype = dtype
    m._ensure_engine(batch).set_params(_mod().perturbed_params(mt, 71))
    return model.EmbeddingModel(m, 'audio', model.AUDIO_POOLING[mt][pooling])


# ---- 1. resident rows are the host rows ------------------------------------------------------------------------------------------
# the 0- and 100-sample clips stay at 48 kHz: resampy refuses an output of no samples
RATES = [44100, 48000, 8000, 48000, 44100, 8000]
CASES = [   # model, pooling, engine batch, db_max_scope, dtype, rates
    (MT, 'original', 2, 'sample', 'f32', None),
    (MT, 'short', 3, 'sample', 'f32', None),
    (MT, 'original', 3, 'batch', 'f32', None),
    ('cnn_L3_orig', 'original', 3, 'sample', 'f32', None),
    (MT, 'original', 3, 'sample', 'bf16', None),
    (MT, 'short', 3, 'sample', 'f32', RATES),
]


@pytest.mark.parametrize('mt,pooling,batch,scope,dtype,rates', CASES)
def test_resident_rows_equal_host_rows(gpu_required, mt, pooling, batch, scope, dtype, rates):
    em = _embedding(mt, pooling, batch, scope, dtype)
    clips = sound_ref.clips(LENGTHS, 2)
    host = em.predict_clips(clips, HOP, rates=rates)
    dev, file_idxs = em.predict_clips(clips, HOP, rates=rates, to_device=True)
    assert isinstance(dev, usc.DeviceFeatures) and em.base._engine.batch == batch
    assert np.array_equal(file_idxs, usc._row_ranges([len(h) for h in host]))
    assert dev.shape == (sum(len(h) for h in host), em.embedding_dim())
    assert em.embedding_dim() == em.output_shape[1]
    assert np.array_equal(dev.to_host(), np.concatenate(host))
    dev.close()


# ---- 2. / 3. the row range and the argument errors ---------------------------------------------------------------------------------
@pytest.mark.parametrize('pooling,B', [('original', 3), ('short', 2)])          # the windowed and the global pooling kernel
def test_nothing_is_written_outside_the_row_range(gpu_required, pooling, B):
    eng = _lib.Engine(MT, B)
    eng.set_params(_mod().perturbed_params(MT, 71))
    pool = model.AUDIO_POOLING[MT][pooling]
    clips = sound_ref.clips([F + 4 * HOP + 7, 100, F], 3)
    table, counts = features.frame_table([len(c) for c in clips], HOP)
    n = int(counts.sum())
    assert n == 7 and n % B != 0
    samples = np.concatenate(clips)
    want = eng.embed_audio_frames(samples, table, pool)
    D = want.shape[1]
    total, row0 = n + 2 * B + 5, B + 2
    dst = _lib.Features(np.full((total, D), SENTINEL, np.float32))
    assert eng.embed_audio_frames(samples, table, pool, dst=dst, row0=row0) is dst
    got = dst.download()
    assert np.array_equal(got[row0:row0 + n], want)
    assert np.all(got[:row0] == SENTINEL) and np.all(got[row0 + n:] == SENTINEL)
    dst.close()
    eng.close()


def test_destination_errors_leave_the_destination_alone(gpu_required):
    eng = _lib.Engine(MT, 2)
    pool = model.AUDIO_POOLING[MT]['short']
    clip = sound_ref.clips([F + HOP], 4)[0]
    table, _ = features.frame_table([len(clip)], HOP)          # two frames
    win, nt = resample.get_filter('kaiser_best')
    desc = np.array([[0, len(clip), 48000, 0, len(clip), 0]], np.int64)
    for D, row0, why in ((516, 0, 'columns'), (512, -1, 'outside'), (512, 4, 'outside')):
        dst = _lib.Features(np.full((5, D), SENTINEL, np.float32))
        with pytest.raises(_lib.L3Error, match='error -1: l3_embed_audio_frames_dev: .*' + why):
            eng.embed_audio_frames(clip, table, pool, dst=dst, row0=row0)
        with pytest.raises(_lib.L3Error, match='error -1: l3_embed_audio_clips_resampled_dev: .*' + why):
            eng.embed_audio_clips_resampled(clip, desc, win, nt, len(clip), table, pool, dst=dst, row0=row0)
        assert np.all(dst.download() == SENTINEL)
        dst.close()
    assert eng.lib.l3_embed_audio_frames_dev(eng.h, clip.ctypes.data, len(clip), table.ctypes.data, 2, pool[0], pool[1], None, 0) == -1
    assert b'dst must not be NULL' in eng.lib.l3_last_error(eng.h)
    ok = _lib.Features.alloc(5, 512)
    assert np.all(ok.download() == 0)
    eng.embed_audio_frames(clip, table, pool, dst=ok, row0=3)          # the last two rows: the range may end at n
    got = ok.download()
    assert np.all(got[:3] == 0) and np.array_equal(got[3:], eng.embed_audio_frames(clip, table, pool))
    ok.close()
    with pytest.raises(_lib.L3Error, match='error -1: l3_feat_alloc'):
        _lib.Features.alloc(0, 512)
    eng.close()


# ---- 4. the per-file mean kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [2, 3, 10, 50, 64])
def test_file_mean_op_is_numpys_mean_and_argmax(gpu_required, C):
    probs, files = sound_ref.file_mean_case(C)
    want_mean, want_pred = sound_ref.file_mean(probs, files)
    mean, pred = _lib.op_file_mean(probs, files)
    assert mean.dtype == np.float32 and pred.dtype == np.int32
    assert np.array_equal(mean, want_mean) and np.array_equal(pred, want_pred)
    # files in another order, overlapping: each is reduced on its own
    other = np.array([[5, 1005], [0, 1], [3, 70], [files[-1, 0], files[-1, 1]]], np.int64)
    mean, pred = _lib.op_file_mean(probs, other)
    want_mean, want_pred = sound_ref.file_mean(probs, other)
    assert np.array_equal(mean, want_mean) and np.array_equal(pred, want_pred)


def test_file_mean_op_rejects_bad_input(gpu_required):
    probs = np.full((4, 3), 1 / 3, np.float32)
    for files, why in (([[0, 5]], 'file 0'), ([[0, 2], [2, 2]], 'file 1'), ([[-1, 2]], 'file 0'), (np.zeros((0, 2)), 'n_files')):
        with pytest.raises(_lib.L3Error, match='error -1: l3_op_file_mean: .*' + why):
            _lib.op_file_mean(probs, files)
    with pytest.raises(_lib.L3Error, match='error -1: l3_op_file_mean: .*class count'):
        _lib.op_file_mean(np.zeros((2, 65), np.float32), [[0, 2]])


# ---- 5. MLPModel.predict_files -------------------------------------------------------------------------------------------------------
def test_mlp_predict_files_equals_the_host_loop(gpu_required):
    r = np.random.RandomState(7)
    sizes = [1, 2, 63, 64, 65, 1000, 5]
    X = r.randn(sum(sizes), 512).astype(np.float32)
    file_idxs = usc._row_ranges(sizes)
    m = classifier.MLPModel(512, num_classes=10, seed=5)
    probs = m.predict(X)
    dev = usc.DeviceFeatures(X)
    mean, pred = m.predict_files(dev, file_idxs)
    assert mean.dtype == np.float32 and mean.shape == (len(sizes), 10)
    assert np.array_equal(pred, classifier._file_predictions(probs, file_idxs))
    assert np.array_equal(mean, np.stack([probs[s:e].mean(axis=0) for s, e in file_idxs]))
    assert np.array_equal(dev.to_host(), X)          # the matrix is only read
    with pytest.raises(_lib.L3Error, match='error -1: l3_mlp_predict_files_dev: .*file 0'):
        m.predict_files(dev, [[0, len(X) + 1]])
    with pytest.raises(TypeError):
        m.predict_files(X, file_idxs)
    dev.close()


# ---- 6. / 7. end to end ---------------------------------------------------------------------------------------------------------------
_E2E = {}


@pytest.fixture(scope='module')
def e2e(gpu_required):
    """the embedding (cnn_L3_melspec2, 'short': D = 512, engine batch 3), the six clips and their host rows, once"""
    if not _E2E:
        em = _embedding(MT, 'short', 3)
        clips = sound_ref.clips(LENGTHS, 2)
        host = em.predict_clips(clips, HOP)
        _E2E.update(em=em, clips=clips, X=np.concatenate(host), file_idxs=usc._row_ranges([len(h) for h in host]))
    return _E2E


def _models(width, seed=9):
    """kind -> a trained classifier of `width` inputs: a seeded MLP of 10 classes; an SVC and a forest on 60 seeded rows of 3 classes"""
    r = np.random.RandomState(seed)
    rows = r.randn(60, width).astype(np.float32)
    labels = np.arange(60) % 3
    return {
        'mlp': classifier.MLPModel(width, num_classes=10, seed=11),
        'svm': svm.SVC(probability=True, random_state=0).fit(rows, labels),
        'rf': forest.RandomForestClassifier(n_estimators=8, random_state=0).fit(rows, labels),
    }


def _mean_and_argmax(probs, file_idxs, classes=None):
    mean = np.stack([probs[s:e].mean(axis=0) for s, e in file_idxs])
    pred = classifier._file_predictions(probs, file_idxs)
    return mean, pred if classes is None else classes[pred]


# Which yardstick each model gets in the framewise test.
#   mlp, rf: the existing path on HOST rows -- predict_clips to the host, MinMaxScaler.transform / StandardScaler.transform in NumPy,
#       predict / predict_proba on the host rows, NumPy's per-file mean and arg-max.  Both models score host rows and device rows with
#       the same kernels (l3_mlp_predict / _dev; l3_forest_predict_proba / l3_forest_score), so the bits agree.
#   svm: SVC.predict_proba on host rows couples the pairwise probabilities in NumPy, evaluate() couples them on the device, and the two
#       agree to rounding only (tests/test_svm_eval_gpu.py compares them with _proba_close, not bit for bit).  So the SVM is compared
#       with the same model's evaluate() on DeviceFeatures(host rows after the host transforms): the device scoring on the host
#       path's rows, which leaves the resident embedding and the device transforms as what the comparison tests.
@pytest.mark.parametrize('kind', ['mlp', 'svm', 'rf'])
@pytest.mark.parametrize('min_max,non_overlap', [(True, False), (False, False), (True, True)])
def test_framewise_end_to_end_equals_the_existing_path(e2e, kind, min_max, non_overlap):
    X, file_idxs = e2e['X'], e2e['file_idxs']
    if 'models' not in e2e:
        e2e['models'] = _models(512)
    clf = e2e['models'][kind]
    mm = usc.MinMaxScaler().fit(X) if min_max else usc.MinMaxScaler()
    std = usc.StandardScaler().fit(mm.transform(X) if min_max else X)
    sc = sound.SoundClassifier(e2e['em'], clf, std, min_max_scaler=mm, non_overlap=non_overlap, non_overlap_chunk_size=2,
                               hop_size=HOP / 48000.0)
    got = sc.predict_clips(e2e['clips'])
    # the existing path on host rows
    rows, idxs = X, file_idxs
    if non_overlap:
        keep, idxs = usc.non_overlap_rows(file_idxs, 2)
        rows = X[keep]
        assert len(rows) < len(X)
    if min_max:
        rows = mm.transform(rows)
    rows = std.transform(rows)
    assert rows.dtype == np.float32
    if kind == 'mlp':
        want_proba, want_pred = _mean_and_argmax(clf.predict(rows), idxs)
    elif kind == 'rf':
        want_proba, want_pred = _mean_and_argmax(clf.predict_proba(rows), idxs, clf.classes_)
    else:
        on_dev = usc.DeviceFeatures(rows)
        ref = clf.evaluate(on_dev, file_idxs=idxs, outputs=('file_proba', 'file_predict'))
        on_dev.close()
        want_proba, want_pred = ref['file_proba'], ref['file_predict']
    assert got['file_proba'].shape == (len(LENGTHS), 10 if kind == 'mlp' else 3)
    assert got['file_proba'].dtype == want_proba.dtype
    assert np.array_equal(got['file_proba'], want_proba)
    assert np.array_equal(got['file_predict'], want_pred)


@pytest.mark.parametrize('kind', ['mlp', 'svm', 'rf'])
def test_stats_mode_end_to_end_equals_the_device_pieces(e2e, kind):
    X, file_idxs = e2e['X'], e2e['file_idxs']
    if 'stats' not in e2e:
        # the existing device pieces on uploaded host embeddings, up to the standardiser they fit
        mm = usc.MinMaxScaler().fit(X)
        ref = usc.DeviceFeatures(X)
        ref.handle.affine32(mm.scale_, mm.min_)
        ref.handle.file_stats(file_idxs)
        std = usc.StandardScaler().fit(ref.to_host())
        ref.handle.standardize(std.mean_, std.scale_)
        e2e['stats'] = dict(mm=mm, std=std, rows=ref.to_host(), models=_models(7 * 512, seed=10))
        ref.close()
    st = e2e['stats']
    clf = st['models'][kind]
    one_row = usc._row_ranges(np.ones(len(file_idxs), dtype=np.int64))
    ref = usc.DeviceFeatures(st['rows'])
    assert ref.shape == (len(LENGTHS), 7 * 512)
    if kind == 'mlp':
        want_proba, want_pred = _mean_and_argmax(clf.predict(ref), one_row)
    elif kind == 'svm':
        got_ref = clf.evaluate(ref, file_idxs=one_row, outputs=('file_proba', 'file_predict'))
        want_proba, want_pred = got_ref['file_proba'], got_ref['file_predict']
    else:
        got_ref = clf.evaluate(ref, file_idxs=one_row, outputs=('file_mean', 'file_predict'))
        want_proba, want_pred = got_ref['file_mean'][0], got_ref['file_predict'][0]
    ref.close()
    sc = sound.SoundClassifier(e2e['em'], clf, st['std'], min_max_scaler=st['mm'], feature_mode='stats', hop_size=HOP / 48000.0)
    got = sc.predict_clips(e2e['clips'])
    assert np.array_equal(got['file_proba'], want_proba) and np.array_equal(got['file_predict'], want_pred)


# ---- 8. a run directory and the command line --------------------------------------------------------------------------------------------
def _wav(path, pcm, rate):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.astype('<i2').tobytes())
    return str(path)


def test_from_run_and_the_command_line(e2e, tmp_path, capsys):
    X = e2e['X']
    weights = str(tmp_path / 'l3.h5')
    e2e['em'].base.save_weights(weights)
    run = tmp_path / 'run'
    run.mkdir()
    (run / 'config.json').write_text(json.dumps(dict(model_type='mlp', feature_mode='framewise', non_overlap=False,
                                                     non_overlap_chunk_size=10)))
    mm = usc.MinMaxScaler().fit(X)
    for name, scaler in (('min_max_scaler.pkl', mm), ('stdizer.pkl', usc.StandardScaler().fit(mm.transform(X)))):
        (run / name).write_bytes(pickle.dumps(scaler))
    mlp = classifier.MLPModel(512, num_classes=10, seed=11)
    mlp.save_weights(str(run / 'model.h5'))
    r = np.random.RandomState(5)
    paths = [_wav(tmp_path / 'a.wav', r.randint(-20000, 20000, size=(24000, 2)), 48000),          # 0.5 s stereo: one frame
             _wav(tmp_path / 'b.wav', r.randint(-20000, 20000, size=(28665, 1)), 22050)]          # 1.3 s mono: four frames
    em = model.load_embedding(weights, MT, 'audio', 'short')
    sc = sound.SoundClassifier.from_run(em, str(run), hop_size=HOP / 48000.0)
    assert sc.kind == 'mlp' and sc.min_max_scaler is not None
    for a, b in zip(sc.classifier.get_weights(), mlp.get_weights()):
        assert np.array_equal(a, b)
    by_file = sc.predict_files(paths)
    read = [features.read_wav(p) for p in paths]
    by_clip = sc.predict_clips([x for x, _ in read], rates=[sr for _, sr in read])
    assert by_file['file_proba'].shape == (2, 10)
    for k in ('file_proba', 'file_predict'):
        assert np.array_equal(by_file[k], by_clip[k])
    out = io.StringIO()
    cli_classify.main(['--model-dir', str(run), '--weights', weights, '--model-type', MT, '--pooling-type', 'short'] + paths, out=out)
    lines = [json.loads(line) for line in out.getvalue().splitlines()]
    assert [d['path'] for d in lines] == paths
    assert [d['class'] for d in lines] == by_file['file_predict'].tolist()
    assert all(len(d['proba']) == 10 for d in lines)
    assert np.array_equal(np.array([d['proba'] for d in lines], np.float32), by_file['file_proba'])
