"""The parameter search without a validation fold on the GPU: l3_feat_split (csrc/featprep.hip) against NumPy's integer indexing bit
for bit, and classifier.cross_validate / train / train_svm_fold with parameter_search_valid_fold=False and a split seed on splits
that stay resident: the folds against separate per-fold calls, the parts the fits receive against X[train_idx] / X[valid_idx], no
download during the search, and every matrix the search made closed afterwards.  Every comparison is for equal bits: the cut is a
copy, and everything after it is the existing code on an identical matrix."""
import ctypes as C
import os

import numpy as np
import pytest

from param_split_ref import GRID_POINTS, load_config, load_pickle, write_tree
from l3embedding_amd import _lib, classifier, usc

pytestmark = pytest.mark.gpu

DS = [1, 5, 8, 24, 6144]          # 4-byte pieces (1, 5), 16-byte pieces in flat runs (8, 24), a row longer than one wave's span
ROWS = [3, 257, 3000]             # 64 rows for D = 6144


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _source(n, D, seed=0):
    # distinct bit patterns, signed zeros and denormals included: a copy must not touch any of them
    r = np.random.RandomState(1000 * seed + D + n)
    x = r.randn(n, D).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] = np.float32(-0.0)
    flat[3::11] = np.float32(1e-42)
    return x


def _tables(n):
    """name -> (rows_a, rows_b or None)"""
    r = np.random.RandomState(n)
    perm = r.permutation(n)
    cut = max(1, int(0.85 * n))
    return {
        'a permutation cut at 85 %': (perm[:cut], perm[cut:]),
        'reversed': (np.arange(n - 1, -1, -1)[:cut], np.arange(n - 1, -1, -1)[cut:]),
        'repeats, longer than the source': (r.randint(0, n, 2 * n + 5), r.randint(0, n, n + 1)),
        'a single row': (np.array([n - 1]), np.array([0])),
        'n_b = 0': (perm, None),
        'n_b = 0, an empty table': (perm[:cut], np.zeros(0, np.int64)),
    }


def _check_split(src, x, rows_a, rows_b, name):
    a, b = src.split(rows_a, rows_b)
    try:
        assert a.shape == (len(rows_a), x.shape[1]) and a.device == src.device, name
        np.testing.assert_array_equal(_bits(a.download()), _bits(x[rows_a]), err_msg=name + ': A')
        if rows_b is None or len(rows_b) == 0:
            assert b is None, name
        else:
            assert b.shape == (len(rows_b), x.shape[1]) and b.device == src.device, name
            np.testing.assert_array_equal(_bits(b.download()), _bits(x[rows_b]), err_msg=name + ': B')
    finally:
        a.close()
        if b is not None:
            b.close()
    np.testing.assert_array_equal(_bits(src.download()), _bits(x), err_msg=name + ': the source')          # as it was


@pytest.mark.parametrize('D', DS)
def test_split_equals_indexing(gpu_required, D):
    for n in ([64] if D == 6144 else ROWS):
        x = _source(n, D)
        src = _lib.Features(x, device=0)
        try:
            for name, (rows_a, rows_b) in _tables(n).items():
                _check_split(src, x, rows_a, rows_b, '%d x %d, %s' % (n, D, name))
        finally:
            src.close()


def test_split_row_index_past_2_16(gpu_required):
    n = 70000
    x = _source(n, 4)
    src = _lib.Features(x, device=0)
    r = np.random.RandomState(2)
    rows_a = np.concatenate((np.arange(65530, 65545), r.permutation(n)[:60000], [n - 1, 0, 65535, 65536]))
    rows_b = np.concatenate(([65536, 65535, n - 1], r.randint(65536, n, 9000), r.randint(0, 65536, 1000)))
    _check_split(src, x, rows_a, rows_b, 'both sides of row 65 536')
    # the outputs are handles like any other: split again, operated on, without touching what they came from
    a, b = src.split(rows_a, rows_b)
    aa, _ = a.split(np.arange(len(rows_a) - 1, -1, -1))
    a.gather([1, 0])
    np.testing.assert_array_equal(_bits(aa.download()), _bits(x[rows_a[::-1]]))
    np.testing.assert_array_equal(_bits(a.download()), _bits(x[rows_a[[1, 0]]]))
    np.testing.assert_array_equal(_bits(b.download()), _bits(x[rows_b]))
    for h in (src, a, b, aa):
        h.close()


def test_split_refusals(gpu_required):
    n = 9
    x = _source(n, 5)
    src = _lib.Features(x, device=0)
    good_a, good_b = np.array([8, 0, 3, 3]), np.array([2, 0])
    for bad in (-1, n):
        with pytest.raises(_lib.L3Error, match=r'libl3hip error -1: l3_feat_split: rows_a\[2\] = %d outside \[0, 9\)' % bad):
            src.split([1, 2, bad, 3], good_b)
        with pytest.raises(_lib.L3Error, match=r'libl3hip error -1: l3_feat_split: rows_b\[1\] = %d outside \[0, 9\)' % bad):
            src.split(good_a, [4, bad])
        with pytest.raises(_lib.L3Error, match=r'rows_a\[0\] = %d outside' % bad):
            src.split([bad])
    with pytest.raises(_lib.L3Error, match='need 1 <= n_a'):
        src.split([], good_b)
    # the out pointers stay as they were
    lib = _lib.load()
    out_a, out_b = C.c_void_p(12345), C.c_void_p(678)
    a, b = np.array([1, n], np.int64), np.array([-1], np.int64)
    ptr = lambda t: t.ctypes.data_as(C.c_void_p)
    assert lib.l3_feat_split(src.h, ptr(a), 2, ptr(good_b.astype(np.int64)), 2, C.byref(out_a), C.byref(out_b)) == -1
    assert b'rows_a[1] = 9 outside [0, 9)' in lib.l3_last_error(None)
    assert lib.l3_feat_split(src.h, ptr(a), 1, ptr(b), 1, C.byref(out_a), C.byref(out_b)) == -1
    assert b'rows_b[0] = -1 outside [0, 9)' in lib.l3_last_error(None)
    assert lib.l3_feat_split(src.h, ptr(a), 1, None, 1, C.byref(out_a), C.byref(out_b)) == -1          # n_b without its table
    assert lib.l3_feat_split(src.h, ptr(a), 1, ptr(b), 0, C.byref(out_a), None) == -1                   # a table without n_b
    assert lib.l3_feat_split(src.h, ptr(a), 1, None, 0, None, None) == -1
    assert lib.l3_feat_split(None, ptr(a), 1, None, 0, C.byref(out_a), None) == -1
    assert out_a.value == 12345 and out_b.value == 678
    # and a valid call still works, on the source as it was
    _check_split(src, x, good_a, good_b, 'after the refusals')
    with pytest.raises(_lib.L3Error, match='outside'):
        usc.DeviceFeatures.from_handle(src).split([n])
    src.close()


def test_device_features_split(gpu_required):
    x = _source(50, 24)
    whole = usc.DeviceFeatures(x, 0)
    kept, held = whole.split([4, 49, 0], [7])
    assert isinstance(kept, usc.DeviceFeatures) and isinstance(held, usc.DeviceFeatures) and kept.device == held.device == 0
    assert len(kept) == 3 and held.shape == (1, 24)
    np.testing.assert_array_equal(_bits(kept.to_host()), _bits(x[[4, 49, 0]]))
    np.testing.assert_array_equal(_bits(held.to_host()), _bits(x[[7]]))
    only, none = whole.split(np.arange(50)[::-1])
    assert none is None
    np.testing.assert_array_equal(_bits(only.to_host()), _bits(x[::-1]))
    whole.close()          # the parts own their rows
    np.testing.assert_array_equal(_bits(kept.to_host()), _bits(x[[4, 49, 0]]))
    for f in (kept, held, only):
        f.close()


# ---- the search on resident splits ----------------------------------------------------------------------------------------------------
SEARCH = dict(parameter_search=True, parameter_search_valid_fold=False, parameter_search_split_seed=6, use_min_max=True, random_state=4)
MLP_ARGS = dict(train_batch_size=8, num_epochs=3)


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return write_tree(tmp_path_factory.mktemp('param_split_gpu'))


@pytest.fixture
def downloads(monkeypatch):
    """the DeviceFeatures.to_host calls made from here on"""
    made = []
    to_host = usc.DeviceFeatures.to_host
    monkeypatch.setattr(usc.DeviceFeatures, 'to_host', lambda self: made.append(self) or to_host(self))
    return made


def _scaler_state(s):
    return {k: np.asarray(v) for k, v in vars(s).items()}


@pytest.mark.parametrize('train_with_valid', [False, True])
@pytest.mark.parametrize('model_type', ['mlp', 'svm'])
def test_cross_validate_equals_separate_folds(gpu_required, tree, tmp_path, downloads, model_type, train_with_valid):
    args = dict(SEARCH, parameter_search_train_with_valid=train_with_valid, **(MLP_ARGS if model_type == 'mlp' else {}))
    folds = [1, 2, 3, 4, 5]
    out = classifier.cross_validate(tree, str(tmp_path / 'cv'), model_type=model_type, fold_seed=5, preprocess_device=0, **args)
    assert not downloads          # the splits stayed on the GPU from the bank through the cut and every fit
    record = load_pickle(os.path.join(out, 'results.pkl'))
    assert record['folds'] == folds
    for i, (fold_num, fold_dir) in enumerate(zip(folds, record['fold_dirs'])):
        np.random.seed(5)
        if model_type == 'mlp':
            alone = classifier.train(tree, str(tmp_path / 'alone'), fold_num, model_type='mlp', preprocess_device=0, **args)
        else:
            alone = classifier.train_svm_fold(tree, str(tmp_path / 'alone'), fold_num, preprocess_device=0, **args)
        assert sorted(os.listdir(fold_dir)) == sorted(os.listdir(alone))
        config = load_config(fold_dir)
        assert config['parameter_search_split_seed'] == 6 and config['preprocess_device'] == 0
        got, want = load_pickle(os.path.join(fold_dir, 'results.pkl')), load_pickle(os.path.join(alone, 'results.pkl'))
        np.testing.assert_equal(got, want)          # dictionaries, lists and NaN (a class without examples) alike
        np.testing.assert_equal({part: record[part][i] for part in ('train', 'valid', 'test')}, got)
        assert len(got['valid']['search']) == (GRID_POINTS if model_type == 'mlp' else len(classifier.SVM_SEARCH_CS))
        assert got['train']['search_params_best_values'] == got['valid']['search_params_best_values']
        for name in ('stdizer.pkl', 'min_max_scaler.pkl'):
            a, b = _scaler_state(load_pickle(os.path.join(fold_dir, name))), _scaler_state(load_pickle(os.path.join(alone, name)))
            assert sorted(a) == sorted(b)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=name + ' ' + k)
        if model_type == 'svm':
            a, b = load_pickle(os.path.join(fold_dir, 'model.pkl')), load_pickle(os.path.join(alone, 'model.pkl'))
            assert a.C == b.C == got['valid']['search_params_best_values'][0]
            for name in ('dual_coef_', 'probA_', 'probB_', 'support_', 'intercept_'):
                np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    assert not downloads


def _watch_the_fold(monkeypatch):
    """-> (whole, made): `whole` receives the preprocessed training DeviceFeatures and its bits, `made` every DeviceFeatures that a
    split gives"""
    whole, made = [], []
    preprocess = classifier.preprocess_split_data

    def preprocessed(*splits, **kwargs):
        scalers = preprocess(*splits, **kwargs)
        whole.extend((splits[0]['features'], splits[0]['features'].handle.download(), splits[0]['labels'].copy()))
        return scalers
    monkeypatch.setattr(classifier, 'preprocess_split_data', preprocessed)
    split = usc.DeviceFeatures.split

    def watched(self, rows_a, rows_b=None):
        parts = split(self, rows_a, rows_b)
        made.extend(p for p in parts if p is not None)
        return parts
    monkeypatch.setattr(usc.DeviceFeatures, 'split', watched)
    return whole, made


def _closed(f):
    return f.handle.h is None


@pytest.mark.parametrize('train_with_valid', [False, True])
@pytest.mark.parametrize('model_type', ['mlp', 'svm'])
def test_the_fits_receive_the_cut_rows(gpu_required, tree, tmp_path, monkeypatch, downloads, model_type, train_with_valid):
    whole, made = _watch_the_fold(monkeypatch)
    received = []          # (training part, its bits, its labels, validation part or None, its bits, its labels) per fit

    def note(tr, va):
        assert not downloads          # nothing was downloaded up to this fit; the test's own downloads go past to_host
        received.append((tr['features'], tr['features'].handle.download(), np.asarray(tr['labels']),
                         va['features'] if va else None, va['features'].handle.download() if va else None,
                         np.asarray(va['labels']) if va else None))
    if model_type == 'mlp':
        train_mlp = classifier.train_mlp
        monkeypatch.setattr(classifier, 'train_mlp', lambda tr, va, te, md, **kw: note(tr, va) or train_mlp(tr, va, te, md, **kw))
        points = GRID_POINTS
    else:          # one fit of the whole grid on the training part, then one scoring per cost with the validation part
        score = classifier._svm_metrics_on_device
        monkeypatch.setattr(classifier, '_svm_metrics_on_device',
                            lambda clf, tr, va, te, nc: note(tr, va) or score(clf, tr, va, te, nc))
        points = len(classifier.SVM_SEARCH_CS)
    args = dict(SEARCH, parameter_search_train_with_valid=train_with_valid, preprocess_device=0, **(MLP_ARGS if model_type == 'mlp' else {}))
    np.random.seed(3)
    if model_type == 'mlp':
        classifier.train(tree, str(tmp_path), 2, model_type='mlp', **args)
    else:
        classifier.train_svm_fold(tree, str(tmp_path), 2, **args)
    original, X, y = whole
    train_idx, valid_idx = usc.stratified_shuffle_split(y, 0.15, 6)
    assert len(received) == points + (1 if train_with_valid else 0) and len(made) == 2
    for tr, tr_bits, tr_y, va, va_bits, va_y in received[:points]:
        assert tr is made[0] and va is made[1] and tr is not original
        np.testing.assert_array_equal(_bits(tr_bits), _bits(X[train_idx]))
        np.testing.assert_array_equal(_bits(va_bits), _bits(X[valid_idx]))
        np.testing.assert_array_equal(tr_y, y[train_idx])
        np.testing.assert_array_equal(va_y, y[valid_idx])
    if train_with_valid:          # the retrain: the original matrix itself, as it was, and no validation data
        tr, tr_bits, tr_y, va, _, _ = received[points]
        assert tr is original and va is None
        np.testing.assert_array_equal(_bits(tr_bits), _bits(X))
        np.testing.assert_array_equal(tr_y, y)
    assert not downloads
    assert all(_closed(f) for f in made) and _closed(original)


@pytest.mark.parametrize('model_type', ['mlp', 'svm'])
def test_the_parts_are_closed_after_a_failure(gpu_required, tree, tmp_path, monkeypatch, model_type):
    whole, made = _watch_the_fold(monkeypatch)
    calls = []

    def failing(*args, **kwargs):
        calls.append(len(calls))
        if len(calls) == 2:          # the second grid point
            raise RuntimeError('the second point fails')
        return None, {'accuracy': 0.5}, {'accuracy': 0.5}, {}
    if model_type == 'mlp':
        monkeypatch.setattr(classifier, 'train_mlp', failing)
    else:
        monkeypatch.setattr(classifier, '_svm_metrics_on_device', lambda *a: failing()[1:])
    with pytest.raises(RuntimeError, match='the second point fails'):
        classifier.cross_validate(tree, str(tmp_path), model_type=model_type, folds=[3], preprocess_device=0, **SEARCH)
    assert len(calls) == 2 and len(made) == 2
    assert all(_closed(f) for f in made) and _closed(whole[0])
