"""Folds resident on the GPU: l3_feat_assemble (csrc/featprep.hip) against np.concatenate, usc.FoldBank.split against usc.get_split,
usc.preprocess_split_data(device=0) on resident splits against uploaded ones, classifier.cross_validate against separate per-fold
calls, the searches' merge of two resident splits, and who closes a fold's splits after a failure.  Every comparison is for equal
bits: the assembly is a copy, and everything after it is the existing code on an identical matrix."""
import os
import pickle

import numpy as np
import pytest

from foldbank_ref import assert_same_split, write_tree
from l3embedding_amd import _lib, classifier, usc

pytestmark = pytest.mark.gpu

DS = [1, 5, 130, 257, 512]          # multiples of 4 and not, one row wider than a block's 256 lanes
SOURCE_ROWS = [1, 7, 64, 3, 129, 2, 33, 500, 10, 1000]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _source(n, D, seed):
    # distinct bit patterns, signed zeros and denormals included: a copy must not touch any of them
    r = np.random.RandomState(1000 * seed + D)
    x = r.randn(n, D).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7] = np.float32(-0.0)
    flat[3::11] = np.float32(1e-42)
    return x


@pytest.fixture(scope='module')
def sources(gpu_required):
    made = {D: [_source(n, D, i) for i, n in enumerate(SOURCE_ROWS)] for D in DS}
    handles = {D: [_lib.Features(x, device=0) for x in xs] for D, xs in made.items()}
    yield made, handles
    for hs in handles.values():
        for h in hs:
            h.close()


def _segment_lists(D):
    """name -> [(source index, lo, hi)]"""
    r = np.random.RandomState(D)
    interleaved = []
    for k in range(40):
        s = int(r.randint(len(SOURCE_ROWS)))
        lo = int(r.randint(0, SOURCE_ROWS[s]))
        interleaved.append((s, lo, int(r.randint(lo, SOURCE_ROWS[s] + 1))))
    return {
        'one row': [(0, 0, 1)],
        'one row of a long source': [(9, 998, 999)],
        '1000 one-row segments': [(9, int(i), int(i) + 1) for i in r.permutation(1000)],
        'a source twice': [(4, 0, 129), (4, 0, 129)],
        'a source twice, overlapping': [(7, 100, 400), (7, 50, 150)],
        'interleaved': interleaved,
        'every source whole, three times': [(s, 0, n) for s, n in enumerate(SOURCE_ROWS)] * 3,          # 5247 rows: several waves at any D
        'empty among others': [(1, 3, 3), (2, 0, 64), (0, 1, 1), (0, 0, 0), (3, 1, 2), (9, 1000, 1000), (5, 0, 2), (6, 33, 33)],
        # with an odd D a row starts on a 16-byte boundary when its index is a multiple of 4: source rows 1, 4, 3, 8, 5 go to the output
        # rows 0, 4, 9, 12, 25, so the second and the fourth segment move as 16-byte accesses (with a tail) and the others as 4-byte
        'odd rows': [(4, 1, 5), (4, 4, 9), (7, 3, 6), (7, 8, 21), (4, 5, 6)],
    }


@pytest.mark.parametrize('D', DS)
def test_assemble_equals_concatenate(sources, D):
    made, handles = sources
    for name, segs in _segment_lists(D).items():
        want = np.concatenate([made[D][s][lo:hi] for s, lo, hi in segs])
        out = _lib.Features.assemble([(handles[D][s], lo, hi) for s, lo, hi in segs], device=0)
        try:
            assert out.shape == want.shape and out.device == 0, name
            np.testing.assert_array_equal(_bits(out.download()), _bits(want), err_msg=name)
        finally:
            out.close()
    for x, h in zip(made[D], handles[D]):          # the sources are as they were
        np.testing.assert_array_equal(_bits(h.download()), _bits(x))


def test_assemble_row_index_past_2_16(gpu_required):
    r = np.random.RandomState(5)
    xs = [r.randn(n, 5).astype(np.float32) for n in (40000, 30001)]
    hs = [_lib.Features(x, device=0) for x in xs]
    segs = [(0, 0, 40000), (1, 1, 30001)]          # 70 000 rows; the second source starts at an odd row
    out = _lib.Features.assemble([(hs[s], lo, hi) for s, lo, hi in segs])
    assert out.shape == (70000, 5)
    np.testing.assert_array_equal(_bits(out.download()), _bits(np.concatenate([xs[s][lo:hi] for s, lo, hi in segs])))
    # the result is a handle like any other: it can be a source, and be operated on, without touching what it came from
    again = _lib.Features.assemble([(out, 69990, 70000), (hs[0], 0, 1)])
    out.gather(np.arange(69999, -1, -1))
    np.testing.assert_array_equal(_bits(again.download()), _bits(np.concatenate((xs[1][29991:], xs[0][:1]))))
    np.testing.assert_array_equal(_bits(out.download(0, 2)), _bits(xs[1][:-3:-1]))
    np.testing.assert_array_equal(_bits(hs[1].download()), _bits(xs[1]))
    for h in hs + [out, again]:
        h.close()


def test_assemble_refusals(sources):
    made, handles = sources
    a, b, wide = handles[5][1], handles[5][0], handles[130][1]          # 7 x 5, 1 x 5, 7 x 130
    many = _lib.Features(np.zeros((70000, 1), np.float32))
    cases = [
        ([], 'need at least one segment'),
        ([(a, 0, 7), (wide, 0, 1)], 'segment 1: the source has 130 columns, segment 0 has 5'),
        ([(a, -1, 3)], r'segment 0: rows \[-1, 3\) outside'),
        ([(a, 0, 7), (b, 0, 1), (a, 2, 8)], r'segment 2: rows \[2, 8\) outside the source\'s \[0, 7\)'),
        ([(b, 0, 1), (a, 5, 4)], r'segment 1: rows \[5, 4\) outside'),
        ([(a, 3, 3), (b, 1, 1)], 'hold 0 rows in total'),
        ([(many, 0, 70000)] * 30679, r'segment 30678: the total passes 2\^31 - 1 rows'),
    ]
    for segs, message in cases:
        with pytest.raises(_lib.L3Error, match=message):
            _lib.Features.assemble(segs, device=0)
    # a source on another device: the request for device 1 is refused for its sources before device 1 is looked for
    with pytest.raises(_lib.L3Error, match='segment 0: the source is on device 0, not on device 1'):
        _lib.Features.assemble([(a, 0, 7)], device=1)
    with pytest.raises(ValueError, match='segment 1'):
        _lib.Features.assemble([(a, 0, 7), (made[5][0], 0, 1)])
    # *out stays as it was
    import ctypes as C
    lib = _lib.load()
    out = C.c_void_p(12345)
    table = np.zeros(1, _lib.Features.SEGMENT)
    table[0] = (a.h.value, 0, 8)
    assert lib.l3_feat_assemble(0, table.ctypes.data_as(C.c_void_p), 1, C.byref(out)) != 0 and out.value == 12345
    table[0] = (0, 0, 1)
    assert lib.l3_feat_assemble(0, table.ctypes.data_as(C.c_void_p), 1, C.byref(out)) != 0 and out.value == 12345
    assert b'segment 0: the source is NULL' in lib.l3_last_error(None)
    # and a valid call still works
    ok = _lib.Features.assemble([(a, 1, 3), (b, 0, 1), (a, 7, 7)])
    np.testing.assert_array_equal(_bits(ok.download()), _bits(np.concatenate((made[5][1][1:3], made[5][0]))))
    ok.close(), many.close()


# ---- FoldBank ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp('foldbank_gpu')
    return {'esc50': write_tree(root / 'a', 'esc50'), 'us8k': write_tree(root / 'b', 'us8k', seed=1)}


@pytest.mark.parametrize('dataset', ['esc50', 'us8k'])
def test_bank_split_equals_get_split(gpu_required, trees, dataset):
    with usc.FoldBank(trees[dataset], dataset, device=0) as bank:
        for test_fold, valid in ((0, True), (1, False), (2, True), (bank.num_folds - 1, True)):
            got = bank.split(test_fold, valid=valid)
            for g, w in zip(got, usc.get_split(trees[dataset], test_fold, dataset, valid=valid)):
                assert g is None or (isinstance(g['features'], usc.DeviceFeatures) and g['features'].device == 0)
                assert_same_split(g, w)
            for g in got:
                if g:
                    g['features'].close()
        # a split that was preprocessed in place leaves the bank as it was
        got = bank.split(0)
        usc.preprocess_split_data(*got, use_min_max=True, device=0)
        for g, w in zip(bank.split(0), usc.get_split(trees[dataset], 0, dataset)):
            assert_same_split(g, w)
    with pytest.raises(ValueError, match='closed'):
        bank.split(0)


def test_bank_survives_a_failed_split(gpu_required, trees, monkeypatch):
    with usc.FoldBank(trees['esc50'], 'esc50', device=0) as bank:
        calls = []
        assemble = usc.DeviceFeatures.assemble.__func__

        def failing(cls, segments, device=0):
            calls.append(len(calls))
            if len(calls) == 2:          # the second of the three matrices: as a failed allocation surfaces
                raise _lib.L3Error('libl3hip error 2: l3_feat_assemble: device allocation failed')
            return assemble(cls, segments, device)
        monkeypatch.setattr(usc.DeviceFeatures, 'assemble', classmethod(failing))
        with pytest.raises(_lib.L3Error):
            bank.split(0)
        monkeypatch.undo()
        for g, w in zip(bank.split(0), usc.get_split(trees['esc50'], 0, 'esc50')):
            assert_same_split(g, w)


# ---- preprocess_split_data on resident splits -----------------------------------------------------------------------------------------
def _scaler_state(s):
    return {k: np.asarray(v) for k, v in vars(s).items()}


@pytest.mark.parametrize('use_min_max', [False, True])
@pytest.mark.parametrize('non_overlap', [False, True])
@pytest.mark.parametrize('feature_mode', ['framewise', 'stats'])
def test_preprocess_resident_splits(gpu_required, trees, feature_mode, non_overlap, use_min_max):
    args = dict(feature_mode=feature_mode, non_overlap=non_overlap, non_overlap_chunk_size=4, use_min_max=use_min_max, device=0)
    with usc.FoldBank(trees['us8k'], 'us8k', device=0) as bank:
        got = bank.split(2)
        handles = [d['features'].handle for d in got]
        np.random.seed(21)
        got_scalers = usc.preprocess_split_data(*got, **args)
        got_state = np.random.get_state()
    assert [d['features'].handle for d in got] == handles          # preprocessed where they were: no upload, no new handle
    want = usc.get_split(trees['us8k'], 2, 'us8k')
    np.random.seed(21)
    want_scalers = usc.preprocess_split_data(*want, **args)
    np.testing.assert_array_equal(got_state[1], np.random.get_state()[1])
    assert got_state[2:] == np.random.get_state()[2:]
    for g, w in zip(got_scalers, want_scalers):
        a, b = _scaler_state(g), _scaler_state(w)
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_bits(g['features'].to_host()), _bits(w['features'].to_host()))
        np.testing.assert_array_equal(g['labels'], w['labels'])
        assert len(g['file_idxs']) == len(w['file_idxs'])
        for a, b in zip(g['file_idxs'], w['file_idxs']):
            np.testing.assert_array_equal(a, b)


def test_preprocess_device_mismatch(gpu_required, trees):
    with usc.FoldBank(trees['esc50'], 'esc50', device=0) as bank:
        splits = bank.split(0)
        with pytest.raises(ValueError, match='on device 0, the preprocessing runs on device 1'):
            usc.preprocess_split_data(*splits, device=1)
        with pytest.raises(ValueError, match='device is None'):
            usc.preprocess_split_data(*splits, device=None)
        for g, w in zip(splits, usc.get_split(trees['esc50'], 0, 'esc50')):          # untouched by the refusals
            assert_same_split(g, w)


# ---- cross_validate -------------------------------------------------------------------------------------------------------------------
def _write_feature_tree(root, D=24, files_per_fold=6):
    """the 5-fold tree of test_featprep_gpu's fold driver test"""
    r = np.random.RandomState(0)
    centres = r.randn(50, D) * 2
    for fold in range(1, 6):
        d = os.path.join(root, 'fold%d' % fold)
        os.makedirs(d)
        for i in range(files_per_fold):
            label = (fold + i) % 3
            frames = (centres[label] + r.randn(r.randint(3, 9), D)).astype(np.float32)
            np.savez(os.path.join(d, 'clip%d.npz' % i), X=frames, y=np.array(label))


def _load(path):
    with open(path, 'rb') as fh:
        return pickle.load(fh)


@pytest.mark.parametrize('model_type,search', [('mlp', False), ('svm', False), ('svm', True)])
def test_cross_validate_equals_separate_folds(gpu_required, tmp_path, model_type, search):
    feats = str(tmp_path / 'features' / 'esc50' / 'l3' / 'x')
    _write_feature_tree(feats)
    args = dict(use_min_max=True, random_state=4, parameter_search=search, parameter_search_train_with_valid=search)
    if model_type == 'mlp':
        args.update(train_batch_size=8, num_epochs=3, learning_rate=1e-3)
    out = classifier.cross_validate(feats, str(tmp_path / 'cv'), model_type=model_type, fold_seed=5, preprocess_device=0, **args)
    record = _load(os.path.join(out, 'results.pkl'))
    assert record['folds'] == [1, 2, 3, 4, 5]
    for fold_num, fold_dir in zip(record['folds'], record['fold_dirs']):
        np.random.seed(5)
        if model_type == 'mlp':
            alone = classifier.train(feats, str(tmp_path / 'alone'), fold_num, model_type='mlp', preprocess_device=0, **args)
        else:
            alone = classifier.train_svm_fold(feats, str(tmp_path / 'alone'), fold_num, preprocess_device=0, **args)
        assert sorted(os.listdir(fold_dir)) == sorted(os.listdir(alone))
        got, want = _load(os.path.join(fold_dir, 'results.pkl')), _load(os.path.join(alone, 'results.pkl'))
        np.testing.assert_equal(got, want)          # dictionaries, lists and NaN (a class without examples) alike
        np.testing.assert_equal(record_fold(record, fold_num), got)
        for name in ('stdizer.pkl', 'min_max_scaler.pkl'):
            a, b = _scaler_state(_load(os.path.join(fold_dir, name))), _scaler_state(_load(os.path.join(alone, name)))
            assert sorted(a) == sorted(b)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=name + ' ' + k)
        if model_type == 'svm':
            a, b = _load(os.path.join(fold_dir, 'model.pkl')), _load(os.path.join(alone, 'model.pkl'))
            assert a.C == b.C
            for name in ('dual_coef_', 'probA_', 'probB_', 'support_', 'intercept_'):
                np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)
    if model_type == 'mlp':
        assert len(record['train'][0]['loss_history']) == 3 and 'loss_history' not in record['aggregate']['train']
    if search:
        assert 'search' in record['valid'][0] and 'search' not in record['aggregate']['valid']
    with np.errstate(all='ignore'):
        want = classifier.aggregate_metrics([{'accuracy': m['accuracy']} for m in record['test']])
    assert record['aggregate']['test']['accuracy'] == want['accuracy']


def record_fold(record, fold_num):
    i = record['folds'].index(fold_num)
    return {part: record[part][i] for part in ('train', 'valid', 'test')}


# ---- train_svm_search's merge of two resident splits ---------------------------------------------------------------------------------
def test_search_merges_resident_splits_on_the_device(gpu_required, tmp_path, monkeypatch):
    r = np.random.RandomState(0)
    nc, D = 4, 12
    centres = r.randn(nc, D) * 0.9

    def split(n):
        y = np.arange(n) % nc
        return {'features': (centres[y] + r.randn(n, D)).astype(np.float32), 'labels': y}
    train, valid = split(160), split(60)
    yf = np.arange(8) % nc
    test = {'features': (centres[np.repeat(yf, 6)] + r.randn(48, D)).astype(np.float32), 'labels': yf,
            'file_idxs': [(6 * f, 6 * f + 6) for f in range(8)]}
    d1, d2 = str(tmp_path / 'a'), str(tmp_path / 'b')
    os.makedirs(d1), os.makedirs(d2)
    args = dict(Cs=(0.1, 1, 10), train_with_valid=True, num_classes=nc, random_state=3)
    np.random.seed(11)
    want = classifier.train_svm_search(train, valid, test, d1, **args)
    resident = [dict(d, features=usc.DeviceFeatures(d['features'], 0)) for d in (train, valid, test)]
    downloads = []
    to_host = usc.DeviceFeatures.to_host
    monkeypatch.setattr(usc.DeviceFeatures, 'to_host', lambda self: downloads.append(self) or to_host(self))
    np.random.seed(11)
    got = classifier.train_svm_search(*resident, d2, **args)
    assert not downloads          # merged and shuffled where the splits are
    assert got[0].C == want[0].C
    for k in range(1, 4):
        np.testing.assert_equal(got[k], want[k])
    for name in ('classes_', 'support_', 'support_vectors_', 'n_support_', 'dual_coef_', 'intercept_', 'probA_', 'probB_'):
        np.testing.assert_array_equal(getattr(got[0], name), getattr(want[0], name), err_msg=name)
    for d, x in zip(resident, (train, valid, test)):          # the splits themselves are as they were
        np.testing.assert_array_equal(_bits(to_host(d['features'])), _bits(x['features']))


def _closed(f):
    return f.handle.h is None


@pytest.mark.parametrize('D', [20, 7])          # rows of 80 bytes move as 16-byte accesses, rows of 28 bytes as 4-byte ones
def test_param_search_merges_resident_splits_on_the_device(gpu_required, tmp_path, monkeypatch, D):
    """train_param_search with a validation fold and train_with_valid on two resident splits: the retrain's train + valid is put
    together and shuffled on the GPU, as train_svm_search's is, and everything equals the same search on the same rows as arrays"""
    r = np.random.RandomState(D)
    nc = 4
    centres = r.randn(nc, D) * 0.9

    def split(n):
        y = np.arange(n) % nc
        return {'features': (centres[y] + r.randn(n, D)).astype(np.float32), 'labels': y}
    train, valid = split(96), split(32)
    yf = np.arange(8) % nc
    test = {'features': (centres[np.repeat(yf, 6)] + r.randn(48, D)).astype(np.float32), 'labels': yf,
            'file_idxs': [(6 * f, 6 * f + 6) for f in range(8)]}
    d1, d2 = str(tmp_path / 'a'), str(tmp_path / 'b')
    os.makedirs(d1), os.makedirs(d2)
    args = dict(train_func=classifier.train_svm, search_space={'C': [0.5, 2.0]}, train_with_valid=True, evaluate_on_device=True,
                num_classes=nc, random_state=3)
    np.random.seed(7)
    want = classifier.train_param_search(train, valid, test, d1, **args)

    resident = [usc.DeviceFeatures(d['features'], 0) for d in (train, valid)]
    made = []
    assemble = usc.DeviceFeatures.assemble.__func__

    def watched(cls, segments, device=0):
        made.append(assemble(cls, segments, device))
        return made[-1]
    monkeypatch.setattr(usc.DeviceFeatures, 'assemble', classmethod(watched))
    np.random.seed(7)
    got = classifier.train_param_search(dict(train, features=resident[0]), dict(valid, features=resident[1]), test, d2, **args)
    for name in ('dual_coef_', 'support_', 'intercept_', 'probA_', 'probB_'):
        np.testing.assert_array_equal(getattr(got[0], name), getattr(want[0], name), err_msg=name)
    for k in range(1, 4):
        np.testing.assert_equal(got[k], want[k])
    assert got[1]['search_params_best_values'] == want[1]['search_params_best_values'] and len(got[2]['search']) == 2
    # the merged matrix was made on the GPU and is closed; the caller's two are open and as they were
    assert len(made) == 1 and all(_closed(f) for f in made)
    for f, d in zip(resident, (train, valid)):
        assert not _closed(f)
        np.testing.assert_array_equal(_bits(f.to_host()), _bits(d['features']))
        f.close()


def test_cross_validate_closes_the_fold_after_an_early_failure(gpu_required, tmp_path, monkeypatch):
    """a failure between the assembly of a fold's splits and its fit (here: the preprocessing) closes the splits, and the bank"""
    feats = str(tmp_path / 'features' / 'esc50' / 'l3' / 'x')
    _write_feature_tree(feats)
    banks, made = [], []
    split = usc.FoldBank.split

    def watched(self, test_fold_idx, valid=True):
        splits = split(self, test_fold_idx, valid=valid)
        banks.append(self)
        made.extend(d['features'] for d in splits if d)
        return splits
    monkeypatch.setattr(usc.FoldBank, 'split', watched)

    def failing(*splits, **kwargs):
        assert len(made) == 3 and not any(_closed(f) for f in made)          # the splits exist
        raise RuntimeError('the preprocessing fails')
    monkeypatch.setattr(classifier, 'preprocess_split_data', failing)
    with pytest.raises(RuntimeError, match='the preprocessing fails'):
        classifier.cross_validate(feats, str(tmp_path / 'out'), preprocess_device=0, folds=[2])
    assert len(made) == 3 and all(isinstance(f, usc.DeviceFeatures) and _closed(f) for f in made)
    assert len(banks) == 1 and banks[0].folds is None
