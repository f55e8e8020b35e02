"""Fold preprocessing on the GPU (csrc/featprep.hip; data/usc/features.py:52-150,243-253): every kernel against NumPy -- bit for
bit where the contract counts roundings, within the derived bounds of tests/featprep_ref.py where a summation order differs --
then the whole of usc.preprocess_split_data(device=0), the device-to-device hand-off to the MLP and the fold driver."""
import os
import pickle

import numpy as np
import pytest

import featprep_ref as ref
from l3embedding_amd import _lib, classifier, usc

pytestmark = pytest.mark.gpu

DS = [1, 5, 64, 130]          # a lone column, the scalar tail, exactly one dword x 4 slab of lanes, more than one slab + a tail
NS = [1, 2, 3, 1000, ref.CHUNK + 1, 3 * ref.CHUNK - 1]
BIG = np.float32(np.finfo(np.float32).max / 2)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _matrix(n, D, seed=0):
    """columns of different scale and offset; column 0 constant; with D > 1 the last column has min == max too"""
    r = np.random.RandomState(seed + 7 * n + D)
    x = (r.randn(n, D) * r.uniform(0.1, 4.0, size=D) + r.uniform(-3, 3, size=D)).astype(np.float32)
    x[:, 0] = np.float32(0.3)
    if D > 1:
        x[:, -1] = np.float32(-2.5)
    return x


@pytest.fixture(scope='module')
def cases():
    return {(n, D): _matrix(n, D) for n in NS for D in DS}


@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('n', NS)
def test_scaler_operators(gpu_required, cases, n, D):
    x = cases[(n, D)]
    f = _lib.Features(x)
    assert f.shape == (n, D)
    np.testing.assert_array_equal(_bits(f.download()), _bits(x))
    np.testing.assert_array_equal(_bits(f.download(n // 2, n)), _bits(x[n // 2:]))

    # min-max scaler: extrema, then the two-rounding transform, all NumPy's bits
    mm = usc.MinMaxScaler().fit(x)
    lo, hi = f.minmax()
    np.testing.assert_array_equal(_bits(lo), _bits(mm.data_min_))
    np.testing.assert_array_equal(_bits(hi), _bits(mm.data_max_))
    assert mm.scale_[0] == 1.0          # min == max: scaled by 1
    f.affine32(mm.scale_, mm.min_)
    scaled = mm.transform(x)
    np.testing.assert_array_equal(_bits(f.download()), _bits(scaled))

    # standardiser: moments within the derived bound, the transform (given the host's scaler) NumPy's bits
    std = usc.StandardScaler().fit(scaled)
    mean, var = f.moments()
    mean_bound, var_bound = ref.moments_bounds(scaled, std.var_)
    err_m, err_v = np.abs(mean - std.mean_), np.abs(var - std.var_)
    print('n %d D %d: mean err / bound %.3g, var err / bound %.3g' % (
        n, D, np.max(err_m / np.maximum(mean_bound, 1e-300)), np.max(err_v / np.maximum(var_bound, 1e-300))))
    assert np.all(err_m <= mean_bound) and np.all(err_v <= var_bound)
    assert var[0] == 0.0 and std.var_[0] == 0.0 and std.scale_[0] == 1.0          # the constant column, on both sides
    mean2, var2 = f.moments()
    assert mean.tobytes() == mean2.tobytes() and var.tobytes() == var2.tobytes()
    f.standardize(std.mean_, std.scale_)
    np.testing.assert_array_equal(_bits(f.download()), _bits(std.transform(scaled)))
    f.close()


@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('n', [1, 3, 1000])
def test_gather(gpu_required, cases, n, D):
    x = cases[(n, D)]
    f = _lib.Features(x)
    r = np.random.RandomState(n + D)
    rows = np.concatenate((r.permutation(n), r.randint(0, n, size=5), [n - 1, 0]))          # a permutation, repeats, both ends
    bad = rows.copy()
    bad[len(bad) // 2] = n
    with pytest.raises(_lib.L3Error, match=r'libl3hip error -1: l3_feat_gather: rows\[\d+\] = %d outside' % n):
        f.gather(bad)
    assert f.shape == (n, D)
    np.testing.assert_array_equal(_bits(f.download()), _bits(x))          # a refused gather leaves the matrix intact
    with pytest.raises(_lib.L3Error, match='outside'):
        f.gather([-1])
    f.gather(rows)
    assert f.shape == (len(rows), D)
    np.testing.assert_array_equal(_bits(f.download()), _bits(x[rows]))
    f.close()


FILE_ROWS = [1, 2, 3, 4, 10, 31, ref.LDS_ROWS, ref.LDS_ROWS + 1, 2 * ref.LDS_ROWS + 6]


@pytest.mark.parametrize('D', [5, 130])
def test_file_stats(gpu_required, D):
    """files of every interesting length in ONE matrix (not in row order, and not covering it): those that fit the LDS slab, the
    cap itself, and longer ones the kernel selects from global memory"""
    r = np.random.RandomState(D)
    n = sum(FILE_ROWS) + 4
    x = (r.randn(n, D) * r.uniform(0.1, 4.0, size=D) + r.uniform(-3, 3, size=D)).astype(np.float32)
    x[:, 1] = np.float32(1.25)                                   # constant: the zero rule, skew 0 and kurtosis -3
    x[:, 2] = np.round(x[:, 2])                                   # many ties around the median
    x[:, 3] = np.where(r.rand(n) < 0.5, BIG, -BIG)                # the even median's a + b must not overflow
    x[:, 4] = np.abs(x[:, 4]) * np.float32(1e-3) - np.float32(1e-3)
    ends = np.cumsum(FILE_ROWS) + 2
    file_idxs = np.stack((ends - np.array(FILE_ROWS), ends), axis=1)[::-1].copy()
    f = _lib.Features(x)
    with pytest.raises(_lib.L3Error, match='empty or outside'):
        f.file_stats([[0, 3], [5, 5]])
    f.file_stats(file_idxs)
    got = f.download()
    f.close()
    assert got.shape == (len(FILE_ROWS), 7 * D)
    for i, (s, e) in enumerate(file_idxs):
        xs = x[s:e]
        with np.errstate(over='ignore', invalid='ignore'):
            want = usc.compute_stats_features(xs)
        # (the float32 mean and variance of the +-FLT_MAX / 2 column overflow to the same infinities on both sides)
        np.testing.assert_array_equal(_bits(got[i, :5 * D]), _bits(want[:5 * D]), err_msg='file of %d rows' % (e - s))
        skew, kurt, skew_bound, kurt_bound, zero = ref.skew_kurt64(xs)
        gs, gk = got[i, 5 * D:6 * D].astype(np.float64), got[i, 6 * D:].astype(np.float64)
        half_ulp = lambda v: 0.5 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)          # noqa: E731
        es, ek = np.abs(gs - skew), np.abs(gk - kurt)
        print('F %d D %d: skew err / bound %.3g, kurtosis err / bound %.3g' % (
            e - s, D, np.max(es / (skew_bound + half_ulp(gs))), np.max(ek / (kurt_bound + half_ulp(gk)))))
        assert np.all(es <= skew_bound + half_ulp(gs)) and np.all(ek <= kurt_bound + half_ulp(gk))
        assert zero[1] and got[i, 5 * D + 1] == 0.0 and got[i, 6 * D + 1] == -3.0
        assert np.all(gs[zero] == 0.0) and np.all(gk[zero] == -3.0)


# ---- the whole of preprocess_split_data -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def splits():
    return ref.make_splits(21, D=130)


@pytest.mark.parametrize('use_min_max', [False, True])
@pytest.mark.parametrize('non_overlap', [False, True])
@pytest.mark.parametrize('feature_mode', ['framewise', 'stats'])
def test_pipeline(gpu_required, splits, feature_mode, non_overlap, use_min_max):
    kw = dict(feature_mode=feature_mode, non_overlap=non_overlap, use_min_max=use_min_max)
    host, dev, dev2 = ref.copy_splits(splits), ref.copy_splits(splits), ref.copy_splits(splits)
    np.random.seed(77)
    h_mm, h_std = usc.preprocess_split_data(*host, non_overlap_chunk_size=4, **kw)
    after_host = np.random.get_state()
    np.random.seed(77)
    d_mm, d_std = usc.preprocess_split_data(*dev, non_overlap_chunk_size=4, device=0, **kw)
    after_dev = np.random.get_state()
    assert np.array_equal(after_dev[1], after_host[1]) and after_dev[2] == after_host[2]          # one draw, at the same place
    for h, d in zip(host, dev):
        assert isinstance(d['features'], usc.DeviceFeatures) and d['features'].shape == h['features'].shape
        assert len(d['features']) == len(h['features'])
        np.testing.assert_array_equal(d['labels'], h['labels'])
        assert len(d['file_idxs']) == len(h['file_idxs'])
        for a, b in zip(d['file_idxs'], h['file_idxs']):
            np.testing.assert_array_equal(a, b)
    assert type(d_mm) is usc.MinMaxScaler and type(d_std) is usc.StandardScaler
    assert sorted(vars(d_mm)) == sorted(vars(h_mm)) and sorted(vars(d_std)) == sorted(vars(h_std))
    for k in ('data_min_', 'data_max_', 'data_range_', 'scale_', 'min_') if use_min_max else ():
        assert getattr(d_mm, k).dtype == getattr(h_mm, k).dtype
        np.testing.assert_array_equal(_bits(getattr(d_mm, k)), _bits(getattr(h_mm, k)))

    # the standardiser, within the bound of the matrix it was fitted on: the host pipeline up to that point (the bound does not
    # depend on the order of the rows)
    pre = ref.copy_splits(splits)
    np.random.seed(77)
    ref.host_pipeline(*pre, chunk_size=4, stdizer=_Identity(), **kw)
    mean_bound, var_bound = ref.moments_bounds(pre[0]['features'], h_std.var_)
    err_m, err_v = np.abs(d_std.mean_ - h_std.mean_), np.abs(d_std.var_ - h_std.var_)
    print('%s: mean err / bound %.3g, var err / bound %.3g' % (kw, np.max(err_m / np.maximum(mean_bound, 1e-300)),
                                                            np.max(err_v / np.maximum(var_bound, 1e-300))))
    assert np.all(err_m <= mean_bound) and np.all(err_v <= var_bound)
    assert d_std.n_samples_seen_ == h_std.n_samples_seen_
    np.testing.assert_array_equal(d_std.scale_, usc._handle_zeros(np.sqrt(d_std.var_)))

    # every split: the host pipeline re-run with the device's own standardiser, bit for bit, every element
    again = ref.copy_splits(splits)
    np.random.seed(77)
    ref.host_pipeline(*again, chunk_size=4, stdizer=d_std, **kw)
    for a, d in zip(again, dev):
        got = d['features'].to_host()
        np.testing.assert_array_equal(_bits(got), _bits(a['features']))
        np.testing.assert_array_equal(_bits(d['features'].rows(1, len(got))), _bits(got[1:]))

    # determinism: the device path again, the same bytes
    np.random.seed(77)
    e_mm, e_std = usc.preprocess_split_data(*dev2, non_overlap_chunk_size=4, device=0, **kw)
    assert e_std.mean_.tobytes() == d_std.mean_.tobytes() and e_std.var_.tobytes() == d_std.var_.tobytes()
    for a, b in zip(dev, dev2):
        assert a['features'].to_host().tobytes() == b['features'].to_host().tobytes()
    for d in dev + dev2:
        d['features'].close()


class _Identity(object):
    def transform(self, X):
        return X


# ---- hand-off to the MLP ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('validation', ['fold', 'split'])
def test_mlp_handoff_is_bit_identical(gpu_required, splits, validation):
    data = ref.copy_splits(splits)
    np.random.seed(3)
    usc.preprocess_split_data(*data, device=0)
    tr, va, te = data
    y, yv = classifier.one_hot(tr['labels'], 4), classifier.one_hot(va['labels'], 4)
    results = []
    for on_device in (True, False):
        x, xv, xt = (d['features'] if on_device else d['features'].to_host() for d in data)
        m, _, _ = classifier.construct_mlp_model((130,), num_classes=4, seed=5)
        m.compile(lr=1e-3)
        kw = dict(validation_data=(xv, yv)) if validation == 'fold' else dict(validation_split=0.15)
        hist = m.fit(x, y, batch_size=16, epochs=2, random_state=9, **kw)
        results.append((m.get_weights(), hist, m.predict(xt), m.predict(x)))
    (w_dev, h_dev, p_dev, q_dev), (w_host, h_host, p_host, q_host) = results
    for a, b in zip(w_dev, w_host):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert h_dev == h_host and set(h_dev) == {'loss', 'acc', 'val_loss', 'val_acc'} and len(h_dev['loss']) == 2
    np.testing.assert_array_equal(_bits(p_dev), _bits(p_host))
    np.testing.assert_array_equal(_bits(q_dev), _bits(q_host))
    for d in data:
        d['features'].close()


def test_features_destroyed_after_set_data_dev(gpu_required):
    """the MLP copies the rows into its own matrices: the l3_feat may go right after the hand-off"""
    r = np.random.RandomState(2)
    x = r.randn(70, 33).astype(np.float32)
    y = r.randint(0, 3, size=70).astype(np.int32)
    weights = []
    for on_device in (True, False):
        m = _lib.MLP(33, 3, 16, seed=1)
        if on_device:
            f = _lib.Features(x)
            m.set_data_dev(f, 0, 60, y[:60], f, 60, 70, y[60:])
            f.close()
            junk = _lib.Features(np.full((70, 33), 9.0, np.float32))          # likely to reuse the freed memory
        else:
            m.set_data(x[:60], y[:60], x[60:], y[60:])
        logs = [m.epoch(np.random.RandomState(e).permutation(60), 1e-3, 4 * e) for e in range(2)]
        weights.append((m.get_weights(), logs))
        m.close()
    junk.close()
    for a, b in zip(weights[0][0], weights[1][0]):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    assert weights[0][1] == weights[1][1]


def test_mlp_handoff_checks(gpu_required):
    f = _lib.Features(np.zeros((6, 5), np.float32))
    m = _lib.MLP(4, 3, 2)
    with pytest.raises(_lib.L3Error, match='not 4 columns wide'):
        m.set_data_dev(f, 0, 6, np.zeros(6, np.int32))
    m = _lib.MLP(5, 3, 2)
    with pytest.raises(_lib.L3Error, match=r'y_train\[2\] = 3 outside \[0, 3\)'):
        m.set_data_dev(f, 0, 6, np.array([0, 1, 3, 0, 0, 0], np.int32))
    with pytest.raises(_lib.L3Error, match='row range'):
        m.set_data_dev(f, 2, 7, np.zeros(5, np.int32))
    with pytest.raises(_lib.L3Error, match='outside the matrix'):
        m.predict_dev(f, 0, 7)
    m.set_data_dev(f, 1, 5, np.zeros(4, np.int32), f, 5, 6, np.zeros(1, np.int32))
    assert (m.n_train, m.n_valid) == (4, 1)
    assert m.predict_dev(f).shape == (6, 3)


# ---- the fold driver ----------------------------------------------------------------------------------------------------------------
def _write_feature_tree(root, D=24, files_per_fold=6):
    r = np.random.RandomState(0)
    centres = r.randn(50, D) * 2
    for fold in range(1, 6):
        d = os.path.join(root, 'fold%d' % fold)
        os.makedirs(d)
        for i in range(files_per_fold):
            label = (fold + i) % 3
            frames = (centres[label] + r.randn(r.randint(3, 9), D)).astype(np.float32)
            np.savez(os.path.join(d, 'clip%d.npz' % i), X=frames, y=np.array(label))


@pytest.mark.parametrize('feature_mode', ['framewise', 'stats'])
def test_fold_driver(gpu_required, tmp_path, feature_mode):
    feats = str(tmp_path / 'features' / 'esc50' / 'l3' / 'x')
    _write_feature_tree(feats)
    results = []
    for dev in (None, 0):
        np.random.seed(5)
        out = classifier.train(feats, str(tmp_path / ('out%s' % dev)), 2, model_type='mlp', feature_mode=feature_mode,
                               use_min_max=True, train_batch_size=8, random_state=4, num_epochs=3, learning_rate=1e-3,
                               preprocess_device=dev)
        results.append(pickle.load(open(os.path.join(out, 'results.pkl'), 'rb')))
        std = pickle.load(open(os.path.join(out, 'stdizer.pkl'), 'rb'))
        assert type(std) is usc.StandardScaler and std.mean_.dtype == np.float64
    host, dev = results
    # the training folds hold fewer than L3_FEAT_CHUNK_ROWS rows, so the device adds them in NumPy's order: the standardiser, the
    # features and with them every metric are the host run's, bit for bit
    for part in ('train', 'valid', 'test'):
        assert sorted(dev[part]) == sorted(host[part])
        for k, v in host[part].items():
            np.testing.assert_array_equal(np.asarray(dev[part][k], np.float64), np.asarray(v, np.float64), err_msg=part + ' ' + k)
    assert len(host['train']['loss_history']) == 3
