"""CPU tests of the principal components (pca.py, csrc/pca.hip's contract): the NumPy oracle against an SVD of the centred
rows, the sign rule with ties, n_components as an integer, a fraction and None, the whitening refusal on a rank-deficient input, the
binding table, the refusals that come before the device, from_arrays and pickling, and the command line with the device part replaced
by NumPy."""
import os
import pickle
import re

import numpy as np
import pytest

import pca_ref as R
from l3embedding_amd import _lib, cli_pca, pca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ['l3_pca_create', 'l3_pca_destroy', 'l3_pca_splits', 'l3_pca_set_rows', 'l3_pca_set_rows_dev', 'l3_pca_mean', 'l3_pca_set_mean',
           'l3_pca_scatter', 'l3_pca_set_model', 'l3_pca_transform', 'l3_pca_transform_dev', 'l3_pca_inverse', 'l3_pca_inverse_dev',
           'l3_pca_time']


def host_fit(model, X):
    """what PCA.fit does, with the device's two results (mean, scatter) taken from the oracle"""
    m64 = R.mean_ref(X)
    m32 = m64.astype(np.float32)
    model._finish(X.shape[0], m32, R.scatter_ref(X, m32))
    return model


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(300, 40), (129, 200), (500, 7)], ids=lambda s: '%d-%d' % s)
def test_fit_ref_agrees_with_an_svd_of_the_centred_rows(shape):
    n, D = shape
    X = R.embedding_like(np.random.RandomState(n + D), n, D).astype(np.float64)
    ref = R.fit_ref(X)
    xc = X - X.mean(axis=0)
    _, sv, vt = np.linalg.svd(xc, full_matrices=False)
    var = sv ** 2 / (n - 1)
    r = min(n - 1, D)
    assert np.allclose(ref['variance'][:r], var[:r], rtol=1e-10, atol=1e-12 * var[0])
    assert np.all(ref['variance'][r:] <= 1e-10 * var[0])          # a rank of at most n - 1
    assert np.all(np.diff(ref['variance']) <= 0)
    # the spans: distinct singular values, so each axis is the SVD's up to its sign
    dots = np.abs(np.sum(ref['components'][:r] * vt[:r], axis=1))
    assert np.all(dots > 1 - 1e-8)
    assert abs(ref['ratio'].sum() - 1.0) < 1e-12
    # the blocked float64 scatter about the float32 mean is np.cov up to the mean's rounding
    m32 = X.mean(axis=0).astype(np.float32)
    S = R.scatter_ref(X.astype(np.float32), m32)
    assert np.allclose(S / (n - 1), ref['covariance'], rtol=0, atol=1e-6 * var[0])


def test_sign_rule_with_ties():
    w = np.array([[1.0, -3.0, 2.0], [-2.0, 2.0, 1.0], [2.0, -2.0, 1.0], [0.0, 0.0, 0.0], [-0.5, 0.25, 0.5]])
    for rule in (pca.sign_rule, R.sign_rule):
        got = rule(w)
        assert np.array_equal(got[0], [-1.0, 3.0, -2.0])           # the largest magnitude becomes positive
        assert np.array_equal(got[1], [2.0, -2.0, -1.0])           # |-2| == |2|: the lower index decides
        assert np.array_equal(got[2], [2.0, -2.0, 1.0])            # already positive at the lower index
        assert np.array_equal(got[3], [0.0, 0.0, 0.0])
        assert np.array_equal(got[4], [0.5, -0.25, -0.5])
        assert np.array_equal(w[0], [1.0, -3.0, 2.0])              # the input is left as it is


def test_eigen_equals_the_oracle_and_clips_round_off():
    rng = np.random.RandomState(5)
    A = rng.randn(30, 6)
    C = A.T @ A
    lam, axes = pca.eigen(C)
    ref_lam, ref_axes = R.eigen_ref(C)
    assert np.array_equal(lam, ref_lam) and np.array_equal(axes, ref_axes)
    B = rng.randn(3, 8)
    lam, _ = pca.eigen(B.T @ B)                                    # rank 3 of 8: the rest is round-off of either sign
    assert np.all(lam >= 0.0) and np.all(lam[3:] < 1e-12)


def test_n_components_as_integer_fraction_and_none():
    X = R.embedding_like(np.random.RandomState(1), 200, 12)
    ref = R.fit_ref(X)
    full = host_fit(pca.PCA(), X)
    assert full.n_components_ == 12 and full.components_.shape == (12, 12) and full.components_.dtype == np.float32
    assert full.mean_.dtype == np.float32 and full.explained_variance_.dtype == np.float64 and full.n_samples_ == 200
    assert np.allclose(full.explained_variance_, ref['variance'], rtol=1e-5)
    assert abs(full.explained_variance_ratio_.sum() - 1.0) < 1e-12
    three = host_fit(pca.PCA(3), X)
    assert three.components_.shape == (3, 12) and np.array_equal(three.components_, full.components_[:3])
    for share in (0.5, 0.9, 0.999, float(ref['ratio'][0])):
        got = host_fit(pca.PCA(share), X)
        assert got.n_components_ == R.count_for_ref(ref['ratio'], share)
        assert got.explained_variance_ratio_.sum() >= share > got.explained_variance_ratio_[:-1].sum()
    assert not hasattr(full, 'covariance_')
    kept = host_fit(pca.PCA(2, keep_covariance=True), X)
    assert np.allclose(kept.covariance_, ref['covariance'], atol=1e-5)
    for bad in (0, -1, 1.0, 1.5, 0.0, True, 'all'):
        with pytest.raises(ValueError, match='n_components'):
            pca.PCA(bad)
    with pytest.raises(ValueError, match='only 12 features'):
        host_fit(pca.PCA(13), X)


def test_whiten_refuses_a_component_of_zero_variance():
    rng = np.random.RandomState(2)
    X = (rng.randn(60, 5) @ rng.randn(5, 9)).astype(np.float32)          # rank 5 of 9
    X[:, 8] = 3.0                                                         # and a constant column: an exactly zero direction
    with pytest.raises(ValueError, match=r'whiten=True: component \d+ has the explained variance'):
        host_fit(pca.PCA(whiten=True), X)
    model = pca.PCA(whiten=True)
    try:
        host_fit(model, X)
    except ValueError:
        pass
    assert model.components_ is None                                      # a refused fit leaves no model
    ok = host_fit(pca.PCA(5, whiten=True), X)
    assert ok.scale_.dtype == np.float32 and np.array_equal(ok.scale_, (1.0 / np.sqrt(ok.explained_variance_)).astype(np.float32))
    assert host_fit(pca.PCA(5), X).scale_ is None


# ---- the binding, refusals, pickling ----------------------------------------------------------------------------------------------------------
def test_every_symbol_is_in_the_binding_and_the_header():
    header = open(os.path.join(ROOT, 'include', 'l3hip.h')).read()
    declared = set(re.findall(r'\b(l3_(?:op_)?pca[a-z_0-9]*)\s*\(', re.sub(r'/\*.*?\*/', '', header, flags=re.S)))
    assert declared == set(SYMBOLS)
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
    assert '#define L3_PCA_CHAIN 256' in header and _lib.PCA_CHAIN == R.R == 256
    assert '#define L3_PCA_MEAN_SEG 256' in header and _lib.PCA_MEAN_SEG == 256
    assert '#define L3_PCA_FILL 512' in header and _lib.PCA_FILL == 512
    assert '#define L3_PCA_MAX_SPLITS 256' in header and _lib.PCA_MAX_SPLITS == 256
    assert '#define L3_PCA_MAX_D 16384' in header and _lib.PCA_MAX_D == 16384


def test_the_split_rule_of_the_oracle():
    assert R.splits_ref(240000, 512) == 51 and R.splits_ref(60000, 6144) == 1 and R.splits_ref(2051, 40) == 9
    assert R.splits_ref(100000, 19) == 256 and R.splits_ref(40, 6144) == 1
    assert R.split_ranges(2051, 3) == [(0, 768), (768, 1536), (1536, 2051)]
    assert R.split_ranges(1300, 7) == [(256 * c, min(1300, 256 * (c + 1))) for c in range(6)]          # clamped to the 6 chains
    for n, s in ((2051, 7), (1300, 2), (40, 3)):
        ranges = R.split_ranges(n, s)
        assert ranges[0][0] == 0 and ranges[-1][1] == n
        assert all(a[1] == b[0] and a[0] < a[1] and a[1] % 256 == 0 for a, b in zip(ranges, ranges[1:]))


def test_refusals_come_before_the_device():
    """every one of these is a ValueError on a machine without a GPU: nothing reaches the library"""
    X = np.zeros((10, 4), np.float32)
    with pytest.raises(ValueError, match='float32'):
        pca.PCA(2).fit(X.astype(np.float64))
    with pytest.raises(ValueError, match='at least 2 rows'):
        pca.PCA(2).fit(X[:1])
    with pytest.raises(ValueError, match='only 4 features'):
        pca.PCA(5).fit(X)
    with pytest.raises(ValueError, match='fit comes first'):
        pca.PCA(2).transform(X)
    for D in (0, 16385, 2.0, True):
        with pytest.raises(ValueError, match='D must be'):
            _lib.PCA(D)
    h = _lib.PCA(4)
    with pytest.raises(ValueError, match='set_rows comes first'):
        h.mean()
    with pytest.raises(ValueError, match='set_rows comes first'):
        h.scatter()
    with pytest.raises(ValueError, match='at least 2 rows'):
        h.set_rows(X[:1])
    with pytest.raises(ValueError, match='columns'):
        h.set_rows(np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match='set_model comes first'):
        h.transform(X)
    with pytest.raises(ValueError, match='components must be float32'):
        h.set_model(np.zeros(4, np.float32), np.zeros((5, 4), np.float32))
    with pytest.raises(ValueError, match='scale'):
        h.set_model(np.zeros(4, np.float32), np.zeros((2, 4), np.float32), np.array([1.0, 0.0], np.float32))
    with pytest.raises(ValueError, match='mean must be'):
        h.set_mean(np.array([0, 0, np.nan, 0], np.float32))
    h.n, h.has_mean = 10, True          # (stand for resident rows: the argument checks that follow them)
    with pytest.raises(ValueError, match='splits'):
        h.scatter(splits=257)
    h.n = 0
    model = pca.PCA.from_arrays(np.zeros(4, np.float32), np.eye(4, dtype=np.float32)[:2])
    with pytest.raises(ValueError, match='expecting 4'):
        model.transform(np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError, match='expecting 2'):
        model.inverse_transform(np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match='float32'):
        pca.PCA.from_arrays(np.zeros(4), np.eye(4, dtype=np.float32))
    with pytest.raises(ValueError, match='needs the explained variances'):
        pca.PCA.from_arrays(np.zeros(4, np.float32), np.eye(4, dtype=np.float32), whiten=True)
    with pytest.raises(ValueError, match='component 1 has'):
        pca.PCA.from_arrays(np.zeros(4, np.float32), np.eye(4, dtype=np.float32)[:2], explained_variance=[1.0, 0.0], whiten=True)
    assert h.h is None and model._h is None          # no handle was ever created


def test_from_arrays_and_pickle_round_trips():
    rng = np.random.RandomState(3)
    mean, w = rng.randn(6).astype(np.float32), np.linalg.qr(rng.randn(6, 6))[0][:3].astype(np.float32)
    model = pca.PCA.from_arrays(mean, w, explained_variance=[4.0, 1.0, 0.25], whiten=True)
    assert model.n_components_ == 3 and np.array_equal(model.scale_, np.array([0.5, 1.0, 2.0], np.float32))
    model._h = object()          # stands for a device handle
    back = pickle.loads(pickle.dumps(model))
    model._h = None
    assert back._h is None and back.whiten is True and back.n_components_ == 3
    for name in ('mean_', 'components_', 'explained_variance_', 'scale_'):
        assert np.array_equal(getattr(back, name), getattr(model, name))
    fitted = host_fit(pca.PCA(0.9), R.embedding_like(rng, 100, 8))
    back = pickle.loads(pickle.dumps(fitted))
    assert back.n_components_ == fitted.n_components_ and np.array_equal(back.components_, fitted.components_)
    assert np.array_equal(back.explained_variance_ratio_, fitted.explained_variance_ratio_) and back.n_samples_ == 100


# ---- the command line -----------------------------------------------------------------------------------------------------------------------
def test_cli_parser():
    command, args = cli_pca.parse_arguments(['fit', '--features', 'a.npz', 'dir', '--n-components', '50', '--whiten', '--out', 'm.npz'])
    assert command == 'fit' and args == dict(features=['a.npz', 'dir'], n_components=50, whiten=True, device=0, out='m.npz')
    command, args = cli_pca.parse_arguments(['fit', '--features', 'a.npz', '--n-components', '0.95', '--out', 'm.npz'])
    assert args['n_components'] == 0.95 and args['whiten'] is False
    assert cli_pca.parse_arguments(['fit', '--features', 'a.npz', '--n-components', 'all', '--out', 'm.npz'])[1]['n_components'] is None
    command, args = cli_pca.parse_arguments(['transform', '--model', 'm.npz', '--features', 'F', '--out', 'G', '--device', '1'])
    assert command == 'transform' and args == dict(model='m.npz', features='F', out='G', device=1)
    for bad in (['fit', '--features', 'a.npz', '--out', 'm.npz'],                                      # no --n-components
                ['fit', '--features', 'a.npz', '--n-components', '0', '--out', 'm.npz'],
                ['fit', '--features', 'a.npz', '--n-components', '1.5', '--out', 'm.npz'],
                ['fit', '--features', 'a.npz', '--n-components', 'many', '--out', 'm.npz'],
                ['transform', '--features', 'F', '--out', 'G']):
        with pytest.raises(SystemExit):
            cli_pca.parse_arguments(bad)


def test_cli_transform_carries_the_other_arrays_over(tmp_path, monkeypatch):
    """the device part (PCA.transform) replaced by the float64 oracle: what is tested is the files"""
    rng = np.random.RandomState(4)
    mean, w = rng.randn(6).astype(np.float32), np.linalg.qr(rng.randn(6, 6))[0][:2].astype(np.float32)
    np.savez(tmp_path / 'model.npz', mean=mean, components=w, explained_variance=np.array([2.0, 1.0]), explained_variance_ratio=np.array([.6, .3]),
             n_samples=50, whiten=False)
    monkeypatch.setattr(pca.PCA, 'transform', lambda self, X, to_device=False: R.project_ref(X, self.mean_, self.components_).astype(np.float32))
    monkeypatch.setattr(pca.PCA, 'close', lambda self: None)
    src = tmp_path / 'F'
    src.mkdir()
    clips = {}
    for name, frames in (('b', 3), ('a', 5)):
        clips[name] = dict(X=rng.randn(frames, 6).astype(np.float32), y=np.array(frames), file_idxs=np.array([[0, frames]]), note=np.array('x' + name))
        np.savez(src / (name + '.npz'), **clips[name])
    out = cli_pca.main(['transform', '--model', str(tmp_path / 'model.npz'), '--features', str(src), '--out', str(tmp_path / 'G')])
    assert [os.path.basename(p) for p in out] == ['a.npz', 'b.npz']
    for name, arrays in clips.items():
        with np.load(tmp_path / 'G' / (name + '.npz')) as npz:
            assert sorted(npz.files) == ['X', 'file_idxs', 'note', 'y']
            assert npz['X'].dtype == np.float32 and npz['X'].shape == (len(arrays['X']), 2)
            assert np.array_equal(npz['X'], R.project_ref(arrays['X'], mean, w).astype(np.float32))
            for key in ('y', 'file_idxs', 'note'):
                assert np.array_equal(npz[key], arrays[key]) and npz[key].dtype == arrays[key].dtype
    # one file in, one file out, under exactly the name given; a clip stored as (frames, 1, D) is taken as its frames
    np.savez(tmp_path / 'one.npz', X=clips['a']['X'].reshape(5, 1, 6), y=np.array(7))
    out = cli_pca.transform(str(tmp_path / 'model.npz'), str(tmp_path / 'one.npz'), str(tmp_path / 'one_out.npz'))
    assert out == [str(tmp_path / 'one_out.npz')]
    with np.load(out[0]) as npz:
        assert npz['X'].shape == (5, 2) and int(npz['y']) == 7
    # cli_knn's loader, which cli_cluster and cli_tsne share, reads the directory written
    from l3embedding_amd.cli_knn import _entries, _load
    X, entry, frame, label, names = _load(_entries([str(tmp_path / 'G')]))
    assert X.shape == (8, 2) and names == ['a', 'b'] and label.tolist() == [5] * 5 + [3] * 3
    np.savez(tmp_path / 'wide.npz', X=np.zeros((2, 7), np.float32), y=np.array(0))
    with pytest.raises(ValueError, match='7 features per frame'):
        cli_pca.transform(str(tmp_path / 'model.npz'), str(tmp_path / 'wide.npz'), str(tmp_path / 'w_out.npz'))


def test_cli_fit_writes_the_model_that_transform_reads(tmp_path, monkeypatch):
    rng = np.random.RandomState(6)
    X = R.embedding_like(rng, 40, 5)
    np.savez(tmp_path / 'clip.npz', X=X, y=np.array(1))
    monkeypatch.setattr(pca.PCA, 'fit', lambda self, rows: host_fit(self, rows))
    out = cli_pca.main(['fit', '--features', str(tmp_path / 'clip.npz'), '--n-components', '3', '--whiten', '--out', str(tmp_path / 'm.npz')])
    model = cli_pca.load_model(out)
    ref = host_fit(pca.PCA(3, whiten=True), X)
    assert model.whiten is True and model.n_components_ == 3
    for name in ('mean_', 'components_', 'explained_variance_', 'scale_'):
        assert np.array_equal(getattr(model, name), getattr(ref, name))
