"""Principal components on the GPU (csrc/pca.hip) against tests/pca_ref.py: the mean and the scatter matrix within the
derived bounds of float64, exact integer rows, the split rule bit for bit, the projection and its inverse, whole fits against the
full-float64 oracle, and the Python layers down to the command line.

Largest observed |S - S64| / bound over the cases of test_scatter_within_the_float64_bound (profiles/r38_pca.txt has the run):
0.050 (333, 19), 0.0819 (1000, 130), 0.0739 (300, 257), 0.0598 (129, 512), 0.0869 (2051, 40), 0.0372 (40, 6144).  Largest |y - y64| /
bound of test_transform_within_the_float64_bound: 0.198 (333, 19, 3) down to 0.0005 (129, 6144, 1), the same with and without a scale."""
import os

import numpy as np
import pytest

import pca_ref as R
from l3embedding_amd import _lib, cli_cluster, cli_pca, cluster, knn, pca, tsne, usc

pytestmark = pytest.mark.gpu

SHAPES = [(333, 19), (1000, 130), (300, 257), (129, 512), (2051, 40), (40, 6144)]
EXACT_SHAPES = [(600, 130), (514, 257)]
SPLIT_SHAPES = [(2051, 40), (1300, 257)]
SPLITS = (1, 2, 3, 7)
PROJECT_SHAPES = [(333, 19, 3), (1000, 130, 130), (300, 257, 129), (300, 257, 40), (129, 6144, 1)]
FIT_SHAPES = [(300, 40, None), (1000, 512, None), (129, 700, 20)]
U = R.U


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. and 2.: mean and scatter against float64 ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: '%d-%d' % s)
def moments(request, gpu_required):
    n, D = request.param
    X = R.embedding_like(np.random.RandomState(n + D), n, D)
    h = _lib.PCA(D)
    h.set_rows(X)
    m64, m32 = h.mean()
    again = h.mean()
    S = h.scatter()
    S_again = h.scatter()
    h.close()
    return dict(n=n, D=D, X=X, m64=m64, m32=m32, again=again, S=S, S_again=S_again)


def test_mean_within_the_float64_bound(moments):
    m64, m32 = moments['m64'], moments['m32']
    assert m64.dtype == np.float64 and m32.dtype == np.float32 and m64.shape == m32.shape == (moments['D'],)
    err, bound = np.abs(m64 - R.mean_ref(moments['X'])), R.mean_bound(moments['X'])
    print('mean %s: largest |m64 - ref| / bound %.3g' % ((moments['n'], moments['D']), np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)
    assert same_bits(m32, m64.astype(np.float32))
    assert same_bits(moments['again'][0], m64) and same_bits(moments['again'][1], m32)


def test_mean_follows_the_segment_order(moments):
    """the contract's order, replayed in NumPy float64: segments of 256 rows summed row by row, the segment sums added in order"""
    X = moments['X'].astype(np.float64)
    total = np.zeros(moments['D'])
    for lo in range(0, len(X), _lib.PCA_MEAN_SEG):
        seg = np.zeros(moments['D'])
        for row in X[lo:lo + _lib.PCA_MEAN_SEG]:
            seg = seg + row
        total = total + seg
    assert same_bits(moments['m64'], total / float(len(X)))


def test_scatter_within_the_float64_bound(moments):
    """the bound is derived (pca_ref.scatter_bound), not measured, and no entry is left out"""
    S, X, m32 = moments['S'], moments['X'], moments['m32']
    assert S.dtype == np.float64 and S.shape == (moments['D'], moments['D']) and np.all(np.isfinite(S))
    ref, bound = R.scatter_ref(X, m32), R.scatter_bound(X, m32)
    err = np.abs(S - ref)
    ratio = err / np.maximum(bound, 1e-300)
    print('scatter %s: largest |S - S64| / bound %.3g' % ((moments['n'], moments['D']), ratio.max()))
    assert np.all(err <= bound)
    assert np.all(bound[np.diag_indices(moments['D'])] > 0)          # every column varies: the bound is not an empty statement
    assert same_bits(S, np.ascontiguousarray(S.T))
    assert same_bits(S, moments['S_again'])


# ---- 3. exact integer rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda s: '%d-%d' % s)
def test_scatter_of_small_integers_is_exact(shape, gpu_required):
    """rows [Z; 2 c - Z]: the mean is the integer vector c exactly, every centred entry an integer of magnitude < 8, and every
    product and chain sum (at most 256 * 49) exact in float32: S must be the int64 Gram matrix.  Z is not symmetric in its columns,
    so a swap of the tile's two sides or of rows and columns inside it would show."""
    n, D = shape
    rng = np.random.RandomState(n * D)
    Z, c = rng.randint(0, 8, size=(n // 2, D)), rng.randint(0, 8, size=D)
    rows = np.concatenate([Z, 2 * c[None, :] - Z])
    rows = rows[rng.permutation(n)]
    h = _lib.PCA(D)
    h.set_rows(rows.astype(np.float32))
    m64, m32 = h.mean()
    assert np.array_equal(m64, c.astype(np.float64)) and np.array_equal(m32, c.astype(np.float32))
    want = R.gram_exact(rows, c)
    for splits in (0, 1, 2):
        S = h.scatter(splits)
        assert np.array_equal(S, want.astype(np.float64)), 'splits = %d' % splits
    h.close()


# ---- 4. splits ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=SPLIT_SHAPES, ids=lambda s: '%d-%d' % s)
def split_case(request, gpu_required):
    n, D = request.param
    X = R.embedding_like(np.random.RandomState(7 * n + D), n, D)
    h = _lib.PCA(D)
    h.set_rows(X)
    _, m32 = h.mean()
    got = {s: (h.scatter(s), h.scatter(s)) for s in SPLITS + (0,)}
    h.close()
    return dict(n=n, D=D, X=X, m32=m32, got=got, ref=R.scatter_ref(X, m32), bound=R.scatter_bound(X, m32))


@pytest.mark.parametrize('splits', SPLITS)
def test_splits_are_the_sum_of_their_ranges(split_case, splits):
    n, D, X, m32 = split_case['n'], split_case['D'], split_case['X'], split_case['m32']
    S, again = split_case['got'][splits]
    assert np.all(np.abs(S - split_case['ref']) <= split_case['bound'])
    assert same_bits(S, again) and same_bits(S, np.ascontiguousarray(S.T))
    # each range alone, by a handle that holds only that range with the same m32 set, summed in ascending order in NumPy float64
    total = None
    part = _lib.PCA(D)
    for lo, hi in R.split_ranges(n, splits):
        part.set_rows(X[lo:hi])
        part.set_mean(m32)
        P = part.scatter(1)
        total = P if total is None else total + P
    part.close()
    assert same_bits(S, total)


def test_zero_splits_is_the_count_the_header_names(split_case):
    n, D = split_case['n'], split_case['D']
    count = R.splits_ref(n, D)
    assert _lib.pca_splits(n, D) == count
    h = _lib.PCA(D)
    h.set_rows(split_case['X'])
    h.set_mean(split_case['m32'])
    S = h.scatter(count)
    h.close()
    assert same_bits(split_case['got'][0][0], S)
    for nn, dd in ((240000, 512), (60000, 6144), (100000, 19), (2, 1)):
        assert _lib.pca_splits(nn, dd) == R.splits_ref(nn, dd)


def test_rows_that_are_not_finite_are_refused_with_the_row_named(gpu_required):
    X = R.embedding_like(np.random.RandomState(0), 700, 33)
    X[612, 5], X[650, 0] = np.nan, np.inf
    h = _lib.PCA(33)
    with pytest.raises(_lib.L3Error, match='row 612 holds a NaN or an infinity'):
        h.set_rows(X)
    with pytest.raises(ValueError, match='set_rows comes first'):
        h.mean()
    X[612, 5] = 1.0
    dev = _lib.Features(X)
    with pytest.raises(_lib.L3Error, match='row 650 '):
        h.set_rows(dev)
    h.set_rows(dev, 0, 650)          # the rows before it are fine
    assert np.all(np.isfinite(h.mean()[0]))
    dev.close()
    h.close()


# ---- 5. transform and inverse through set_model ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=[(s, w) for s in PROJECT_SHAPES for w in (False, True)],
                ids=lambda p: '%d-%d-%d-%s' % (p[0] + ('scaled' if p[1] else 'plain',)))
def projection(request, gpu_required):
    (n, D, k), scaled = request.param
    rng = np.random.RandomState(n + D + k)
    X = R.embedding_like(rng, n, D)
    W = np.ascontiguousarray(np.linalg.qr(rng.randn(D, k))[0].T.astype(np.float32))          # (k, D), orthonormal rows
    mean = X.astype(np.float64).mean(axis=0).astype(np.float32)
    scale = np.exp(rng.uniform(-2, 2, size=k)).astype(np.float32) if scaled else None
    h = _lib.PCA(D)
    h.set_model(mean, W, scale)
    yield dict(n=n, D=D, k=k, X=X, W=W, mean=mean, scale=scale, h=h, Y=h.transform(X))
    h.close()


def test_transform_within_the_float64_bound(projection):
    p = projection
    Y = p['Y']
    assert Y.dtype == np.float32 and Y.shape == (p['n'], p['k'])
    err = np.abs(Y.astype(np.float64) - R.project_ref(p['X'], p['mean'], p['W'], p['scale']))
    bound = R.project_bound(p['X'], p['mean'], p['W'], p['scale'])
    print('transform %s: largest |y - y64| / bound %.3g' % ((p['n'], p['D'], p['k']), np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)


def test_transform_gives_the_same_bits_from_host_and_device_rows(projection):
    p, h = projection, projection['h']
    dev = _lib.Features(p['X'])
    assert same_bits(h.transform(dev), p['Y'])
    out = h.transform(dev, to_device=True)
    assert isinstance(out, _lib.Features) and out.shape == (p['n'], p['k']) and same_bits(out.download(), p['Y'])
    # rows [lo, hi) of a larger matrix: the bits of those rows transformed alone
    lo, hi = p['n'] // 3, p['n'] - 5
    alone = h.transform(np.ascontiguousarray(p['X'][lo:hi]))
    assert same_bits(alone, p['Y'][lo:hi])
    assert same_bits(h.transform(dev, lo, hi), alone) and same_bits(h.transform(p['X'], lo, hi), alone)
    part = h.transform(dev, lo, hi, to_device=True)
    assert part.shape == (hi - lo, p['k']) and same_bits(part.download(), alone)
    # and back, from the device result
    back = h.inverse(out)
    assert same_bits(back, h.inverse(p['Y'])) and same_bits(h.inverse(out, to_device=True).download(), back)
    assert same_bits(h.inverse(out, lo, hi), back[lo:hi])
    for f in (dev, out, part):
        f.close()


def test_inverse_within_the_float64_bound(projection):
    """the same float32 Y on both sides: the inverse's own arithmetic"""
    p = projection
    back = p['h'].inverse(p['Y'])
    assert back.dtype == np.float32 and back.shape == (p['n'], p['D'])
    err = np.abs(back.astype(np.float64) - R.inverse_ref(p['Y'], p['W'], p['mean'], p['scale']))
    assert np.all(err <= R.inverse_bound(p['Y'], p['W'], p['mean'], p['scale']))


@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'scaled'])
def test_inverse_of_transform_with_a_zero_mean_and_every_component(scaled, gpu_required):
    """k = D and a zero mean: inverse(transform(X)) against the float64 inverse of the float64 projection, within the two bounds
    added -- the projection's, carried through |W| (and the scale), and the inverse's own"""
    n, D = 300, 130
    rng = np.random.RandomState(11)
    X = R.embedding_like(rng, n, D)
    W = np.ascontiguousarray(np.linalg.qr(rng.randn(D, D))[0].T.astype(np.float32))
    zero = np.zeros(D, np.float32)
    scale = np.exp(rng.uniform(-2, 2, size=D)).astype(np.float32) if scaled else None
    h = _lib.PCA(D)
    h.set_model(zero, W, scale)
    Y = h.transform(X)
    back = h.inverse(Y)
    h.close()
    carried = R.project_bound(X, zero, W, scale)
    if scaled:
        carried = carried / scale.astype(np.float64)[None, :]
    bound = carried @ np.abs(W.astype(np.float64)) + R.inverse_bound(Y, W, zero, scale)
    err = np.abs(back.astype(np.float64) - R.inverse_ref(R.project_ref(X, zero, W, scale), W, zero, scale))
    assert np.all(err <= bound)
    assert np.max(np.abs(back - X)) < 1e-4 * np.max(np.abs(X))          # and it is X again, as far as float32 components are orthonormal


# ---- 6. fit end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=FIT_SHAPES, ids=lambda s: '%d-%d-%s' % s)
def fitted(request, gpu_required):
    n, D, rank = request.param
    rng = np.random.RandomState(n + D)
    if rank is None:
        X = R.embedding_like(rng, n, D)
    else:
        X = (rng.randn(n, rank) @ rng.randn(rank, D) + 1.0).astype(np.float32)
    model = pca.PCA(keep_covariance=True).fit(X)
    yield dict(n=n, D=D, rank=rank, X=X, model=model, ref=R.fit_ref(X))
    model.close()


def test_fit_against_the_full_float64_oracle(fitted):
    model, ref, D = fitted['model'], fitted['ref'], fitted['D']
    lam, C = model.explained_variance_, model.covariance_
    assert model.components_.dtype == np.float32 and model.components_.shape == (D, D) and model.mean_.dtype == np.float32
    assert lam.dtype == np.float64 and model.n_samples_ == fitted['n'] and model.n_components_ == D
    lam_max = ref['variance'][0]
    # Weyl: an eigenvalue moves by at most the norm of the perturbation; LAPACK's own error below D 2^-52 lam_max
    weyl = np.linalg.norm(C - ref['covariance'], 'fro') + D * 2.0 ** -52 * lam_max
    print('fit %s: largest |dlam| %.3g, Weyl bound %.3g' % ((fitted['n'], D), np.max(np.abs(lam - ref['variance'])), weyl))
    assert np.all(np.abs(lam - ref['variance']) <= weyl)
    assert np.all(lam >= 0) and np.all(np.diff(lam) <= 0)
    V = model.components_.astype(np.float64)
    assert np.max(np.abs(V @ V.T - np.eye(D))) <= 3 * U
    residual = np.linalg.norm(C @ V.T - V.T * lam[None, :], axis=0)
    print('fit %s: largest |V V^T - I| / u %.3g, largest residual / (u lam_max) %.3g' % (
        (fitted['n'], D), np.max(np.abs(V @ V.T - np.eye(D))) / U, residual.max() / (U * lam_max)))
    assert np.all(residual <= 2 * U * lam_max)
    assert np.array_equal(model.components_, R.sign_rule(model.components_))
    big = np.argmax(np.abs(model.components_), axis=1)
    assert np.all(model.components_[np.arange(D), big] > 0)
    assert abs(model.explained_variance_ratio_.sum() - 1.0) <= 1e-12
    assert np.all(np.abs(model.mean_.astype(np.float64) - ref['mean']) <= U * np.abs(ref['mean']) + R.mean_bound(fitted['X']))


def test_fractional_n_components_picks_the_oracles_count(fitted):
    X, ref = fitted['X'], fitted['ref']
    for share in (0.5, 0.9, 0.99):
        model = pca.PCA(share).fit(X)
        assert model.n_components_ == R.count_for_ref(ref['ratio'], share)
        assert model.components_.shape == (model.n_components_, fitted['D'])
        assert same_bits(model.components_, fitted['model'].components_[:model.n_components_])
        model.close()


def test_whiten_on_a_rank_deficient_input(fitted):
    if fitted['rank'] is None:
        model = pca.PCA(5, whiten=True).fit(fitted['X'])
        Y = model.transform(fitted['X'])
        assert np.allclose(Y.astype(np.float64).var(axis=0, ddof=1), 1.0, rtol=1e-3)          # unit variance: what whitening means
        model.close()
        return
    with pytest.raises(ValueError, match='whiten=True: component'):
        pca.PCA(whiten=True).fit(fitted['X'])
    model = pca.PCA(fitted['rank'], whiten=True).fit(fitted['X'])
    Y = model.transform(fitted['X'])
    assert Y.shape == (fitted['n'], fitted['rank'])
    assert np.allclose(Y.astype(np.float64).var(axis=0, ddof=1), 1.0, rtol=1e-3)
    assert np.allclose(model.inverse_transform(Y), fitted['X'], atol=1e-3 * np.abs(fitted['X']).max())
    model.close()


# ---- 7. use ------------------------------------------------------------------------------------------------------------------------------
def test_projected_device_features_go_into_the_other_models_as_they_are(gpu_required):
    rng = np.random.RandomState(21)
    centres = 4.0 * rng.randn(5, 40)
    X = (centres[rng.randint(0, 5, size=600)] + rng.randn(600, 40)).astype(np.float32)
    dev = usc.DeviceFeatures(X)
    model = pca.PCA(8)
    Y = model.fit_transform(dev, to_device=True)
    assert isinstance(Y, usc.DeviceFeatures) and Y.shape == (600, 8)
    rows = Y.to_host()
    assert same_bits(rows, model.transform(X)) and same_bits(rows, model.transform(dev))
    pair = []
    for given in (Y, rows):
        km = cluster.KMeans(5, n_init=2, max_iter=20, random_state=3).fit(given)
        nn = knn.NearestNeighbors(n_neighbors=6).fit(given)
        dist, idx = nn.kneighbors()
        ts = tsne.TSNE(perplexity=5.0, n_iter=10, exaggeration_iter=5, random_state=0, kl_every=5).fit(given)
        pair.append((km.labels_, km.cluster_centers_, km.inertia_, dist, idx, ts.embedding_))
        km.close()
        nn.close()
        ts.close()
    on_device, on_host = pair
    assert np.array_equal(on_device[0], on_host[0]) and same_bits(on_device[1], on_host[1]) and on_device[2] == on_host[2]
    assert same_bits(on_device[3], on_host[3]) and np.array_equal(on_device[4], on_host[4])
    assert same_bits(on_device[5], on_host[5])
    with pytest.raises(ValueError, match='to_device=True needs'):
        model.transform(X, to_device=True)
    back = model.inverse_transform(Y, to_device=True)
    assert isinstance(back, usc.DeviceFeatures) and back.shape == (600, 40)
    assert same_bits(back.to_host(), model.inverse_transform(rows))
    for f in (dev, Y, back):
        f.handle.close()
    model.close()


def test_cli_fit_then_transform_then_cluster(tmp_path, gpu_required):
    rng = np.random.RandomState(5)
    src = tmp_path / 'F'
    src.mkdir()
    clips = []
    for c in range(6):
        frames = rng.randint(20, 40)
        X = (3.0 * (c % 3) + rng.randn(frames, 24)).astype(np.float32)
        np.savez(src / ('clip%d.npz' % c), X=X, y=np.array(c % 3))
        clips.append(X)
    model_path = cli_pca.main(['fit', '--features', str(src), '--n-components', '4', '--whiten', '--out', str(tmp_path / 'model.npz')])
    out = cli_pca.main(['transform', '--model', model_path, '--features', str(src), '--out', str(tmp_path / 'G')])
    assert len(out) == 6
    ref = pca.PCA(4, whiten=True).fit(np.concatenate(clips))
    for c, X in enumerate(clips):
        with np.load(tmp_path / 'G' / ('clip%d.npz' % c)) as npz:
            assert same_bits(npz['X'], ref.transform(X)) and int(npz['y']) == c % 3
    ref.close()
    cluster_path = cli_cluster.main(['fit', '--features', str(tmp_path / 'G'), '--clusters', '3', '--seed', '1', '--n-init', '2', '--out',
                                     str(tmp_path / 'km.npz')])
    with np.load(cluster_path) as npz:
        assert npz['centroids'].shape == (3, 4) and len(npz['labels']) == sum(len(X) for X in clips)
        assert 0.0 <= float(npz['purity']) <= 1.0
    assert os.path.exists(cluster_path)
