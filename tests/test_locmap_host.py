"""Host tests of the sound localisation maps: the NumPy oracle of tests/locmap_ref.py against plain loops, the CSR
builder, crossmodal.upsample_map against the per-pixel formula, and the Python layer's refusals -- nothing here needs a GPU."""
import math

import numpy as np
import pytest

from l3embedding_amd import _lib, cli_retrieval, crossmodal

import locmap_ref as R


# ---- the oracle against loops ----------------------------------------------------------------------------------------------------
def _loop_margin(mrow, trow, wd, bd):
    acc = 0.0
    for k in range(len(wd)):
        acc += max(float(mrow[k]) + float(trow[k]), 0.0) * float(wd[k])
    return acc + float(bd)


def _loop_peak(row):
    """the order of a peak, location by location"""
    best, at = -math.inf, -1
    for l, m in enumerate(row):
        if m != m:
            continue
        if at < 0 or m > best:          # equal margins: the earlier location stays
            best, at = float(m), l
    return best, at


def test_maps_ref_against_loops():
    rng = np.random.RandomState(0)
    n, L, nq, H = 2, 3, 4, 5
    m, t, wd, bd = rng.randn(n * L, H), rng.randn(nq, H), rng.randn(H), 0.25
    got = R.maps_ref(m, t, wd, bd, L)
    assert got.shape == (n, nq, L)
    for i in range(n):
        for j in range(nq):
            for l in range(L):
                assert abs(got[i, j, l] - _loop_margin(m[i * L + l], t[j], wd, bd)) < 1e-12
    b = R.maps_bound(m, t, wd, bd, L)
    assert b.shape == got.shape and np.all(b > 0)
    assert np.allclose(b[1, 2], R.margins_bound(m[L:], t[2:3], wd, bd)[:, 0], rtol=1e-12, atol=0)          # that pair's own bound


def test_peaks_ref_against_loops_with_ties_and_nans():
    nan, inf = np.nan, np.inf
    maps = np.array([[[1.0, 3.0, 2.0], [2.0, 2.0, 1.0]],           # a plain maximum; a tie: the smaller location
                     [[nan, -1.0, -1.0], [nan, nan, nan]],         # a NaN never wins; every margin NaN
                     [[0.0, -0.0, nan], [-inf, nan, -inf]],        # +0 == -0: the first; a real -inf is a margin
                     [[nan, nan, 5.0], [inf, inf, 1.0]]], np.float32)
    peak, arg = R.peaks_ref(maps)
    assert peak.dtype == np.float32 and arg.dtype == np.int32
    for i in range(maps.shape[0]):
        for j in range(maps.shape[1]):
            want, at = _loop_peak(maps[i, j])
            assert arg[i, j] == at and (peak[i, j] == want), (i, j)
    assert arg.tolist() == [[1, 0], [1, -1], [0, 0], [2, 0]]
    assert peak[1, 1] == -inf and peak[2, 1] == -inf and not np.signbit(peak[2, 0])
    rng = np.random.RandomState(1)
    maps = rng.randint(-2, 3, (2, 3, 3)).astype(np.float64)          # 2 items x 3 queries x 3 locations, many ties
    maps[rng.rand(2, 3, 3) < 0.3] = nan
    peak, arg = R.peaks_ref(maps)
    for i in range(2):
        for j in range(3):
            want, at = _loop_peak(maps[i, j])
            assert arg[i, j] == at and peak[i, j] == want


def test_peak_ranks_ref_is_the_rank_count_over_S():
    rng = np.random.RandomState(2)
    S = rng.randint(0, 4, (5, 6)).astype(np.float32)          # ties with the truth: not counted
    ta, tv = rng.randint(0, 6, 5), rng.randint(0, 5, 6)
    gv, ga = rng.randint(0, 3, 5), rng.randint(0, 3, 6)
    for groups in (None, (gv, ga)):
        rv, ra = R.peak_ranks_ref(S, ta, tv, *(groups or (None, None)))
        for i in range(5):
            assert rv[i] == sum(1 for j in range(6) if S[i, j] > S[i, ta[i]] and (groups is None or gv[i] != ga[j]))
        for j in range(6):
            assert ra[j] == sum(1 for i in range(5) if S[i, j] > S[tv[j], j] and (groups is None or gv[i] != ga[j]))
    assert R.peak_ranks_ref(S, ta)[1] is None


# ---- the CSR builder -------------------------------------------------------------------------------------------------------------
def test_csr_round_trip_of_the_caller_s_order():
    items = np.array([3, 0, 3, 5, 0, 3, 5], np.int64)          # repeated items; 1, 2, 4 and 6 absent
    queries = np.array([10, 11, 12, 13, 14, 15, 16])
    ptr, order = _lib.csr_by_item(items, 7)
    assert ptr.dtype == np.int64 and ptr.tolist() == [0, 2, 2, 2, 5, 5, 7, 7]
    assert order.tolist() == [1, 4, 0, 2, 5, 3, 6]              # stable: a repeated item keeps the caller's order
    q = queries[order]
    for i in range(7):
        assert sorted(q[ptr[i]:ptr[i + 1]].tolist()) == sorted(queries[items == i].tolist())
    result = q * 2                                              # what a kernel gives in CSR order ...
    back = np.empty_like(result)
    back[order] = result
    assert back.tolist() == (queries * 2).tolist()              # ... returns in the caller's
    p2, q2 = _lib.csr_check(ptr, q, 7, 17)
    assert p2.dtype == np.int64 and q2.dtype == np.int32
    with pytest.raises(ValueError, match='outside'):
        _lib.csr_by_item(np.array([0, 7]), 7)
    for bad_ptr, bad_q, why in (([0, 1], [0], 'integers'), ([1, 1, 1, 1, 1, 1, 1, 7], q, 'start at 0'), ([0, 2, 1, 2, 5, 5, 7, 7], q, 'decrease'),
                                (ptr, q[:-1], 'item_ptr'), (np.zeros(8, np.int64), [], '>= 1'), (ptr, q + 1, 'outside'), (None, q, 'None')):
        with pytest.raises(ValueError, match=why):
            _lib.csr_check(bad_ptr, bad_q, 7, 17)


# ---- upsample_map ----------------------------------------------------------------------------------------------------------------
def _upsample_loop(m, oh, ow):
    H, W = m.shape
    out = np.empty((oh, ow))
    for y in range(oh):
        sy = min(max((y + 0.5) * H / oh - 0.5, 0.0), H - 1.0)
        y0 = int(math.floor(sy))
        y1, fy = min(y0 + 1, H - 1), sy - int(math.floor(sy))
        for x in range(ow):
            sx = min(max((x + 0.5) * W / ow - 0.5, 0.0), W - 1.0)
            x0 = int(math.floor(sx))
            x1, fx = min(x0 + 1, W - 1), sx - int(math.floor(sx))
            out[y, x] = (1 - fy) * ((1 - fx) * m[y0, x0] + fx * m[y0, x1]) + fy * ((1 - fx) * m[y1, x0] + fx * m[y1, x1])
    return out


@pytest.mark.parametrize('shape,size', [((28, 28), (224, 224)), ((3, 5), (7, 4)), ((1, 1), (3, 2)), ((4, 6), (4, 6)), ((32, 24), (5, 9))])
def test_upsample_map_against_the_per_pixel_formula(shape, size):
    m = np.random.RandomState(shape[0]).randn(*shape)
    got = crossmodal.upsample_map(m, size)
    assert got.shape == size and got.dtype == np.float64
    assert np.abs(got - _upsample_loop(m, *size)).max() < 1e-12
    assert got.min() >= m.min() - 1e-12 and got.max() <= m.max() + 1e-12          # an interpolation: inside the data's range
    if shape == size:
        assert np.array_equal(got, m)


def test_upsample_map_batches_dtype_and_refusals():
    m = np.random.RandomState(3).randn(2, 3, 4, 5).astype(np.float32)
    got = crossmodal.upsample_map(m, 8)
    assert got.shape == (2, 3, 8, 8) and got.dtype == np.float32
    assert np.abs(got[1, 2] - _upsample_loop(m[1, 2].astype(np.float64), 8, 8)).max() < 1e-6
    assert np.array_equal(crossmodal.upsample_map(np.full((2, 2), 3.0), (5, 5)), np.full((5, 5), 3.0))
    for bad_m, bad_size in ((np.zeros(4), 8), (np.zeros((2, 2), np.int32), 8), (np.zeros((2, 2)), 0), (np.zeros((2, 2)), (1, 2, 3))):
        with pytest.raises(ValueError):
            crossmodal.upsample_map(bad_m, bad_size)


# ---- refusals of the Python layer, before any device is touched ------------------------------------------------------------------------
def test_pairs_map_refusals_need_no_device():
    p = _lib.Pairs(512, 512, 128)
    for side, n, H, W in ((2, 1, 1, 1), (0, 0, 28, 28), (0, 4, 0, 28), (1, 2 ** 31, 1, 1)):
        with pytest.raises(ValueError):
            p.map_reserve(side, n, H, W)
    with pytest.raises(ValueError, match='map_reserve'):
        p.map_put(None, 0, 0, 1)
    for call in (lambda: p.map_list([0, 1], [0]), lambda: p.map_peaks(), lambda: p.map_ranks(np.zeros(1, np.int32)), lambda: p.map_time('peaks')):
        with pytest.raises(ValueError, match='come first'):
            call()
    with pytest.raises(ValueError, match='one of'):
        p.map_time('matrix')
    assert p.h is None          # no handle was created: nothing reached the library


def test_operator_refusals_need_no_device():
    H, L = 32, 3
    m, t, wd = np.zeros((2 * L, H), np.float32), np.zeros((4, H), np.float32), np.zeros(H, np.float32)
    bad = [lambda: _lib.op_map_list(m[:5], t, wd, 0.0, L, [0, 1, 1], [0]),                       # rows not a multiple of L
           lambda: _lib.op_map_list(m, t, wd, 0.0, 0, [0, 1, 1], [0]),
           lambda: _lib.op_map_list(m, t[:, :16], wd, 0.0, L, [0, 1, 1], [0]),
           lambda: _lib.op_map_list(np.zeros((6, 48), np.float32), np.zeros((4, 48), np.float32), np.zeros(48, np.float32), 0.0, L, [0, 1, 1], [0]),
           lambda: _lib.op_map_list(m, t, wd, 0.0, L, [0, 1, 1], [4]),                           # a query out of range
           lambda: _lib.op_map_list(m, t, wd, 0.0, L, [0, 1], [0]),                              # one offset per item and the end
           lambda: _lib.op_map_list(m, t, wd, 0.0, L, [0, 1, 1], [0], maps=False, peaks=False),
           lambda: _lib.op_map_peaks(m, t, wd, 0.0, L, 0, 3),
           lambda: _lib.op_map_peaks(m, t, wd, 0.0, L, 1, 1),
           lambda: _lib.op_map_peaks(m, t, wd, 0.0, L, 0, 2, 2, 5)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()


def test_evaluate_bank_and_cli_refuse_map_options_before_anything_runs(capsys):
    for kw in ({'maps_top': 0}, {'maps_top': 1, 'peak': True}, {'maps_top': -1, 'peak': True, 'topk': 4}, {'maps_top': 5, 'peak': True, 'topk': 4}):
        with pytest.raises(ValueError, match='maps_top'):
            crossmodal.evaluate_bank(None, None, **kw)
    for argv in (['w.h5', 'tiny_L3', 'c.npz', '--maps-top', '2'],                                          # no --maps-path
                 ['w.h5', 'tiny_L3', 'c.npz', '--maps-path', 'm.npz', '--maps-top', '2'],                    # no --top-k
                 ['w.h5', 'tiny_L3', 'c.npz', '--maps-path', 'm.npz', '--top-k', '2', '--maps-top', '3']):
        with pytest.raises(SystemExit) as exc:
            cli_retrieval.main(argv)
        assert exc.value.code == 2
    assert '--maps-top' in capsys.readouterr().err
