"""GPU tests of the sound localisation maps (csrc/locmap.hip, the location entry points of csrc/engine.hip, crossmodal.PairScorer's map
side).  The map kernel alone through l3_op_map_list / l3_op_map_peaks at the smallest shapes that cross every edge
(two tiles of locations with the second ragged, the real 784 once, one location; 1, 64 and 70 queries; head 32 and 128): every stored
margin bit-equal to the pair kernel's and within tests/pairs_ref.py's bound of float64, peak and arg equal to the order of a peak
applied to the GPU's own map, peaks and list bit-equal for any block and grouping, planted ties and NaNs, the rank mode against the
NumPy count over the GPU's own S.  Then the engine's location rows against what the project had (l3_tower_features,
l3_get_activation) and the scorer's maps against l3_pairs_list over the same rows set as items."""
import numpy as np
import pytest

from l3embedding_amd import _lib, avsample, crossmodal, model
from oracle import l3_oracle as o

import locmap_ref as R

pytestmark = pytest.mark.gpu

TILE = 64          # locations and queries of one accumulation (L3_PAIRS_TILE)
ITEMS = 3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _all_pairs(n_items, nq):
    """every (item, query) pair in CSR form by item, the queries in order"""
    return np.arange(n_items + 1, dtype=np.int64) * nq, np.tile(np.arange(nq, dtype=np.int32), n_items)


def _inputs(seed, L, nq, H):
    rng = np.random.RandomState(seed)
    return (rng.randn(ITEMS * L, H).astype(np.float32), rng.randn(nq, H).astype(np.float32), rng.randn(H).astype(np.float32),
            np.float32(-0.37))


def _order_holds(maps, peak, arg):
    """peak and arg are the order of a peak applied to these very maps: every pair, bit for bit"""
    want_peak, want_arg = R.peaks_ref(maps)
    assert np.array_equal(arg, want_arg)
    assert np.array_equal(bits(peak), bits(want_peak))


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------
SHAPES = [(70, 1, 32), (70, 64, 128), (70, 70, 32), (70, 70, 128), (1, 70, 32), (1, 1, 128), (1, 64, 32), (784, 70, 128)]


@pytest.mark.parametrize('L,nq,H', SHAPES)
def test_map_kernel_margins_peaks_and_groupings(gpu_required, L, nq, H):
    m, t, wd, bd = _inputs(L + nq + H, L, nq, H)
    ptr, q = _all_pairs(ITEMS, nq)
    maps, peak, arg = _lib.op_map_list(m, t, wd, bd, L, ptr, q)
    assert maps.shape == (ITEMS * nq, L)
    maps = maps.reshape(ITEMS, nq, L)
    # the chain is the pair kernel's: the same bits as its matrix of (location row, query) margins
    pair = _lib.op_pair_margins(m, t, wd, bd).reshape(ITEMS, L, nq).transpose(0, 2, 1)
    assert np.array_equal(bits(maps), bits(pair))
    # ... and within the pair's bound of float64
    ref, bound = R.maps_ref(m, t, wd, bd, L), R.maps_bound(m, t, wd, bd, L)
    err = np.abs(maps - ref)
    print('L=%d nq=%d H=%d: worst error / bound %.3f' % (L, nq, H, float((err / bound).max())))
    assert np.all(err <= bound)
    # peak and arg: the order applied to the GPU's own stored map, every pair
    _order_holds(maps, peak.reshape(ITEMS, nq), arg.reshape(ITEMS, nq))
    if L == 1:
        assert not arg.any()
    # the peaks mode: the same bits, for the whole block and for blocks of it
    S, A = _lib.op_map_peaks(m, t, wd, bd, L)
    assert S.shape == (ITEMS, nq) and np.array_equal(bits(S), bits(peak.reshape(ITEMS, nq))) and np.array_equal(A, arg.reshape(ITEMS, nq))
    for i0, i1, j0, j1 in ((1, 3, 0, nq), (0, 1, nq - 1, nq), (2, 3, nq // 2, nq), (0, 3, max(0, nq - 65), nq)):
        Sb, Ab = _lib.op_map_peaks(m, t, wd, bd, L, i0, i1, j0, j1)
        assert np.array_equal(bits(Sb), bits(S[i0:i1, j0:j1])) and np.array_equal(Ab, A[i0:i1, j0:j1])
    # any CSR grouping of the same pairs: shuffled, repeated and absent queries, an item without any; peaks without maps
    rng = np.random.RandomState(L)
    counts = [min(nq, 3), 0, 2 * nq + 5]          # item 2 lists more than two workgroups' worth, with repeats
    qs = [rng.randint(0, nq, c).astype(np.int32) for c in counts]
    ptr2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    m2, p2, a2 = _lib.op_map_list(m, t, wd, bd, L, ptr2, np.concatenate(qs))
    items = np.repeat(np.arange(ITEMS), counts)
    assert np.array_equal(bits(m2), bits(maps[items, np.concatenate(qs)]))
    assert np.array_equal(bits(p2), bits(S[items, np.concatenate(qs)])) and np.array_equal(a2, A[items, np.concatenate(qs)])
    none, p3, a3 = _lib.op_map_list(m, t, wd, bd, L, ptr2, np.concatenate(qs), maps=False)
    assert none is None and np.array_equal(bits(p3), bits(p2)) and np.array_equal(a3, a2)
    m4, p4, a4 = _lib.op_map_list(m, t, wd, bd, L, ptr2, np.concatenate(qs), peaks=False)
    assert p4 is None and a4 is None and np.array_equal(bits(m4), bits(m2))


def test_planted_ties_go_to_the_smaller_location(gpu_required):
    """Duplicate location rows in different tiles, in one tile across lanes, and inside one lane's four locations; the duplicated row
    is built to be every query's peak (large where wd > 0, very negative where wd < 0), so the tie is at the top."""
    L, nq, H = 130, 70, 32
    m, t, wd, bd = _inputs(5, L, nq, H)
    top = np.where(wd > 0, 10.0, -50.0).astype(np.float32)
    m = m.reshape(ITEMS, L, H)
    firsts = []
    for i, places in enumerate(((100, 5, 129), (9, 7), (66, 65, 64, 128))):
        for l in places:
            m[i, l] = top
        firsts.append(min(places))
    m[0, 77] = m[0, 3]          # a tie below the top changes nothing
    m = m.reshape(ITEMS * L, H)
    maps, peak, arg = _lib.op_map_list(m, t, wd, bd, L, *_all_pairs(ITEMS, nq))
    maps, arg = maps.reshape(ITEMS, nq, L), arg.reshape(ITEMS, nq)
    assert np.array_equal(bits(maps[0, :, 100]), bits(maps[0, :, 5])) and np.array_equal(bits(maps[0, :, 77]), bits(maps[0, :, 3]))
    for i in range(ITEMS):
        assert np.all(arg[i] == firsts[i]), i
    _order_holds(maps, peak.reshape(ITEMS, nq), arg)
    S, A = _lib.op_map_peaks(m, t, wd, bd, L)
    assert np.array_equal(bits(S), bits(peak.reshape(ITEMS, nq))) and np.array_equal(A, arg)


def test_planted_nans_never_win(gpu_required):
    """item 0: one location whose margin is NaN with every query; item 1: every location so; item 2: untouched.  The chain's
    max(u + t, 0) turns a NaN unit into 0 (fmaxf), so a NaN margin is planted as +inf - inf: an infinite unit where wd > 0 and
    another where wd < 0."""
    L, nq, H = 70, 70, 32
    m, t, wd, bd = _inputs(6, L, nq, H)
    clean = _lib.op_map_peaks(m, t, wd, bd, L)
    up, down = int(np.flatnonzero(wd > 0)[0]), int(np.flatnonzero(wd < 0)[0])
    m = m.reshape(ITEMS, L, H)
    m[0, 67, [up, down]] = np.inf
    m[1][:, [up, down]] = np.inf
    m = m.reshape(ITEMS * L, H)
    maps, peak, arg = _lib.op_map_list(m, t, wd, bd, L, *_all_pairs(ITEMS, nq))
    maps, peak, arg = maps.reshape(ITEMS, nq, L), peak.reshape(ITEMS, nq), arg.reshape(ITEMS, nq)
    assert np.all(np.isnan(maps[0, :, 67])) and not np.isnan(np.delete(maps[0], 67, axis=1)).any() and np.all(np.isnan(maps[1]))
    assert np.all(arg[0] != 67) and np.all(arg[0] >= 0) and np.all(np.isfinite(peak[0]))
    assert np.all(arg[1] == -1) and np.all(np.isneginf(peak[1]))
    _order_holds(maps, peak, arg)
    S, A = _lib.op_map_peaks(m, t, wd, bd, L)
    assert np.array_equal(bits(S), bits(peak)) and np.array_equal(A, arg)
    assert np.array_equal(bits(S[2]), bits(clean[0][2])) and np.array_equal(A[2], clean[1][2])


AGAINST64 = dict(seed=11, L=70, nq=70, H=128)


def _exempt_share(m, t, wd, bd, L):
    """float64 alone: (ref, bound, peak64, arg64, exempt) -- a pair is exempt from the arg-max comparison when its float64 runner-up
    is within twice the largest bound of its locations"""
    ref, bound = R.maps_ref(m, t, wd, bd, L), R.maps_bound(m, t, wd, bd, L)
    peak64, arg64 = R.peaks_ref(ref)
    if L == 1:
        return ref, bound, peak64, arg64, np.zeros(peak64.shape, bool)
    second = np.sort(ref, axis=-1)[..., -2]
    return ref, bound, peak64, arg64, (peak64 - second) <= 2.0 * bound.max(axis=-1)


def test_peaks_against_float64(gpu_required):
    """|peak - peak64| <= the larger of the pair's bounds at the two arg-max locations (peak32 = m32[a32] <= m64[a32] + b[a32] <=
    peak64 + b[a32], and peak32 >= m32[a64] >= peak64 - b[a64]); arg equals the float64 arg-max except where the float64 runner-up is
    within twice the pair's bound.  Seed 11, 3 items x 70 queries x 70 locations, head 128: 1 of the 210 pairs (0.48 %) falls under that
    exemption by the float64 reference alone (the smallest gap between a peak and its runner-up is 5.5e-4, the largest bound 7.9e-4;
    the same chain in float32 NumPy finds the float64 arg-max in all 210); the cap is 10 %."""
    c = AGAINST64
    m, t, wd, bd = _inputs(c['seed'], c['L'], c['nq'], c['H'])
    ref, bound, peak64, arg64, exempt = _exempt_share(m, t, wd, bd, c['L'])
    share = float(exempt.mean())
    print('exempt share %.4f; smallest gap %.3e, largest bound %.3e' % (share, float((peak64 - np.sort(ref, axis=-1)[..., -2]).min()),
                                                                       float(bound.max())))
    assert share <= 0.10
    S, A = _lib.op_map_peaks(m, t, wd, bd, c['L'])
    assert np.all(A >= 0)
    b32 = np.take_along_axis(bound, A[..., None].astype(np.int64), axis=-1)[..., 0]
    b64 = np.take_along_axis(bound, arg64[..., None].astype(np.int64), axis=-1)[..., 0]
    assert np.all(np.abs(S - peak64) <= np.maximum(b32, b64))
    assert np.all((A == arg64) | exempt)


# ---- the handle: ranks over S, state, the C ABI's refusals ----------------------------------------------------------------------------
def _head(rng, nv, na, H):
    return ((rng.randn(nv + na, H) / np.sqrt(nv + na)).astype(np.float32), rng.randn(H).astype(np.float32),
            rng.randn(H, 2).astype(np.float32), rng.randn(2).astype(np.float32))


@pytest.fixture(scope='module')
def mapped70(gpu_required):
    """70 frames of 70 locations (40 channels) and 70 seconds (24 wide), head 64; the seconds of the second half are bit-for-bit
    copies of the first half's, so every truth column has a twin and ties with the truth exist.  Clip groups of sizes 1 .. 7."""
    rng = np.random.RandomState(70)
    nv, na, H, n, L = 40, 24, 64, 70, 70
    head = _head(rng, nv, na, H)
    loc = rng.randn(n * L, nv).astype(np.float32)
    A = rng.randn(n, na).astype(np.float32)
    A[35:] = A[:35]
    groups, g = [], 0
    while len(groups) < n:
        groups += [g] * (g % 7 + 1)
        g += 1
    p = _lib.Pairs(nv, na, H)
    p.set_head(*head)
    p.set_audio(A)
    f = _lib.Features(loc)
    p.map_reserve(0, n, 7, 10)
    p.map_put(f, 35 * L, 35, 35)          # in two chunks, the second first
    p.map_put(f, 0, 0, 35)
    S, arg = p.map_peaks()
    yield dict(p=p, f=f, loc=loc, A=A, head=head, groups=np.array(groups[:n], np.int32), n=n, L=L, S=S, arg=arg)
    p.close()
    f.close()


def _rank_cases(n, g):
    diag = np.arange(n)
    perm = np.random.RandomState(7).permutation(n)
    many = np.random.RandomState(8).randint(0, n, n)          # not a permutation: several frames share a second
    return [(diag, diag, None), (diag, diag, g), (perm, np.argsort(perm), g), (many, many[::-1].copy(), None), (perm, None, g),
            (None, np.argsort(perm), None)]


def test_map_ranks_equal_the_numpy_count_over_the_gpu_s_own_S(mapped70):
    s = mapped70
    p, S, n = s['p'], s['S'], s['n']
    assert np.array_equal(bits(S[:, 35:]), bits(S[:, :35]))          # the twins tie bit for bit
    ties = False
    for ta, tv, groups in _rank_cases(n, s['groups']):
        rv, ra = p.map_ranks(ta, tv, groups, groups)
        wv, wa = R.peak_ranks_ref(S, ta, tv, groups, groups)
        for got, want in ((rv, wv), (ra, wa)):
            assert (got is None) == (want is None)
            if want is not None:
                assert got.dtype == np.int32 and np.array_equal(got, want)
        if ta is not None and groups is None:
            ties = ties or bool(np.any((S == S[np.arange(n), ta][:, None]).sum(axis=1) > 1))
    assert ties          # the strict comparison was exercised
    a, b = p.map_ranks(np.arange(n), np.arange(n), s['groups'], s['groups']), p.map_ranks(np.arange(n), np.arange(n), s['groups'], s['groups'])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])          # run to run


def test_handle_maps_have_the_bits_of_the_rows_set_as_items(mapped70):
    """the map of (frame i, second j) is l3_pairs_list over frame i's location rows set as items; its peak is S_ij"""
    s = mapped70
    p, n, L = s['p'], s['n'], s['L']
    rng = np.random.RandomState(3)
    iv, ia = rng.randint(0, n, 40), rng.randint(0, n, 40)
    ptr, order = _lib.csr_by_item(iv, n)
    maps, peak, arg = p.map_list(ptr, ia[order].astype(np.int32))
    assert np.array_equal(bits(peak), bits(s['S'][iv[order], ia[order]])) and np.array_equal(arg, s['arg'][iv[order], ia[order]])
    p.set_vision(s['f'])          # every location row an item: 4900 of them
    rows = (iv[order][:, None] * L + np.arange(L)[None, :]).reshape(-1)
    want = p.list(rows, np.repeat(ia[order], L)).reshape(40, L)
    assert np.array_equal(bits(maps), bits(want))


def test_audio_side_map_and_ranks(gpu_required):
    """side 1: the seconds' locations (W1a, + b1) queried by the frames; S comes back as items x queries = seconds x frames"""
    rng = np.random.RandomState(9)
    nv, na, H, nf, ns, L = 24, 40, 32, 66, 5, 6
    head = _head(rng, nv, na, H)
    V, loc = rng.randn(nf, nv).astype(np.float32), rng.randn(ns * L, na).astype(np.float32)
    p, f = _lib.Pairs(nv, na, H), _lib.Features(loc)
    p.set_head(*head)
    p.set_vision(V)
    p.map_reserve(1, ns, 2, 3)
    p.map_put(f, 0, 0, ns)
    S, arg = p.map_peaks()
    assert S.shape == (ns, nf)
    maps, peak, _ = p.map_list(*_all_pairs(ns, nf))
    p.set_audio(f)          # the location rows as seconds: the same bits from the pair kernel
    M = p.matrix()          # (nf, ns L)
    assert np.array_equal(bits(maps.reshape(ns, nf, L)), bits(M.reshape(nf, ns, L).transpose(1, 0, 2)))
    assert np.array_equal(bits(peak.reshape(ns, nf)), bits(S))
    ta, tv = rng.randint(0, ns, nf), rng.randint(0, nf, ns)
    gv, ga = rng.randint(0, 3, nf), rng.randint(0, 3, ns)
    for groups in ((None, None), (gv, ga)):
        rv, ra = p.map_ranks(ta, tv, *groups)
        wv, wa = R.peak_ranks_ref(S.T, ta, tv, *groups)          # frames x seconds
        assert np.array_equal(rv, wv) and np.array_equal(ra, wa)
    p.close(), f.close()


def test_library_refuses_bad_map_arguments_and_states(mapped70):
    s = mapped70
    p = s['p']
    lib, h, ptr = p.lib, p.h, _lib._ptr
    n = s['n']
    out, idx = np.zeros(n * n, np.float32), np.zeros(n * n, np.int32)
    good_ptr, q = _all_pairs(n, 1)
    bad_q = q.copy()
    bad_q[5] = n
    dec = good_ptr.copy()
    dec[3] = 9
    t_ok, t_bad = np.zeros(n, np.int32), np.full(n, n, np.int32)
    wrong = _lib.Features(np.zeros((70, 39), np.float32))
    calls = [lambda: lib.l3_pairs_map_reserve(h, 2, 1, 1, 1), lambda: lib.l3_pairs_map_reserve(h, 0, 1, 0, 4),
             lambda: lib.l3_pairs_map_put(h, None, 0, 0, 1), lambda: lib.l3_pairs_map_put(h, wrong.h, 0, 0, 1),
             lambda: lib.l3_pairs_map_put(h, s['f'].h, 0, 69, 2), lambda: lib.l3_pairs_map_put(h, s['f'].h, 69 * 70 + 1, 0, 1),
             lambda: lib.l3_pairs_map_list(h, ptr(good_ptr), ptr(bad_q), ptr(out), None, None),
             lambda: lib.l3_pairs_map_list(h, ptr(dec), ptr(q), ptr(out), None, None),
             lambda: lib.l3_pairs_map_list(h, ptr(good_ptr), ptr(q), None, None, None),
             lambda: lib.l3_pairs_map_list(h, None, ptr(q), ptr(out), None, None),
             lambda: lib.l3_pairs_map_peaks(h, 0, n + 1, 0, n, ptr(out), ptr(idx)), lambda: lib.l3_pairs_map_peaks(h, 3, 3, 0, n, ptr(out), None),
             lambda: lib.l3_pairs_map_peaks(h, 0, 1, 0, 1, None, None),
             lambda: lib.l3_pairs_map_ranks(h, ptr(t_bad), None, None, None, ptr(idx), None),
             lambda: lib.l3_pairs_map_ranks(h, ptr(t_ok), None, ptr(t_ok), None, ptr(idx), None),
             lambda: lib.l3_pairs_map_ranks(h, ptr(t_ok), None, None, None, None, None),
             lambda: lib.l3_pairs_map_time(h, 3, 1, None)]
    for k, call in enumerate(calls):
        assert call() == -1, k          # L3_EINVAL
        assert lib.l3_last_error(None), k
    wrong.close()
    S, arg = p.map_peaks()
    assert np.array_equal(bits(S), bits(s['S'])) and np.array_equal(arg, s['arg'])          # nothing happened to the map
    # L3_ESTATE: a fresh handle step by step, and a map voided by a new head
    q2 = _lib.Pairs(40, 24, 64)
    q2._handle()
    one = np.zeros(1, np.float32)
    assert q2.lib.l3_pairs_map_peaks(q2.h, 0, 1, 0, 1, ptr(one), None) == -4 and b'set_head' in q2.lib.l3_last_error(None)
    q2.set_head(*s['head'])
    assert q2.lib.l3_pairs_map_peaks(q2.h, 0, 1, 0, 1, ptr(one), None) == -4 and b'reserve' in q2.lib.l3_last_error(None)
    assert q2.lib.l3_pairs_map_put(q2.h, s['f'].h, 0, 0, 1) == -4
    q2.map_reserve(0, 2, 7, 10)
    q2.map_put(s['f'], 0, 0, 1)
    assert q2.lib.l3_pairs_map_peaks(q2.h, 0, 1, 0, 1, ptr(one), None) == -4 and b'put' in q2.lib.l3_last_error(None)
    q2.map_put(s['f'], 70, 1, 1)
    assert q2.lib.l3_pairs_map_peaks(q2.h, 0, 1, 0, 1, ptr(one), None) == -4 and b'l3_pairs_set_audio' in q2.lib.l3_last_error(None)
    q2.set_audio(s['A'])
    assert np.array_equal(bits(q2.map_peaks()[0]), bits(s['S'][:2]))
    q2.set_head(*s['head'])          # voids the sets and what was put
    assert q2.lib.l3_pairs_map_peaks(q2.h, 0, 1, 0, 1, ptr(one), None) == -4
    with pytest.raises(ValueError, match='come first'):
        q2.map_peaks()
    q2.close()


def test_map_time_runs(mapped70):
    for what in ('list', 'peaks', 'ranks'):
        assert mapped70['p'].map_time(what, reps=1) > 0.0          # a figure for the record; no time is asserted


# ---- the engine's location rows ----------------------------------------------------------------------------------------------------
MT = 'cnn_L3_melspec2'
SHAPE = {0: (28, 28, 512), 1: (32, 24, 512)}


def _params(mt, seed):
    P = o.init_params(mt, seed=seed)
    rng = np.random.RandomState(seed)
    P['dense_1/bias'] = (0.1 * rng.randn(*P['dense_1/bias'].shape)).astype(np.float32)
    P['dense_2/bias'] = rng.randn(2).astype(np.float32)
    return P


def _last_bn(e, tower):
    prefix = ('vision_model', 'audio_model')[tower]
    return [n for n, _, _ in e.param_table() if n.startswith(prefix + '/batch_normalization') and n.endswith('/gamma')][-1][:-len('/gamma')]


@pytest.fixture(scope='module')
def melspec2(gpu_required):
    """cnn_L3_melspec2 at engine batch 2 and 3 items: the last engine batch holds one real row"""
    m = model.L3Model(MT)
    m._assign(_params(MT, 21))
    e = m._ensure_engine(2)
    v, a, _ = o.synthetic_batch(3, seed=31)
    yield dict(m=m, e=e, x=(v[:3], a[:3]))
    m._drop_engines()


@pytest.mark.parametrize('tower', [0, 1])
def test_location_rows_against_features_and_activation(melspec2, tower):
    e, x = melspec2['e'], melspec2['x'][tower]
    H, W, C = e.tower_locations_shape(tower)
    assert (H, W, C) == SHAPE[tower] and C == e.tower_dim(tower)
    L = H * W
    loc = e.tower_locations(tower, x)
    act = e.activation(_last_bn(e, tower))          # the engine's current batch: item 2 and a row of zeros' worth of input
    rows = loc.download()
    loc.close()
    assert rows.shape == (3 * L, C)
    assert np.array_equal(bits(rows[2 * L:]), bits(act.reshape(2, L, C)[0]))
    feats = e.tower_features(tower, x)
    assert np.array_equal(bits(rows.reshape(3, L, C).max(axis=1)), bits(feats))
    # item 0 alone: the same bits; into the middle of a larger matrix: only its rows are written
    dst = _lib.Features.alloc(3 * L, C)
    e.tower_locations(tower, x[:1], dst=dst, row0=1)
    got = dst.download()
    dst.close()
    assert np.array_equal(bits(got[L:2 * L]), bits(rows[:L])) and not got[:L].any() and not got[2 * L:].any()
    small = _lib.Features.alloc(3 * L - 1, C)
    narrow = _lib.Features.alloc(3 * L, C - 1)
    for bad, why in ((small, 'rows'), (narrow, 'columns')):
        with pytest.raises(_lib.L3Error, match=why):
            e.tower_locations(tower, x, dst=bad)
    small.close(), narrow.close()


def test_location_rows_bf16_engine(gpu_required):
    e = _lib.Engine(MT, 2, dtype='bf16')
    e.set_params(_params(MT, 21))
    v = o.synthetic_batch(3, seed=31)[0][:3]
    H, W, C = e.tower_locations_shape(0)
    loc = e.tower_locations(0, v)
    rows = loc.download()
    loc.close()
    act = e.activation(_last_bn(e, 0))
    assert np.array_equal(bits(rows[2 * H * W:]), bits(act.reshape(2, H * W, C)[0]))
    assert np.array_equal(bits(rows.reshape(3, H * W, C).max(axis=1)), bits(e.tower_features(0, v)))
    e.close()


def _bank():
    rs = np.random.RandomState(4)
    clips = [(rs.randint(0, 256, (8, 240, 320, 3)).astype(np.uint8), rs.randint(-32768, 32768, (2 * 48000 + 7, 2)).astype(np.int16)),
             (rs.randint(0, 256, (3, 243, 317, 3)).astype(np.uint8), rs.randint(-32768, 32768, (int(0.6 * 48000),)).astype(np.int16))]
    bank = avsample.ClipBank(0, sum(f.size for f, _ in clips), sum(len(x) + 8 for _, x in clips), resize=256)
    for f, x in clips:
        bank.add(f, x, 48000)
    return bank


def test_sampled_form_equals_the_rows_form(melspec2):
    e = melspec2['e']
    bank = _bank()
    rec, _ = crossmodal.retrieval_records(bank.clips, fps=4)
    assert len(rec) == 3
    batch = avsample.sample_batch(bank, rec)
    rows = (o.preprocess_video(batch['video']), o.pcm2float(batch['audio'], np.float32))
    for tower in (0, 1):
        H, W, C = SHAPE[tower]
        want = e.tower_locations(tower, rows[tower])
        loc, pooled = _lib.Features.alloc(4 * H * W, C), _lib.Features.alloc(4, C)
        e.tower_locations_sampled(bank, rec, tower, loc, pooled=pooled, row0=1)
        got, w = loc.download(), want.download()
        assert np.array_equal(bits(got[H * W:]), bits(w)) and not got[:H * W].any()
        assert np.array_equal(bits(pooled.download()[1:]), bits(w.reshape(3, H * W, C).max(axis=1)))
        want.close(), loc.close(), pooled.close()
    bad = rec.copy()
    bad['audio_start'][2] = 1
    loc = _lib.Features.alloc(3 * 28 * 28, 512)
    with pytest.raises(_lib.L3Error, match='sample 2'):
        e.tower_locations_sampled(bank, bad, 0, loc)
    loc.close(), bank.close()


def test_scorer_maps_equal_the_pair_list_over_location_rows(melspec2):
    m, (v, a) = melspec2['m'], melspec2['x']
    L = 28 * 28
    (loc, hw), _ = m.predict_locations(video=v)
    assert hw == (28, 28) and loc.shape == (3 * L, 512)
    A = m.predict_towers(audio=a)[1]
    sc = crossmodal.PairScorer(m).set_items(A=A)
    iv, ia = np.array([2, 0, 2, 1, 0]), np.array([0, 1, 2, 2, 1])          # repeated frames, out of order
    sc.set_maps(0, v, chunk_items=1)
    one, peak, arg = sc.maps(iv, ia, peaks=True)
    S1 = sc.peaks()
    sc.set_maps(0, v, chunk_items=64)
    many = sc.maps(iv, ia)
    S64 = sc.peaks(block_bytes=1)
    sc.set_maps(0, (loc, hw), chunk_items=2)
    assert one.shape == (5, 28, 28) and np.array_equal(bits(one), bits(many)) and np.array_equal(bits(sc.maps(iv, ia)), bits(one))
    assert np.array_equal(bits(S1[0]), bits(S64[0])) and np.array_equal(S1[1], S64[1])          # every pair: chunking leaves M as it is
    _order = R.peaks_ref(one.reshape(5, L))
    assert np.array_equal(bits(peak), bits(_order[0])) and np.array_equal(arg, _order[1])
    assert np.array_equal(bits(peak), bits(S1[0][iv, ia])) and np.array_equal(bits(sc.pair_peaks(iv, ia)[0]), bits(peak))
    rv, ra = sc.peak_ranks()
    wv, wa = R.peak_ranks_ref(S1[0], np.arange(3), np.arange(3))
    assert np.array_equal(rv, wv) and np.array_equal(ra, wa)
    sc.handle.set_vision(loc.handle)          # the 3 x 784 location rows as items
    rows = (iv[:, None] * L + np.arange(L)[None, :]).reshape(-1)
    want = sc.handle.list(rows, np.repeat(ia, L)).reshape(5, 28, 28)
    assert np.array_equal(bits(one), bits(want))
    # the pooled pair score is the head at the per-channel maximum, not the maximum of the head: the read-out is another quantity
    assert crossmodal.upsample_map(one[0], (224, 224)).shape == (224, 224)
    sc.close(), loc.close()


def test_a_model_without_a_global_pool_is_refused(gpu_required):
    e = _lib.Engine('tiny_L3', 2)
    for tower in (0, 1):
        with pytest.raises(ValueError, match='no per-location form'):
            e.tower_locations_shape(tower)
        with pytest.raises(ValueError, match='no per-location form'):
            e.tower_locations(tower, np.zeros((1, 224, 224, 3) if tower == 0 else (1, 1, 48000), np.float32))
    import ctypes as C
    dst = _lib.Features.alloc(4, 360)
    assert e.lib.l3_tower_locations_dev(e.h, 0, _lib._ptr(np.zeros(224 * 224 * 3, np.float32)), 1, dst.h, 0) == -1
    assert e.lib.l3_tower_locations_shape(e.h, 2, None, None, C.byref(C.c_int())) == -1
    dst.close(), e.close()


def test_cli_maps_path_reranks_consistently_with_peak_ranks(gpu_required, tmp_path):
    """--maps-path: the saved maps' peaks are the saved peaks, and ranking the bank by best-location scores computed from the scorer
    gives the saved peak ranks; the default outputs are those of a run without the option"""
    from l3embedding_amd import cli_retrieval
    m = model.L3Model(MT)
    m._assign(_params(MT, 5))
    weights = str(tmp_path / 'w.h5')
    m.save_weights(weights)
    rs = np.random.RandomState(4)
    paths = []
    for i, (nf, ns) in enumerate(((8, 2 * 48000 + 7), (4, 48000))):
        paths.append(str(tmp_path / ('clip%d.npz' % i)))
        np.savez(paths[-1], frames=rs.randint(0, 256, (nf, 240, 320, 3)).astype(np.uint8), audio=rs.randint(-32768, 32768, ns).astype(np.int16), rate=48000)
    base = [weights, MT] + paths + ['--fps', '4', '--recall-at', '1', '2', '--batch-size', '2', '--top-k', '2']
    plain = cli_retrieval.main(base)
    mp = str(tmp_path / 'maps.npz')
    got = cli_retrieval.main(base + ['--maps-path', mp, '--maps-top', '1'])
    peak_metrics = got.pop('peak')
    assert got == plain          # everything else is as it was
    z = np.load(mp)
    n = 3
    assert z['truth_map'].shape == (n, 28, 28) and z['top_map'].shape == (n, 1, 28, 28) and z['item_clip'].tolist() == [0, 0, 1]
    pk, ar = R.peaks_ref(z['truth_map'].reshape(n, -1))
    assert np.array_equal(bits(pk), bits(z['truth_peak'])) and np.array_equal(ar, z['truth_arg'])
    have = z['top_arg'][:, 0] >= 0
    pk, ar = R.peaks_ref(z['top_map'][have, 0].reshape(int(have.sum()), -1))
    assert np.array_equal(bits(pk), bits(z['top_peak'][have, 0])) and np.array_equal(ar, z['top_arg'][have, 0])
    # re-rank from the scorer's own S: the truth peaks on its diagonal, the saved ranks from the count over it
    bank = avsample.load_clips(avsample.ClipBank(0, 12 * 240 * 320 * 3, 3 * 48000 + 64, 256), paths)
    rec, groups = crossmodal.retrieval_records(bank.clips, fps=4)
    e = m._ensure_engine(2)
    A = _lib.Features.alloc(n, 512)
    e.tower_features_sampled(bank, rec, aud=A)
    sc = crossmodal.PairScorer(m).set_items(A=A)
    sc.set_maps(0, (bank, rec))
    S, _ = sc.peaks()
    assert np.array_equal(bits(np.diagonal(S)), bits(z['truth_peak']))
    wv, wa = R.peak_ranks_ref(S, np.arange(n), np.arange(n), groups, groups)
    assert np.array_equal(z['peak_rank_v2a'], wv) and np.array_equal(z['peak_rank_a2v'], wa)
    assert peak_metrics['frame_to_audio'] == crossmodal.retrieval_metrics(wv, (1, 2))
    assert peak_metrics['audio_to_frame'] == crossmodal.retrieval_metrics(wa, (1, 2))
    sc.close(), A.close(), bank.close()
    m._drop_engines()
