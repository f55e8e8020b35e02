"""GPU tests of the top-k lists (pair_topk_kernel and topk_merge_kernel of csrc/pairs.hip, l3_pairs_topk, l3_op_pair_topk,
crossmodal.PairScorer.topk, evaluate_bank(topk=), cli_retrieval --top-k).  The reference of every case is tests/pairs_topk_ref.py on
the matrix that Pairs.matrix() or op_pair_margins returns: the indices must be equal, the margins equal as bits."""
import json

import numpy as np
import pytest

from l3embedding_amd import _lib, avsample, crossmodal, model
from oracle import l3_oracle as o

from pairs_topk_ref import same_lists, topk_ref

pytestmark = pytest.mark.gpu

KS = (1, 5, 64)


def _head(rng, nv, na, H):
    return ((rng.randn(nv + na, H) / np.sqrt(nv + na)).astype(np.float32), rng.randn(H).astype(np.float32),
            rng.randn(H, 2).astype(np.float32), rng.randn(2).astype(np.float32))


@pytest.fixture(scope='module')
def scorer130(gpu_required):
    """The fixture of tests/test_pairs_gpu.py: 130 frames and 130 seconds of tiny_L3's widths (three tiles a side, a ragged edge of 2)
    in clip groups of sizes 1 .. 7; the seconds of the second half are bit copies of the first half's, so every margin has a tie."""
    rng = np.random.RandomState(130)
    nv, na, H, n = 360, 350, 64, 130
    head = _head(rng, nv, na, H)
    V, A = rng.randn(n, nv).astype(np.float32), rng.randn(n, na).astype(np.float32)
    A[65:] = A[:65]
    groups, g = [], 0
    while len(groups) < n:
        groups += [g] * (g % 7 + 1)
        g += 1
    groups = np.array(groups[:n], np.int32)
    p = _lib.Pairs(nv, na, H)
    p.set_head(*head)
    p.set_vision(V)
    p.set_audio(A)
    perm = np.random.RandomState(7).permutation(n).astype(np.int32)
    yield dict(p=p, groups=groups, n=n, M=p.matrix(), perm=perm, inv=np.argsort(perm).astype(np.int32))
    p.close()


def _index_broke_a_tie(lists):
    idx, margin = lists
    return bool(np.any((margin[:, :-1] == margin[:, 1:]) & (idx[:, :-1] < idx[:, 1:]) & (idx[:, :-1] >= 0)))


@pytest.mark.parametrize('k', KS)
def test_handle_lists_equal_the_reference(scorer130, k):
    s = scorer130
    p, M, g, n = s['p'], s['M'], s['groups'], s['n']
    assert np.array_equal(M[:, 65:].view(np.uint32), M[:, :65].view(np.uint32))          # the twins tie bit for bit
    diag = np.arange(n, dtype=np.int32)
    ties = False
    for ta, tv, groups in ((None, None, None), (None, None, g), (diag, diag, g), (s['perm'], s['inv'], g)):
        v2a, a2v = p.topk(k, ta, tv, groups, groups)
        assert same_lists(v2a, topk_ref(M, k, ta, groups, groups)), (k, ta is None, groups is None)
        assert same_lists(a2v, topk_ref(M.T, k, tv, groups, groups)), (k, tv is None, groups is None)
        ties = ties or _index_broke_a_tie(v2a)
        if groups is not None:          # no listed item is of the query's own clip, but for the kept truth
            own = (g[np.maximum(v2a[0], 0)] == g[:, None]) & (v2a[0] >= 0)
            assert not own.any() if ta is None else np.all(v2a[0][own] == np.broadcast_to(ta[:, None], own.shape)[own])
    assert ties or k == 1          # a list of one entry has no neighbours; the twin columns tie in every longer one
    # one direction only: the other comes back as None, and what is computed does not change
    v2a, a2v = p.topk(k, None, s['inv'], g, g, directions=('a2v',))
    assert v2a is None and same_lists(a2v, topk_ref(M.T, k, s['inv'], g, g))
    v2a, a2v = p.topk(k, s['perm'], None, g, g, directions='v2a')
    assert a2v is None and same_lists(v2a, topk_ref(M, k, s['perm'], g, g))


def test_the_index_breaks_ties_in_some_list(scorer130):
    """without this the cases above would show nothing about the order: at k = 5 and 64 the twin seconds stand next to each other"""
    p = scorer130['p']
    for k in (5, 64):
        v2a, _ = p.topk(k)
        assert _index_broke_a_tie(v2a)
    v2a, _ = p.topk(1)          # and at k = 1 the smaller twin is the one listed
    assert np.all(v2a[0][:, 0] < 65)


@pytest.mark.parametrize('k', KS)
def test_lists_agree_with_the_rank_counts(scorer130, k):
    s = scorer130
    p, g, n = s['p'], s['groups'], s['n']
    ta, tv = s['perm'], s['inv']
    rv, ra = p.ranks(ta, tv, g, g)
    v2a, a2v = p.topk(k, ta, tv, g, g)
    seen = 0
    for (idx, margin), truth, rank in ((v2a, ta, rv), (a2v, tv, ra)):
        for i in range(n):
            at = np.flatnonzero(idx[i] == truth[i])
            if rank[i] >= k:
                assert len(at) == 0, (i, rank[i])
            if len(at):
                seen += 1
                assert len(at) == 1 and int(np.sum(margin[i] > margin[i, at[0]])) == rank[i], (i, rank[i])
    assert seen > 0


@pytest.mark.parametrize('H', [64, 128])
def test_op_topk_with_forced_segments(gpu_required, H):
    """200 queries against 1500 candidates at k = 10: 24 tiles, most of which insert nothing, so the threshold path is exercised;
    segments 1, 2, 3 and the library's choice all give the reference, and so each other; then with the roles exchanged"""
    rng = np.random.RandomState(H)
    nv, na, k = 200, 1500, 10
    u, t = rng.randn(nv, H).astype(np.float32), rng.randn(na, H).astype(np.float32)
    wd, bd = rng.randn(H).astype(np.float32), np.float32(0.21)
    gv, ga = rng.randint(0, 40, nv).astype(np.int32), rng.randint(0, 40, na).astype(np.int32)
    ta, tv = rng.randint(0, na, nv).astype(np.int32), rng.randint(0, nv, na).astype(np.int32)
    M = _lib.op_pair_margins(u, t, wd, bd)
    want = {(False, False): topk_ref(M, k), (False, True): topk_ref(M, k, ta, gv, ga),
            (True, False): topk_ref(M.T, k), (True, True): topk_ref(M.T, k, tv, ga, gv)}
    for swapped in (False, True):
        q, c = (t, u) if swapped else (u, t)
        for segments in (1, 2, 3, 0):
            assert same_lists(_lib.op_pair_topk(q, c, wd, bd, k, segments=segments), want[swapped, False]), (swapped, segments)
            tr, gq, gc = (tv, ga, gv) if swapped else (ta, gv, ga)
            assert same_lists(_lib.op_pair_topk(q, c, wd, bd, k, tr, gq, gc, segments), want[swapped, True]), (swapped, segments)


def test_edges(gpu_required):
    rng = np.random.RandomState(5)
    H = 64
    wd, bd = rng.randn(H).astype(np.float32), np.float32(-0.4)

    def case(nq, nc, k, truth=None, gq=None, gc=None, segments=0):
        u, t = rng.randn(nq, H).astype(np.float32), rng.randn(nc, H).astype(np.float32)
        got = _lib.op_pair_topk(u, t, wd, bd, k, truth, gq, gc, segments)
        assert same_lists(got, topk_ref(_lib.op_pair_margins(u, t, wd, bd), k, truth, gq, gc)), (nq, nc, k, segments)
        return got

    case(1, 130, 5)
    case(1, 1, 1)
    idx, margin = case(3, 5, 8)          # fewer candidates than k: filler
    assert np.all(idx[:, 5:] == -1) and np.all(margin[:, 5:] == -np.inf) and np.all(idx[:, :5] >= 0)
    for nc in (64, 65):
        for segments in (0, 2):
            case(70, nc, 64, segments=segments)
            case(nc, 70, 3, segments=segments)
    # query 0 is of the clip of every candidate: all filler, or its truth alone
    gq, gc = np.array([7, 1, 2], np.int32), np.full(70, 7, np.int32)
    idx, margin = case(3, 70, 4, None, gq, gc)
    assert np.all(idx[0] == -1) and np.all(margin[0] == -np.inf) and np.all(idx[1:] >= 0)
    idx, margin = case(3, 70, 4, np.array([69, 0, 1], np.int32), gq, gc, segments=2)
    assert idx[0].tolist() == [69, -1, -1, -1] and np.isfinite(margin[0, 0]) and np.all(margin[0, 1:] == -np.inf)


def test_nan_is_never_listed(gpu_required):
    rng = np.random.RandomState(9)
    H, nq, nc, k, row = 64, 70, 130, 6, 66
    u, t = rng.randn(nq, H).astype(np.float32), rng.randn(nc, H).astype(np.float32)
    wd, bd = rng.randn(H).astype(np.float32), np.float32(0.1)
    wd[11] = 0.0
    u[row, 11] = np.inf          # relu(inf + t) * 0 = NaN in every pair of the row
    M = _lib.op_pair_margins(u, t, wd, bd)
    assert np.all(np.isnan(M[row])) and not np.isnan(np.delete(M, row, axis=0)).any()
    idx, margin = _lib.op_pair_topk(u, t, wd, bd, k)
    assert same_lists((idx, margin), topk_ref(M, k))
    assert np.all(idx[row] == -1) and np.all(margin[row] == -np.inf)
    for kk, segments in ((k, 0), (64, 0), (64, 2), (64, 1)):          # the other direction: the row is in no list, however long
        idx, margin = _lib.op_pair_topk(t, u, wd, bd, kk, segments=segments)
        assert same_lists((idx, margin), topk_ref(M.T, kk))
        assert not np.any(idx == row) and not np.isnan(margin).any()


def test_run_to_run(scorer130):
    s = scorer130
    p, g = s['p'], s['groups']
    a, b = p.topk(64, s['perm'], s['inv'], g, g), p.topk(64, s['perm'], s['inv'], g, g)
    assert same_lists(a[0], b[0]) and same_lists(a[1], b[1])


def test_library_refuses_bad_arguments(scorer130):
    """the C ABI's own checks (the wrappers' are tested without a GPU): L3_EINVAL and a message, and the handle is as it was"""
    p, n = scorer130['p'], scorer130['n']
    lib, h, ptr = p.lib, p.h, _lib._ptr
    iv, mv = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.float32)
    ia, ma = np.zeros((n, 3), np.int32), np.zeros((n, 3), np.float32)
    big_i, big_m = np.zeros((n, 65), np.int32), np.zeros((n, 65), np.float32)
    ok = np.zeros(n, np.int32)
    badt = ok.copy()
    badt[3] = n
    neg = ok.copy()
    neg[n - 1] = -1
    calls = [lambda: lib.l3_pairs_topk(h, 0, None, None, None, None, ptr(iv), ptr(mv), None, None),
             lambda: lib.l3_pairs_topk(h, 65, None, None, None, None, ptr(big_i), ptr(big_m), None, None),
             lambda: lib.l3_pairs_topk(h, 3, None, None, None, None, ptr(iv), None, None, None),
             lambda: lib.l3_pairs_topk(h, 3, None, None, None, None, ptr(iv), ptr(mv), None, ptr(ma)),
             lambda: lib.l3_pairs_topk(h, 3, None, None, None, None, None, None, None, None),
             lambda: lib.l3_pairs_topk(h, 3, ptr(ok), None, None, None, ptr(iv), ptr(mv), None, None),
             lambda: lib.l3_pairs_topk(h, 3, None, ptr(ok), None, None, ptr(iv), ptr(mv), ptr(ia), ptr(ma)),
             lambda: lib.l3_pairs_topk(h, 3, None, None, ptr(ok), None, ptr(iv), ptr(mv), None, None),
             lambda: lib.l3_pairs_topk(h, 3, ptr(badt), None, ptr(ok), ptr(ok), ptr(iv), ptr(mv), None, None),
             lambda: lib.l3_pairs_topk(h, 3, ptr(ok), ptr(neg), ptr(ok), ptr(ok), ptr(iv), ptr(mv), ptr(ia), ptr(ma)),
             lambda: lib.l3_pairs_topk(None, 3, None, None, None, None, ptr(iv), ptr(mv), None, None)]
    for k, call in enumerate(calls):
        assert call() == -1, k          # L3_EINVAL
        assert lib.l3_last_error(None), k
    assert not iv.any() and not mv.any() and not ia.any() and not ma.any()          # nothing was written
    u, wd = np.zeros((4, 64), np.float32), np.zeros(64, np.float32)
    o4i, o4m = np.zeros((4, 2), np.int32), np.zeros((4, 2), np.float32)
    ops = [lambda: lib.l3_op_pair_topk(0, ptr(u), ptr(u), ptr(wd), 0.0, 4, 4, 64, 0, None, None, None, 0, ptr(o4i), ptr(o4m)),
           lambda: lib.l3_op_pair_topk(0, ptr(u), ptr(u), ptr(wd), 0.0, 4, 4, 64, 2, None, None, None, -1, ptr(o4i), ptr(o4m)),
           lambda: lib.l3_op_pair_topk(0, ptr(u), ptr(u), ptr(wd), 0.0, 4, 4, 64, 2, None, None, None, 0, None, ptr(o4m)),
           lambda: lib.l3_op_pair_topk(0, ptr(u), ptr(u), ptr(wd), 0.0, 4, 4, 48, 2, None, None, None, 0, ptr(o4i), ptr(o4m)),
           lambda: lib.l3_op_pair_topk(0, ptr(u), ptr(u), ptr(wd), 0.0, 4, 4, 64, 2, ptr(ok), None, None, 0, ptr(o4i), ptr(o4m)),
           lambda: lib.l3_op_pair_topk(0, ptr(u), ptr(u), ptr(wd), 0.0, 4, 4, 64, 2, ptr(badt), ptr(ok), ptr(ok), 0, ptr(o4i), ptr(o4m))]
    for k, call in enumerate(ops):
        assert call() == -1, k
        assert lib.l3_last_error(None), k
    assert np.array_equal(p.matrix().view(np.uint32), scorer130['M'].view(np.uint32))          # the handle gives what it gave
    assert same_lists(p.topk(3)[0], topk_ref(scorer130['M'], 3))


# ---- from a clip bank, and the command line ------------------------------------------------------------------------------------
def _model(mt, seed):
    P = o.init_params(mt, seed=seed)
    rng = np.random.RandomState(seed)
    P['dense_1/bias'] = (0.1 * rng.randn(*P['dense_1/bias'].shape)).astype(np.float32)
    P['dense_2/bias'] = rng.randn(2).astype(np.float32)
    m = model.L3Model(mt)
    m._assign(P)
    return m


def _two_clips():
    """the bank of tests/test_pairs_gpu.py::test_bank_path: 2 s and 0.6 s at 4 frames per second, about 240 x 320"""
    rs = np.random.RandomState(4)
    return [(rs.randint(0, 256, (8, 240, 320, 3)).astype(np.uint8), rs.randint(-32768, 32768, (2 * 48000 + 7, 2)).astype(np.int16)),
            (rs.randint(0, 256, (3, 243, 317, 3)).astype(np.uint8), rs.randint(-32768, 32768, (int(0.6 * 48000),)).astype(np.int16))]


def test_evaluate_bank_lists(gpu_required):
    fps, clips = 4, _two_clips()
    bank = avsample.ClipBank(0, sum(f.size for f, _ in clips), sum(len(x) + 8 for _, x in clips), resize=256)
    for f, x in clips:
        bank.add(f, x, 48000)
    m = _model('tiny_L3', 5)
    e = m._ensure_engine(2)
    plain = crossmodal.evaluate_bank(m, bank, fps=fps, ks=(1, 2))
    out = crossmodal.evaluate_bank(m, bank, fps=fps, ks=(1, 2), topk=3)
    assert sorted(out) == sorted(list(plain) + ['lists']) and {k: out[k] for k in plain} == plain          # the metrics are unchanged
    rec, groups = crossmodal.retrieval_records(bank.clips, fps=fps)
    assert groups.tolist() == [0, 0, 1]
    V, A = _lib.Features.alloc(3, 360), _lib.Features.alloc(3, 350)
    e.tower_features_sampled(bank, rec, vis=V, aud=A)
    sc = crossmodal.PairScorer(m).set_items(V, A)
    M, diag = sc.margins(), np.arange(3)
    for name, mat in (('frame_to_audio', M), ('audio_to_frame', M.T)):
        got = out['lists'][name]
        want = topk_ref(mat, 3, diag, groups, groups)
        assert same_lists((got['index'], got['margin']), want), name
        assert np.array_equal(got['clip'], np.where(want[0] >= 0, groups[np.maximum(want[0], 0)], -1)) and got['clip'].dtype == np.int32
    # items 0 and 1 are of one clip: each keeps its own second and sees item 2's; one filler closes the list
    assert np.all(out['lists']['frame_to_audio']['index'][:2, 2] == -1) and np.all(out['lists']['frame_to_audio']['index'][2] >= 0)
    assert sorted(out['lists']['frame_to_audio']['index'][0, :2].tolist()) == [0, 2]
    # the hardest negatives of the same scorer: every cross-clip pair of this bank, once each
    iv, ia, mg = crossmodal.hard_negatives(sc, groups, 2)
    assert sorted(zip(iv.tolist(), ia.tolist())) == [(0, 2), (1, 2), (2, 0), (2, 1)]
    assert np.array_equal(mg.view(np.uint32), M[iv, ia].view(np.uint32))
    neg = crossmodal.negative_records(rec, iv, ia)
    assert np.all(neg['label'] == 1) and np.all(neg['video_clip'] != neg['audio_clip'])
    sc.close(), V.close(), A.close(), bank.close()
    m._drop_engines()


def test_cli_retrieval_top_k(gpu_required, tmp_path, capsys):
    from l3embedding_amd import cli_retrieval
    m = _model('tiny_L3', 5)
    weights = str(tmp_path / 'w.h5')
    m.save_weights(weights)
    m._drop_engines()
    paths = []
    for i, (f, x) in enumerate(_two_clips()):
        paths.append(str(tmp_path / ('clip%d.npz' % i)))
        np.savez(paths[-1], frames=f, audio=x, rate=48000)
    common = [weights, 'tiny_L3'] + paths + ['--fps', '4', '--recall-at', '1', '2', '--batch-size', '2']
    plain = cli_retrieval.main(common)
    printed = json.loads(capsys.readouterr().out)
    assert sorted(printed) == ['audio_to_frame', 'avc_accuracy', 'clips', 'frame_to_audio', 'items'] and printed == plain
    lists_path = str(tmp_path / 'lists.npz')
    got = cli_retrieval.main(common + ['--top-k', '3', '--lists-path', lists_path])
    printed = json.loads(capsys.readouterr().out)
    assert printed == got and {k: got[k] for k in plain} == plain
    with np.load(lists_path) as z:
        assert sorted(z.files) == sorted(['item_clip'] + ['%s_%s' % (d, f) for d in ('frame_to_audio', 'audio_to_frame')
                                                           for f in ('index', 'clip', 'margin')])
        assert z['item_clip'].tolist() == [0, 0, 1]
        for d in ('frame_to_audio', 'audio_to_frame'):
            assert z[d + '_index'].shape == z[d + '_margin'].shape == z[d + '_clip'].shape == (3, 3)
            assert z[d + '_index'].tolist() == got['lists'][d]['index'] and z[d + '_clip'].tolist() == got['lists'][d]['clip']
            margins = [[None if np.isinf(v) else float(v) for v in row] for row in z[d + '_margin']]
            assert margins == got['lists'][d]['margin']
