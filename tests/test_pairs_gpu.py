"""GPU tests of cross-modal retrieval (csrc/pairs.hip, the tower-feature entry points of csrc/engine.hip,
l3embedding_amd/crossmodal.py): the pair kernel and the projection alone against float64 with the bounds tests/pairs_ref.py
derives, the position independence the rank mode rests on, the ranks against a NumPy count, the whole path against the oracle's
head, and the two new routes to a tower's output against the ones the project had."""
import numpy as np
import pytest

from l3embedding_amd import _lib, avsample, crossmodal, model
from oracle import l3_oracle as o

import pairs_ref as R

pytestmark = pytest.mark.gpu

TILE = R.TILE          # 64 frames x 64 seconds per workgroup (L3_PAIRS_TILE); a lane holds 4 x 4 of them
CROSS_BATCH_BOUND = 5e-6          # of tests/test_embedding_parity_gpu.py: two routes may plan a tower differently
LOGIT_BAR = 1e-3                  # the project's parity bar on logits


def test_tile_constant_is_the_library_s():
    assert TILE == _lib.PAIRS_TILE == 64


# ---- the pair kernel alone ---------------------------------------------------------------------------------------------------
PAIR_SHAPES = [(nv, na) for nv in (TILE - 1, TILE, TILE + 1) for na in (TILE - 1, TILE, TILE + 1)] + [(1, 1), (1, TILE + 1)]


@pytest.mark.parametrize('H', [64, 128])
def test_pair_kernel_against_float64(gpu_required, H):
    rng = np.random.RandomState(H)
    wd, bd = rng.randn(H).astype(np.float32), np.float32(-0.37)
    worst = 0.0
    for nv, na in PAIR_SHAPES:
        u, t = rng.randn(nv, H).astype(np.float32), rng.randn(na, H).astype(np.float32)
        got = _lib.op_pair_margins(u, t, wd, bd)
        ref, bound = R.margins_ref(u, t, wd, bd), R.margins_bound(u, t, wd, bd)
        err = np.abs(got - ref)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (nv, na, float((err / bound).max()))
    print('pair kernel H=%d: worst error / bound %.3f' % (H, worst))
    nv, na = TILE + 1, TILE + 1
    # every unit inactive: the margin is bd, exactly
    u, t = -np.abs(rng.randn(nv, H)).astype(np.float32) - 1, -np.abs(rng.randn(na, H)).astype(np.float32)
    assert np.all(_lib.op_pair_margins(u, t, wd, bd) == bd)
    # u = -t for every pair: h is exactly 0
    r = rng.randn(H).astype(np.float32)
    assert np.all(_lib.op_pair_margins(np.tile(r, (nv, 1)), np.tile(-r, (na, 1)), wd, bd) == bd)


# ---- the projection ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,H', [(512, 128), (360, 64), (350, 64)])
def test_projection_against_float64_and_position_independence(gpu_required, K, H):
    rng = np.random.RandomState(K)
    w, b = (rng.randn(K, H) / np.sqrt(K)).astype(np.float32), rng.randn(H).astype(np.float32)
    x = rng.randn(257, K).astype(np.float32)
    full = None
    for rows in (1, 63, 257):
        for bias in (None, b):
            got = _lib.op_project(x[:rows], w, bias)
            err, bound = np.abs(got - R.project_ref(x[:rows], w, bias)), R.project_bound(x[:rows], w, bias)
            assert np.all(err <= bound), (rows, bias is not None, float((err / bound).max()))
            if rows == 257 and bias is not None:
                full = got
    alone = _lib.op_project(x[5:9], w, b)
    assert np.array_equal(alone.view(np.uint32), full[5:9].view(np.uint32))
    assert np.array_equal(_lib.op_project(x[256:], w, b).view(np.uint32), full[256:].view(np.uint32))


# ---- one scorer for the handle's tests ---------------------------------------------------------------------------------------
def _head(rng, nv, na, H):
    return ((rng.randn(nv + na, H) / np.sqrt(nv + na)).astype(np.float32), rng.randn(H).astype(np.float32),
            rng.randn(H, 2).astype(np.float32), rng.randn(2).astype(np.float32))


@pytest.fixture(scope='module')
def scorer130(gpu_required):
    """130 frames and 130 seconds of tiny_L3's widths in clip groups of sizes 1 .. 7; the seconds of the second half are bit-for-bit
    copies of the first half's (so every truth column has a twin in another clip, and ties exist)."""
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
    yield dict(p=p, V=V, A=A, head=head, groups=groups, n=n, M=p.matrix())
    p.close()


def test_handle_margins_and_probabilities_against_float64(scorer130):
    s = scorer130
    w1, b1, w2, b2 = s['head']
    U, T = _lib.op_project(s['V'], w1[:360]), _lib.op_project(s['A'], w1[360:], b1)          # the handle's kernel: the same bits
    wd64, bd64 = R.head_diff(w2, b2)
    ref, bound = R.margins_ref(U, T, wd64, bd64), R.margins_bound(U, T, wd64, bd64, head_rounded=True)
    assert np.all(np.abs(s['M'] - ref) <= bound)
    P = s['p'].matrix(prob=True)
    assert np.all(np.abs(P - R.sigmoid_ref(ref)) <= R.probability_bound(ref, bound))
    assert P.min() >= 0.0 and P.max() <= 1.0


def test_pairs_are_position_independent(gpu_required):
    """a 65 x 130 matrix, its block [3, 40) x [60, 130) and a shuffled list of all its pairs: bit-equal element by element"""
    rng = np.random.RandomState(65)
    nv, na, H = 512, 512, 128
    p = _lib.Pairs(nv, na, H)
    p.set_head(*_head(rng, nv, na, H))
    V, A = rng.randn(65, nv).astype(np.float32), rng.randn(130, na).astype(np.float32)
    p.set_vision(V)
    fa = _lib.Features(A)          # the seconds from a device matrix, the frames from host rows
    p.set_audio(fa)
    M = p.matrix()
    assert M.shape == (65, 130)
    assert np.array_equal(p.matrix(3, 40, 60, 130).view(np.uint32), M[3:40, 60:130].view(np.uint32))
    assert np.array_equal(p.matrix(64, 65, 129, 130).view(np.uint32), M[64:, 129:].view(np.uint32))
    iv, ia = np.divmod(rng.permutation(65 * 130), 130)
    assert np.array_equal(p.list(iv, ia).view(np.uint32), M[iv, ia].view(np.uint32))
    # a frame projected alone, and as row 0 of another set, scores the same bits
    p.set_vision(V[17:18])
    assert np.array_equal(p.matrix().view(np.uint32), M[17:18].view(np.uint32))
    p.close()
    fa.close()


def test_ranks_equal_the_numpy_count(scorer130):
    s = scorer130
    p, M, g, n = s['p'], s['M'], s['groups'], s['n']
    assert np.array_equal(M[:, 65:].view(np.uint32), M[:, :65].view(np.uint32))          # the twins tie bit for bit
    diag = np.arange(n)
    perm = np.random.RandomState(7).permutation(n)
    inv = np.argsort(perm)
    many_to_one = np.random.RandomState(8).randint(0, n, n)          # not a permutation: several frames share a second
    cases = [(diag, diag, None), (diag, diag, g), (perm, inv, g), (many_to_one, many_to_one[::-1].copy(), None), (perm, None, g),
             (None, inv, None)]
    some_ties = False
    for ta, tv, groups in cases:
        rv, ra = p.ranks(ta, tv, groups, groups)
        wv, wa = R.ranks_ref(M, ta, tv, groups, groups)
        for got, want in ((rv, wv), (ra, wa)):
            assert (got is None) == (want is None)
            if want is not None:
                assert got.dtype == np.int32 and np.array_equal(got, want)
        if ta is not None and groups is None:
            s_true = M[np.arange(n), ta]
            some_ties = some_ties or bool(np.any((M == s_true[:, None]).sum(axis=1) > 1))
    assert some_ties          # the strict comparison was exercised: a tie with the truth is not counted
    # run to run: the same counts
    a, b = p.ranks(perm, inv, g, g), p.ranks(perm, inv, g, g)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_library_refuses_bad_arguments(scorer130):
    """the C ABI's own checks (the Python wrapper's are tested without a GPU): L3_EINVAL and a message, nothing else happens"""
    import ctypes as C
    p = scorer130['p']
    lib, h = p.lib, p.h
    out = np.zeros(16, np.float32)
    idx = np.array([0, 130], np.int32)
    ok = np.zeros(130, np.int32)
    badt = ok.copy()
    badt[3] = 130
    r = np.zeros(130, np.int32)
    ptr = _lib._ptr
    calls = [lambda: lib.l3_pairs_matrix(h, 0, 131, 0, 4, 0, ptr(out)), lambda: lib.l3_pairs_matrix(h, 2, 2, 0, 4, 0, ptr(out)),
             lambda: lib.l3_pairs_matrix(h, 0, 4, 0, 4, 0, None), lambda: lib.l3_pairs_list(h, ptr(idx), ptr(idx), 2, ptr(out)),
             lambda: lib.l3_pairs_list(h, None, ptr(idx), 2, ptr(out)), lambda: lib.l3_pairs_list(h, ptr(idx), ptr(idx), 0, ptr(out)),
             lambda: lib.l3_pairs_ranks(h, ptr(badt), None, None, None, ptr(r), None),
             lambda: lib.l3_pairs_ranks(h, ptr(ok), None, ptr(ok), None, ptr(r), None),
             lambda: lib.l3_pairs_ranks(h, ptr(ok), None, None, None, None, None),
             lambda: lib.l3_pairs_set_vision(h, None, 3), lambda: lib.l3_pairs_set_vision(h, ptr(out), 0),
             lambda: lib.l3_pairs_set_head(h, None, None, None, None),
             lambda: lib.l3_pairs_create(0, 360, 350, 48, C.byref(C.c_void_p()))]
    for k, call in enumerate(calls):
        assert call() == -1, k          # L3_EINVAL
        assert lib.l3_last_error(None), k
    f = _lib.Features(np.zeros((4, 99), np.float32))
    assert lib.l3_pairs_set_audio_dev(h, f.h, 0, 4) == -1 and b'99' in lib.l3_last_error(None)
    assert lib.l3_pairs_set_audio_dev(h, f.h, 0, 5) == -1
    f.close()
    assert np.array_equal(p.matrix(), scorer130['M'])          # the sets are as they were


# ---- end to end against the oracle ---------------------------------------------------------------------------------------------
def _model(mt, seed):
    P = o.init_params(mt, seed=seed)
    rng = np.random.RandomState(seed)
    P['dense_1/bias'] = (0.1 * rng.randn(*P['dense_1/bias'].shape)).astype(np.float32)
    P['dense_2/bias'] = rng.randn(2).astype(np.float32)
    m = model.L3Model(mt)
    m._assign(P)
    return m, P


@pytest.mark.parametrize('mt,nv,na', [('tiny_L3', 3, 4), ('cnn_L3_melspec2', 2, 2)])
def test_end_to_end_against_the_oracle(gpu_required, mt, nv, na):
    m, P = _model(mt, 21)
    v, a, _ = o.synthetic_batch(max(nv, na), seed=31)
    v, a = v[:nv], a[:na]
    V, A = m.predict_towers(v, a, batch_size=2)
    sc = crossmodal.PairScorer(m).set_items(V, A)
    M = sc.margins()
    iv, ia = [x.reshape(-1) for x in np.meshgrid(np.arange(nv), np.arange(na), indexing='ij')]
    ref = o.forward(mt, P, v[iv], a[ia], False, np.float64)['logits']
    want = (ref[:, 1] - ref[:, 0]).reshape(nv, na)
    print('%s: max |margin - oracle| %.3e' % (mt, np.abs(M - want).max()))
    assert np.all(np.abs(M - want) < LOGIT_BAR)
    assert np.array_equal(sc.margins(block_bytes=1).view(np.uint32), M.view(np.uint32))          # row by row: the same bits
    d = min(nv, na)
    probs = m.predict([v[:d], a[:d]], batch_size=2)
    Pm = sc.probabilities()
    assert np.all(np.abs(np.diagonal(Pm)[:d] - probs[:, 1]) < LOGIT_BAR)
    # device-resident features give the same bits as host rows
    Vd, Ad = m.predict_towers(v, a, batch_size=2, to_device=True)
    assert np.array_equal(Vd.to_host().view(np.uint32), V.view(np.uint32)) and np.array_equal(Ad.to_host().view(np.uint32), A.view(np.uint32))
    assert np.array_equal(sc.set_items(Vd, Ad).margins().view(np.uint32), M.view(np.uint32))
    Vd.close(), Ad.close(), sc.close()
    m._drop_engines()


# ---- a tower's output: the new route against TowerModel.predict ---------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 7])
def test_predict_towers_against_tower_model(gpu_required, B):
    n = 9
    v, a, _ = o.synthetic_batch(n, seed=77)
    for construct, x, slot in ((model.construct_tiny_L3_vision_model, v, 0), (model.construct_tiny_L3_audio_model, a, 1)):
        tm = construct()[0]
        par = tm._parent
        par._ensure_engine(B)
        old = tm.predict(x)
        new = par.predict_towers(**{('video', 'audio')[slot]: x})
        assert new[1 - slot] is None and par._engine.batch == B
        got = new[slot]
        assert got.shape == old.shape == (n, (360, 350)[slot])
        diff = np.abs(got - old).max() / np.abs(old).max()
        print('tower %d, engine batch %d: %.2e of the largest value' % (slot, B, diff))
        assert diff < CROSS_BATCH_BOUND
        par._drop_engines()


# ---- from a clip bank ------------------------------------------------------------------------------------------------------------
def _two_clips():
    """2 s and 0.6 s at 4 frames per second, about 240 x 320"""
    rs = np.random.RandomState(4)
    return [(rs.randint(0, 256, (8, 240, 320, 3)).astype(np.uint8), rs.randint(-32768, 32768, (2 * 48000 + 7, 2)).astype(np.int16)),
            (rs.randint(0, 256, (3, 243, 317, 3)).astype(np.uint8), rs.randint(-32768, 32768, (int(0.6 * 48000),)).astype(np.int16))]


def test_bank_path(gpu_required):
    fps = 4
    clips = _two_clips()
    bank = avsample.ClipBank(0, sum(f.size for f, _ in clips), sum(len(x) + 8 for _, x in clips), resize=256)
    for f, x in clips:
        bank.add(f, x, 48000)
    m, _ = _model('tiny_L3', 5)
    e = m._ensure_engine(2)          # three records: one whole engine batch and one filled up
    rec, groups = crossmodal.retrieval_records(bank.clips, fps=fps)
    assert groups.tolist() == [0, 0, 1] and rec['frame'].tolist() == [2, 6, 2]
    V, A = _lib.Features.alloc(5, 360), _lib.Features.alloc(5, 350)
    e.tower_features_sampled(bank, rec, vis=V, aud=A, row0=1)
    Vh, Ah = V.download(), A.download()
    assert not Vh[0].any() and not Vh[4].any() and not Ah[0].any() and not Ah[4].any()          # only rows [1, 4) were written
    batch = avsample.sample_batch(bank, rec)
    Vr, Ar = m.predict_towers(o.preprocess_video(batch['video']), o.pcm2float(batch['audio'], np.float32))
    for got, want in ((Vh[1:4], Vr), (Ah[1:4], Ar)):
        assert np.abs(got - want).max() / np.abs(want).max() < CROSS_BATCH_BOUND
    # one destination alone, and the record checks of the sampled feed
    V2 = _lib.Features.alloc(3, 360)
    e.tower_features_sampled(bank, rec, vis=V2)
    assert np.array_equal(V2.download().view(np.uint32), Vh[1:4].view(np.uint32))
    bad = rec.copy()
    bad['audio_start'][2] = 1
    with pytest.raises(_lib.L3Error, match='sample 2'):
        e.tower_features_sampled(bank, bad, vis=V2)
    with pytest.raises(_lib.L3Error, match='rows'):
        e.tower_features_sampled(bank, rec, vis=V2, row0=1)
    # evaluate_bank is the same chain
    out, rv, ra = crossmodal.evaluate_bank(m, bank, fps=fps, ks=(1, 2), return_ranks=True)
    A2 = _lib.Features(Ah[1:4].copy())
    sc = crossmodal.PairScorer(m).set_items(V2, A2)
    wv, wa = sc.ranks(None, groups, groups)
    assert np.array_equal(rv, wv) and np.array_equal(ra, wa)
    assert out['items'] == 3 and out['clips'] == 2 and out['frame_to_audio'] == crossmodal.retrieval_metrics(wv, (1, 2))
    assert out['audio_to_frame'] == crossmodal.retrieval_metrics(wa, (1, 2)) and 0.0 <= out['avc_accuracy'] <= 1.0
    Mref = R.ranks_ref(sc.margins(), np.arange(3), np.arange(3), groups, groups)
    assert np.array_equal(wv, Mref[0]) and np.array_equal(wa, Mref[1])
    sc.close(), V.close(), A.close(), V2.close(), A2.close(), bank.close()
    m._drop_engines()


def test_cli_retrieval(gpu_required, tmp_path):
    """the command line: weights file and clip files in, the metrics of evaluate_bank out, printed and written"""
    import json
    from l3embedding_amd import cli_retrieval
    m, _ = _model('tiny_L3', 5)
    weights = str(tmp_path / 'w.h5')
    m.save_weights(weights)
    paths = []
    for i, (f, x) in enumerate(_two_clips()):
        paths.append(str(tmp_path / ('clip%d.npz' % i)))
        np.savez(paths[-1], frames=f, audio=x, rate=48000)
    out = str(tmp_path / 'metrics.json')
    got = cli_retrieval.main([weights, 'tiny_L3'] + paths + ['--fps', '4', '--recall-at', '1', '2', '--batch-size', '2', '--output-path', out])
    clips = _two_clips()
    bank = avsample.load_clips(avsample.ClipBank(0, sum(f.size for f, _ in clips), sum(len(x) + 8 for _, x in clips), 256), paths)
    want = crossmodal.evaluate_bank(m, bank, fps=4, ks=(1, 2), batch_size=2)
    bank.close()
    m._drop_engines()
    assert got == want and got['items'] == 3
    with open(out) as fh:
        assert json.load(fh) == want
