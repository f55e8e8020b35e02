"""Top-k retrieval lists and hard negatives without a GPU: the NumPy reference of the lists on hand-made matrices, the records of
mined negatives, hard_negatives' bookkeeping on a stub scorer, and the argument checks of Pairs.topk / PairScorer.topk, which must
refuse every bad argument before the library is called."""
import ctypes
import os
import re

import numpy as np
import pytest

from l3embedding_amd import _build, _lib, avsample, crossmodal

from pairs_topk_ref import same_lists, topk_ref

INF = np.float32(np.inf)


# ---- the reference itself ------------------------------------------------------------------------------------------------------
def test_topk_ref_breaks_a_tie_by_the_index():
    m = np.array([[1.0, 3.0, 3.0, 2.0], [0.0, -0.0, 5.0, 5.0]], np.float32)
    idx, mar = topk_ref(m, 3)
    assert idx.tolist() == [[1, 2, 3], [2, 3, 0]]          # +0 and -0 are equal: index 0 before index 1
    assert mar.tolist() == [[3.0, 3.0, 2.0], [5.0, 5.0, 0.0]]
    assert idx.dtype == np.int32 and mar.dtype == np.float32
    # the other direction is the transpose
    idx, _ = topk_ref(m.T, 1)
    assert idx.tolist() == [[0], [0], [1], [1]]


def test_topk_ref_skips_the_own_group_and_keeps_the_truth():
    m = np.array([[9.0, 8.0, 7.0, 6.0], [1.0, 2.0, 3.0, 4.0]], np.float32)
    gq, gc = [0, 1], [0, 0, 1, 1]
    idx, mar = topk_ref(m, 2, group_q=gq, group_c=gc)
    assert idx.tolist() == [[2, 3], [1, 0]] and mar.tolist() == [[7.0, 6.0], [2.0, 1.0]]
    idx, mar = topk_ref(m, 2, truth=[1, 3], group_q=gq, group_c=gc)          # the truths are of the queries' own groups
    assert idx.tolist() == [[1, 2], [3, 1]] and mar.tolist() == [[8.0, 7.0], [4.0, 2.0]]
    idx, _ = topk_ref(m, 2, truth=[2, 0], group_q=gq, group_c=gc)            # a truth of another group changes nothing
    assert idx.tolist() == [[2, 3], [1, 0]]


def test_topk_ref_fills_short_lists_and_never_lists_nan():
    m = np.array([[1.0, np.nan, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    idx, mar = topk_ref(m, 4)
    assert idx.tolist() == [[0, 2, -1, -1], [-1] * 4]          # a margin of -inf is a candidate; NaN is not
    assert mar[0].tolist() == [1.0, -INF, -INF, -INF] and np.all(mar[1] == -INF)
    idx, mar = topk_ref(np.ones((1, 3), np.float32), 2, group_q=[5], group_c=[5, 5, 5])
    assert idx.tolist() == [[-1, -1]] and np.all(mar == -INF)
    idx, mar = topk_ref(np.ones((1, 3), np.float32), 2, truth=[1], group_q=[5], group_c=[5, 5, 5])
    assert idx.tolist() == [[1, -1]] and mar.tolist() == [[1.0, -INF]]
    assert same_lists((idx, mar), (idx.copy(), mar.copy())) and not same_lists((idx, mar), (idx, -mar))


# ---- records of mined negatives ------------------------------------------------------------------------------------------------
def _three_clips():
    return [avsample.clip_info(70, 240, 320, 2 * 48000 + 100, resize=256),      # two whole seconds; 256 x 342 resized
            avsample.clip_info(3, 301, 227, int(0.4 * 48000), resize=None),     # 0.4 s: one record at 0; odd sizes, as they are
            avsample.clip_info(40, 240, 320, 3 * 48000, resize=256)]            # 40 frames: the third second's frame clamps


def test_negative_records_field_by_field():
    clips = _three_clips()
    rec, groups = crossmodal.retrieval_records(clips, fps=30)
    assert groups.tolist() == [0, 0, 1, 2, 2, 2]
    iv, ia = np.array([0, 2, 5, 1]), np.array([2, 4, 0, 3])
    neg = crossmodal.negative_records(rec, iv, ia)
    assert neg.dtype == _lib.SAMPLE_RECORD and len(neg) == 4
    assert neg['video_clip'].tolist() == [0, 1, 2, 0] and neg['frame'].tolist() == [15, 2, 39, 45]
    assert neg['start_x'].tolist() == [16, 38, 16, 16] and neg['start_y'].tolist() == [59, 1, 59, 59]
    assert neg['audio_clip'].tolist() == [1, 2, 0, 2] and neg['audio_start'].tolist() == [0, 48000, 0, 0]
    assert np.all(neg['label'] == 1)
    assert np.all(neg['flip'] == 0) and np.all(neg['sat_first'] == 1) and np.all(neg['saturation'] == 1.0)
    assert np.all(neg['brightness'] == 0) and np.all(neg['u_gain'] == 0)
    # every record is one the sampled feed accepts: the start within its AUDIO clip, frame and crop inside its VIDEO clip
    for r in neg:
        cv, ca = clips[r['video_clip']], clips[r['audio_clip']]
        assert 0 <= r['audio_start'] <= max(ca.samples - 48000, 0) and 0 <= r['frame'] < cv.frames
        assert 0 <= r['start_x'] <= cv.out_height - 224 and 0 <= r['start_y'] <= cv.out_width - 224
    # the video side's augmentation fields travel with the frame, the gain with the second
    rec2 = rec.copy()
    rec2['flip'][2], rec2['brightness'][2], rec2['u_gain'][4] = 1, 0.25, 0.5
    neg2 = crossmodal.negative_records(rec2, iv, ia)
    assert neg2['flip'].tolist() == [0, 1, 0, 0] and neg2['brightness'].tolist() == [0, 0.25, 0, 0]
    assert neg2['u_gain'].tolist() == [0, 0.5, 0, 0]
    assert len(crossmodal.negative_records(rec, np.zeros(0, np.int32), np.zeros(0, np.int32))) == 0
    for bad in ((iv, ia[:3]), ([6], [0]), ([0], [-1]), ([0.5], [0])):
        with pytest.raises(ValueError):
            crossmodal.negative_records(rec, *bad)


class _StubScorer(object):
    """margins M; topk as the contract has it, through the reference"""

    def __init__(self, M):
        self.M, self.calls = np.asarray(M, np.float32), []

    shape = property(lambda self: self.M.shape)

    def topk(self, k, truth=None, groups_v=None, groups_a=None):
        self.calls.append((k, truth))
        return topk_ref(self.M, k, None, groups_v, groups_a), topk_ref(self.M.T, k, None, groups_a, groups_v)


def test_hard_negatives_drops_fillers_and_duplicates():
    x = 99.0          # own-clip pairs: high scores that must not come back
    M = [[x, x, 0.5], [x, x, 0.4], [0.3, 0.2, x]]
    groups = np.array([0, 0, 1], np.int32)
    s = _StubScorer(M)
    iv, ia, m = crossmodal.hard_negatives(s, groups, 1)
    # frames: (0, 2), (1, 2), (2, 0); seconds: (2, 0) again, (2, 1) new, (0, 2) again
    assert list(zip(iv.tolist(), ia.tolist())) == [(0, 2), (1, 2), (2, 0), (2, 1)]
    assert m.tolist() == [np.float32(v) for v in (0.5, 0.4, 0.3, 0.2)] and iv.dtype == ia.dtype == np.int32
    assert s.calls == [(1, None)]          # no truth pair is kept
    # per_item 2: frames 0 and 1 have one candidate each -- a filler each --, and the seconds' lists add nothing new
    iv, ia, m = crossmodal.hard_negatives(s, groups, 2)
    assert list(zip(iv.tolist(), ia.tolist())) == [(0, 2), (1, 2), (2, 0), (2, 1)]
    assert np.all(np.isfinite(m)) and np.all(groups[iv] != groups[ia])
    # one clip only: nothing but fillers
    iv, ia, m = crossmodal.hard_negatives(_StubScorer(M), np.zeros(3, np.int32), 2)
    assert len(iv) == len(ia) == len(m) == 0
    for bad in (groups[:2], np.zeros((3, 1), np.int32)):
        with pytest.raises(ValueError):
            crossmodal.hard_negatives(s, bad, 1)


# ---- the wrappers' argument checks ---------------------------------------------------------------------------------------------
class _Recorder(object):
    """Stands in for the loaded library: every entry point returns L3_OK and is written down."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


@pytest.fixture
def pairs(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    p = _lib.Pairs(360, 350, 64)
    rng = np.random.RandomState(0)
    p.set_head(rng.randn(710, 64), rng.randn(64), rng.randn(64, 2), rng.randn(2))
    p.set_vision(rng.randn(5, 360).astype(np.float32))
    p.set_audio(rng.randn(7, 350).astype(np.float32))
    assert (p.n_vision, p.n_audio) == (5, 7)
    del lib.calls[:]
    yield p, lib
    p.h = None


def test_topk_wrappers_refuse_bad_arguments_before_any_library_call(pairs):
    p, lib = pairs
    s = crossmodal.PairScorer.__new__(crossmodal.PairScorer)
    s.handle, s.device = p, 0
    gv, ga, ta, tv = [0] * 5, [1] * 7, [0, 1, 2, 3, 6], [0, 1, 2, 3, 4, 0, 0]
    bad = [
        # k out of range, or no integer
        lambda: p.topk(0), lambda: p.topk(65), lambda: p.topk(-1), lambda: p.topk(2.5), lambda: p.topk(None), lambda: p.topk(True),
        lambda: s.topk(0), lambda: s.topk(65),
        # truth without groups
        lambda: p.topk(3, truth_a=ta), lambda: p.topk(3, truth_v=tv), lambda: s.topk(3, truth=(ta, tv)),
        lambda: s.topk(3, truth=(ta, None)),
        # one group vector only
        lambda: p.topk(3, groups_v=gv), lambda: p.topk(3, groups_a=ga), lambda: s.topk(3, groups_v=gv),
        lambda: s.topk(3, None, None, ga),
        # wrong lengths
        lambda: p.topk(3, groups_v=gv, groups_a=ga[:6]), lambda: p.topk(3, groups_v=gv + [0], groups_a=ga),
        lambda: p.topk(3, truth_a=ta[:4], groups_v=gv, groups_a=ga), lambda: p.topk(3, truth_v=tv + [0], groups_v=gv, groups_a=ga),
        lambda: s.topk(3, (ta[:4], tv), gv, ga), lambda: p.topk(3, groups_v=np.zeros((5, 1), int), groups_a=ga),
        # truth out of range, groups that are no ids
        lambda: p.topk(3, truth_a=[0, 1, 2, 3, 7], groups_v=gv, groups_a=ga),
        lambda: p.topk(3, truth_v=[0, 1, 2, 3, 4, 5, 0], groups_v=gv, groups_a=ga),
        lambda: p.topk(3, truth_a=[0, 1, 2, 3, -1], groups_v=gv, groups_a=ga),
        lambda: s.topk(3, (ta, [5] * 7), gv, ga),
        lambda: p.topk(3, groups_v=[0.5] * 5, groups_a=ga), lambda: p.topk(3, groups_v=[-1] * 5, groups_a=ga),
        # directions, and a truth that is no pair
        lambda: p.topk(3, directions=()), lambda: p.topk(3, directions=('v2a', 'both')), lambda: p.topk(3, directions='up'),
        lambda: s.topk(3, truth=ta, groups_v=gv, groups_a=ga),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert lib.calls == [], (k, lib.calls)
    assert (p.n_vision, p.n_audio) == (5, 7)
    # the good calls reach the library, once each, and give arrays of the promised shapes
    (iv, mv), (ia, ma) = p.topk(64, ta, tv, gv, ga)
    assert iv.shape == mv.shape == (5, 64) and ia.shape == ma.shape == (7, 64) and iv.dtype == np.int32 and ma.dtype == np.float32
    v2a, a2v = p.topk(1, directions='a2v')
    assert v2a is None and a2v[0].shape == (7, 1)
    v2a, a2v = p.topk(np.int64(2), groups_v=gv, groups_a=ga, directions=('v2a',))
    assert a2v is None and v2a[1].shape == (5, 2)
    s.topk(3), s.topk(3, None, gv, ga), s.topk(3, (ta, None), gv, ga)
    assert lib.calls == ['l3_pairs_topk'] * 6
    # sets that are not set
    del lib.calls[:]
    p.n_audio = 0
    for call in (lambda: p.topk(3), lambda: s.topk(3)):
        with pytest.raises(ValueError):
            call()
    p.n_audio, p.head_set = 7, False
    with pytest.raises(ValueError):
        p.topk(3)
    assert lib.calls == []


def test_op_pair_topk_refuses_before_any_library_call(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    u, t, wd = np.zeros((3, 64), np.float32), np.zeros((4, 64), np.float32), np.zeros(64, np.float32)
    bad = [lambda: _lib.op_pair_topk(u, t, wd, 0.0, 0), lambda: _lib.op_pair_topk(u, t, wd, 0.0, 65),
           lambda: _lib.op_pair_topk(u, t[:, :32], wd, 0.0, 2), lambda: _lib.op_pair_topk(u, t, wd[:32], 0.0, 2),
           lambda: _lib.op_pair_topk(u[:0], t, wd, 0.0, 2), lambda: _lib.op_pair_topk(u, t, wd, 0.0, 2, segments=-1),
           lambda: _lib.op_pair_topk(u, t, wd, 0.0, 2, segments=257), lambda: _lib.op_pair_topk(u, t, wd, 0.0, 2, truth=[0, 1, 2]),
           lambda: _lib.op_pair_topk(u, t, wd, 0.0, 2, group_q=[0, 1, 2]),
           lambda: _lib.op_pair_topk(u, t, wd, 0.0, 2, truth=[0, 1, 4], group_q=[0] * 3, group_c=[0] * 4),
           lambda: _lib.op_pair_topk(u, t, wd, 0.0, 2, truth=[0, 1], group_q=[0] * 3, group_c=[0] * 4),
           lambda: _lib.op_pair_topk(u, t, wd, 0.0, 2, group_q=[0] * 3, group_c=[0] * 3)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert lib.calls == [], k
    idx, margin = _lib.op_pair_topk(u, t, wd, 0.0, 2, truth=[0, 1, 3], group_q=[0] * 3, group_c=[0] * 4, segments=3)
    assert idx.shape == margin.shape == (3, 2) and lib.calls == ['l3_op_pair_topk']


def test_evaluate_bank_refuses_a_bad_topk_before_anything_runs():
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            crossmodal.evaluate_bank(None, None, topk=bad)


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_exported():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'l3hip.h')).read(), flags=re.S)
    _build.build()
    raw = ctypes.CDLL(_lib.lib_path())
    for name, nargs in (('l3_pairs_topk', 10), ('l3_op_pair_topk', 15)):
        decl = re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, src)
        assert decl, name + ' is not declared in include/l3hip.h'
        assert len(decl.group(1).split(',')) == nargs == len(_lib.SIGNATURES[name][1])
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and hasattr(raw, name)
    assert re.search(r'#define\s+L3_PAIRS_TOPK_MAX\s+64\b', src) and _lib.PAIRS_TOPK_MAX == 64
    assert callable(_lib.Pairs.topk) and callable(_lib.op_pair_topk) and callable(crossmodal.PairScorer.topk)
    assert callable(crossmodal.hard_negatives) and callable(crossmodal.negative_records)
