"""Cross-modal retrieval without a GPU: the factored head against the oracle's, the metrics, the retrieval records, and the argument
checks of the Python wrappers, which must refuse every bad argument before the library is called."""
import numpy as np
import pytest

from l3embedding_amd import _lib, avsample, crossmodal
from oracle import l3_oracle as o

import pairs_ref as R


def test_factored_head_equals_the_oracle_head():
    """margin_ij of the factored form = logits[1] - logits[0] of oracle.forward on the rows (v_i, a_j), to 1e-12: every (i, j) of a
    3 x 3 set, reached by rolling the audio rows (inference-mode towers treat every row on its own)."""
    mt, n = 'tiny_L3', 3
    P = o.init_params(mt, seed=5)
    rng = np.random.RandomState(3)
    P['dense_1/bias'] = rng.randn(*P['dense_1/bias'].shape).astype(np.float32)
    P['dense_2/bias'] = rng.randn(2).astype(np.float32)
    v, a, _ = o.synthetic_batch(n, seed=9)
    got = None
    for shift in range(n):
        ar = np.roll(a, -shift, axis=0)          # row i holds second (i + shift) % n
        ref = o.forward(mt, P, v, ar, False, np.float64)
        if got is None:
            got = R.factored_margins(ref['v'], ref['a'], P['dense_1/kernel'], P['dense_1/bias'], P['dense_2/kernel'], P['dense_2/bias'])
            assert ref['v'].shape == (n, 360) and ref['a'].shape == (n, 350)
        want = ref['logits'][:, 1] - ref['logits'][:, 0]
        for i in range(n):
            j = (i + shift) % n
            assert abs(got[i, j] - want[i]) <= 1e-12 * max(1.0, abs(want[i])), (i, j, got[i, j], want[i])


def test_bounds_hold_for_a_float32_emulation():
    """The derived bounds are not vacuous and not violated by a float32 NumPy run of the same chains (np.float32 arithmetic
    rounds every operation; its multiply-add is two roundings, within one more EPS per term than the fma the bound counts --
    so the emulation is held to twice the bound, and must come within it by a wide margin on average)."""
    rng = np.random.RandomState(0)
    H = 64
    u, t = rng.randn(5, H).astype(np.float32), rng.randn(7, H).astype(np.float32)
    wd, bd = rng.randn(H).astype(np.float32), np.float32(0.3)
    acc = np.zeros((5, 7), np.float32)
    for k in range(H):
        acc = np.maximum(u[:, None, k] + t[None, :, k], np.float32(0)) * wd[k] + acc
    m = acc + bd
    ref, bound = R.margins_ref(u, t, wd, bd), R.margins_bound(u, t, wd, bd)
    assert np.all(np.abs(m - ref) <= 2 * bound)
    assert np.all(bound < 1e-4 * (1 + np.abs(ref)))
    p = R.sigmoid_ref(np.array([-800.0, -90.0, 0.0, 90.0, 800.0]))
    assert np.all(np.isfinite(p)) and p[0] == 0.0 and p[2] == 0.5 and p[4] == 1.0


def test_retrieval_metrics():
    m = crossmodal.retrieval_metrics(np.array([0, 0, 3, 9, 20]), ks=(1, 5, 10))
    assert m['recall@1'] == 0.4 and m['recall@5'] == 0.6 and m['recall@10'] == 0.8
    assert m['median_rank'] == 4.0 and m['n'] == 5
    assert abs(m['mrr'] - np.mean([1, 1, 1 / 4., 1 / 10., 1 / 21.])) < 1e-15
    assert crossmodal.retrieval_metrics([0])['mrr'] == 1.0
    for bad in (np.array([], np.int64), np.array([-1]), np.array([0.5]), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            crossmodal.retrieval_metrics(bad)


def test_ranks_ref_counts_strictly_and_skips_the_own_group():
    m = np.array([[1.0, 1.0, 2.0], [0.0, 3.0, 3.0]], np.float32)
    rv, ra = R.ranks_ref(m, truth_a=[0, 1], truth_v=[0, 1, 1])
    assert rv.tolist() == [1, 0] and ra.tolist() == [0, 0, 0]
    rv, ra = R.ranks_ref(m, truth_a=[0, 0], truth_v=[0, 0, 0], group_v=[0, 1], group_a=[0, 1, 2])
    assert rv.tolist() == [1, 1] and ra.tolist() == [0, 0, 1]          # (1, 1) beats its truth but is of the query's own group


def test_retrieval_records():
    clips = [avsample.clip_info(70, 240, 320, 2 * 48000 + 100, resize=256),      # two whole seconds; 256 x 342 resized
             avsample.clip_info(3, 301, 227, int(0.4 * 48000), resize=None),     # 0.4 s: one record at 0; odd sizes, as they are
             avsample.clip_info(40, 240, 320, 3 * 48000, resize=256)]            # 40 frames: the third second's frame clamps
    rec, groups = crossmodal.retrieval_records(clips, fps=30)
    assert groups.tolist() == [0, 0, 1, 2, 2, 2] and groups.dtype == np.int32
    assert rec.dtype == _lib.SAMPLE_RECORD
    assert rec['video_clip'].tolist() == groups.tolist() and rec['audio_clip'].tolist() == groups.tolist()
    assert rec['audio_start'].tolist() == [0, 48000, 0, 0, 48000, 96000]
    assert rec['frame'].tolist() == [15, 45, 2, 15, 39, 39]
    assert (clips[0].out_height, clips[0].out_width) == (256, 342) and (clips[1].out_height, clips[1].out_width) == (301, 227)
    assert rec['start_x'].tolist() == [16, 16, 38, 16, 16, 16]          # (Ho - 224) // 2: rows
    assert rec['start_y'].tolist() == [59, 59, 1, 59, 59, 59]           # (Wo - 224) // 2: columns
    assert np.all(rec['label'] == 0) and np.all(rec['flip'] == 0) and np.all(rec['saturation'] == 1.0) and np.all(rec['brightness'] == 0)
    # every record is one the sampled feed accepts: start within [0, max(len - 48000, 0)], frame inside the clip, crop inside Ho x Wo
    for r in rec:
        c = clips[r['video_clip']]
        assert 0 <= r['audio_start'] <= max(c.samples - 48000, 0) and 0 <= r['frame'] < c.frames
        assert 0 <= r['start_x'] <= c.out_height - 224 and 0 <= r['start_y'] <= c.out_width - 224
    rec4, _ = crossmodal.retrieval_records(clips[:1], fps=4)
    assert rec4['frame'].tolist() == [2, 6]
    iv, ia = crossmodal.cross_clip_pairs(groups, 50, seed=1)
    assert np.all(groups[iv] != groups[ia])
    iv2, ia2 = crossmodal.cross_clip_pairs(groups, 50, seed=1)
    assert np.array_equal(iv, iv2) and np.array_equal(ia, ia2)


class _Recorder(object):
    """Stands in for the loaded library: every entry point returns L3_OK and is written down."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


class _Feat(_lib.Features):
    def __init__(self, n, d, device=0):          # no library call: a handle that only carries its shape
        self.h, self.device, self._shape, self.lib = 1, device, (n, d), None

    shape = property(lambda self: self._shape)

    def close(self):
        self.h = None


@pytest.fixture
def pairs(monkeypatch):
    lib = _Recorder()
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    p = _lib.Pairs(360, 350, 64)
    rng = np.random.RandomState(0)
    p.set_head(rng.randn(710, 64), rng.randn(64), rng.randn(64, 2), rng.randn(2))
    p.set_vision(rng.randn(5, 360).astype(np.float32))
    p.set_audio(_Feat(9, 350), 2, 9)
    assert (p.n_vision, p.n_audio) == (5, 7)
    assert lib.calls == ['l3_pairs_create', 'l3_pairs_set_head', 'l3_pairs_set_vision', 'l3_pairs_set_audio_dev']
    del lib.calls[:]
    yield p, lib
    p.h = None


def test_wrappers_refuse_bad_arguments_before_any_library_call(pairs, monkeypatch):
    p, lib = pairs
    z = np.zeros
    bad = [
        # NULL pointers
        lambda: p.set_head(None, z(64), z((64, 2)), z(2)),
        lambda: p.set_vision(None),
        lambda: p.list(None, [0]),
        lambda: p.list([0], None),
        lambda: p.ranks(None, None),
        # widths that do not match nv / na / head
        lambda: p.set_head(z((711, 64)), z(64), z((64, 2)), z(2)),
        lambda: p.set_head(z((710, 64)), z(63), z((64, 2)), z(2)),
        lambda: p.set_head(z((710, 64)), z(64), z((64, 3)), z(2)),
        lambda: p.set_head(z((710, 64)), z(64), z((64, 2)), z(3)),
        lambda: p.set_vision(z((4, 350), np.float32)),
        lambda: p.set_audio(z((4, 360), np.float32)),
        lambda: p.set_audio(_Feat(9, 360)),
        lambda: _lib.Pairs(360, 350, 48),
        lambda: _lib.Pairs(0, 350, 64),
        # empty sets
        lambda: p.set_vision(z((0, 360), np.float32)),
        lambda: p.set_audio(_Feat(9, 350), 4, 4),
        lambda: p.list([], []),
        # blocks or indices out of range
        lambda: p.matrix(0, 6, 0, 7),
        lambda: p.matrix(0, 5, 0, 8),
        lambda: p.matrix(-1, 5, 0, 7),
        lambda: p.matrix(3, 3, 0, 7),
        lambda: p.matrix(0, 5, 5, 4),
        lambda: p.set_audio(_Feat(9, 350), 2, 10),
        lambda: p.list([5], [0]),
        lambda: p.list([0], [7]),
        lambda: p.list([0, 1], [0]),
        lambda: p.list([-1], [0]),
        # a truth index out of range, or of the wrong length
        lambda: p.ranks(truth_a=[0, 1, 2, 3, 7]),
        lambda: p.ranks(truth_a=[0, 1, 2, 3]),
        lambda: p.ranks(truth_v=[0, 1, 2, 3, 4, 5, 0]),
        lambda: p.ranks(truth_v=[0, 1, 2, 3, 4, 0, -1]),
        lambda: p.ranks(truth_a=[0] * 5, group_v=[0] * 5),
        lambda: p.ranks(truth_a=[0] * 5, group_v=[0] * 5, group_a=[0] * 6),
        # a feature matrix on another device
        lambda: p.set_vision(_Feat(5, 360, device=1)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert lib.calls == [], (k, lib.calls)
    assert (p.n_vision, p.n_audio) == (5, 7)          # nothing was voided on the way
    # and the good calls do reach the library
    p.matrix(1, 5, 2, 7)
    p.list([0, 4], [6, 0])
    p.ranks(truth_a=[0, 1, 2, 3, 6], truth_v=[0, 1, 2, 3, 4, 0, 0], group_v=[0] * 5, group_a=[1] * 7)
    assert lib.calls == ['l3_pairs_matrix', 'l3_pairs_list', 'l3_pairs_ranks']


def test_scorer_refuses_before_any_library_call(pairs):
    p, lib = pairs
    s = crossmodal.PairScorer.__new__(crossmodal.PairScorer)
    s.handle, s.device = p, 0
    for call in (lambda: s.set_items(), lambda: s.ranks(), lambda: s.ranks(truth=[0, 1, 2, 3, 4]),
                 lambda: s.ranks(truth=([0] * 5, [0] * 7), groups_v=[0] * 5), lambda: s.pairs([9], [0])):
        with pytest.raises(ValueError):
            call()
        assert lib.calls == []
    p.n_vision = p.n_audio = 0
    with pytest.raises(ValueError):
        s.margins()
    assert lib.calls == []
