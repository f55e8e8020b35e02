"""Cross-modal retrieval with a trained AVC model: does this frame go with this second of sound, asked of every (frame, second)
pair of a held-out set -- the evaluation the L3 / "Objects that Sound" line of work reports beside AVC accuracy.

The head factors over the concatenation: each tower runs once per item (`L3Model.predict_towers`, or
`Engine.tower_features_sampled` straight from a `ClipBank`), the two halves of dense_1 are ordinary projections, and a pair costs
`head` x (add, max, fma) on the GPU (csrc/pairs.hip).  `PairScorer` keeps the projected sets on the device and gives the matrix of
margins (logit(corresponding) - logit(not)) in blocks, probabilities, listed pairs, and retrieval ranks and top-k lists in both
directions without ever storing the matrix.  `set_maps` puts one side's last feature map there location by location: `maps` are the
sound localisation maps of listed pairs, `peaks` / `peak_ranks` score a pair by its best location (csrc/locmap.hip).  The lists without the truth pair are the hardest negatives (`hard_negatives`,
`negative_records`).
"""
import numpy as np

from . import _lib

T = 48000            # one second at the sampler's rate
CROP = 224


class PairScorer(object):
    """The AVC head of `model` over pairs.  set_items(V, A): the towers' outputs as arrays or usc.DeviceFeatures."""

    def __init__(self, model, device=None):
        P = model._weights_dict()
        w1, b1, w2, b2 = (np.asarray(P[k], np.float32) for k in ('dense_1/kernel', 'dense_1/bias', 'dense_2/kernel', 'dense_2/bias'))
        nv = 360 if model.model_type == 'tiny_L3' else 512          # the vision tower's flattened output (TowerModel)
        self.device = model.device if device is None else int(device)
        self.model = model
        self.handle = _lib.Pairs(nv, w1.shape[0] - nv, w1.shape[1], device=self.device)
        self.handle.set_head(w1, b1, w2, b2)

    @property
    def shape(self):
        return (self.handle.n_vision, self.handle.n_audio)

    @staticmethod
    def _rows(x):
        handle = getattr(x, 'handle', None)          # usc.DeviceFeatures
        return handle if isinstance(handle, _lib.Features) else x

    def set_items(self, V=None, A=None):
        """V (Nv, nv) frames' and A (Na, na) seconds' tower outputs; a side left None keeps its set"""
        if V is None and A is None:
            raise ValueError('give V, A or both')
        if V is not None:
            self.handle.set_vision(self._rows(V))
        if A is not None:
            self.handle.set_audio(self._rows(A))
        return self

    def _blocks(self, block_bytes, prob):
        nv, na = self.shape
        if nv < 1 or na < 1:
            raise ValueError('set_items comes first')
        rows = max(1, int(block_bytes) // (4 * na))
        out = np.empty((nv, na), np.float32)
        for v0 in range(0, nv, rows):
            v1 = min(nv, v0 + rows)
            out[v0:v1] = self.handle.matrix(v0, v1, 0, na, prob=prob)
        return out

    def margins(self, block_bytes=256 << 20):
        """(Nv, Na) margins, downloaded in blocks of whole rows of at most block_bytes"""
        return self._blocks(block_bytes, False)

    def probabilities(self, block_bytes=256 << 20):
        """(Nv, Na) P(corresponding) = sigmoid(margin)"""
        return self._blocks(block_bytes, True)

    def pairs(self, iv, ia):
        """margins of the listed pairs (iv[q], ia[q])"""
        return self.handle.list(iv, ia)

    def ranks(self, truth=None, groups_v=None, groups_a=None):
        """(rank_v2a, rank_a2v), 0-based: for every frame the number of seconds that score strictly above its own second, and for
        every second the frames likewise; items of the same group (clip) as the query are not negatives.  truth None: frame i goes
        with second i (Nv == Na).  Otherwise (truth_a, truth_v): the index of every frame's second and of every second's frame; one
        of them may be None, and that direction comes back as None."""
        nv, na = self.shape
        if truth is None:
            if nv != na:
                raise ValueError('truth=None pairs frame i with second i and needs Nv == Na, not %d and %d' % (nv, na))
            truth = (np.arange(nv, dtype=np.int32), np.arange(na, dtype=np.int32))
        if not isinstance(truth, (tuple, list)) or len(truth) != 2:
            raise ValueError('truth is None or the pair (truth_a, truth_v)')
        return self.handle.ranks(truth[0], truth[1], groups_v, groups_a)

    def topk(self, k, truth=None, groups_v=None, groups_a=None):
        """((idx_v2a, margin_v2a), (idx_a2v, margin_a2v)): every frame's k best-scoring seconds and every second's k best-scoring
        frames, (n, k) each, best first (ties: the smaller index), filled up with index -1 and margin -inf; items of the query's
        own group (clip) are skipped.  truth None: no truth pair is kept -- with groups these are the hardest negatives.  Otherwise
        (truth_a, truth_v) as in ranks, one of them possibly None: the query's own partner stays a candidate, which gives the
        retrieval list that goes with recall@k.  A truth needs groups."""
        if truth is None:
            truth = (None, None)
        if not isinstance(truth, (tuple, list)) or len(truth) != 2:
            raise ValueError('truth is None or the pair (truth_a, truth_v)')
        return self.handle.topk(k, truth[0], truth[1], groups_v, groups_a)

    # ---- sound localisation maps: the head at every location of one side's last feature map ----
    def set_maps(self, side, source, chunk_items=64):
        """The location map of one side: 0 the frames' image locations, queried by the seconds of set_items(A=...); 1 the seconds'
        time-frequency locations, queried by the frames.  source: the model's input rows ((n, 224, 224, 3) frames / (n, 1, 48000)
        waveforms), (bank, records) of an avsample.ClipBank, or (location rows, (H, W)) as L3Model.predict_locations returns them.
        The towers run chunk_items items at a time and only the projected rows stay: 0.4 MB a frame against 1.6 MB of raw
        locations."""
        if side not in (0, 1):
            raise ValueError('side must be 0 (vision locations) or 1 (audio locations), not %r' % (side,))
        chunk = int(chunk_items)
        if chunk < 1:
            raise ValueError('chunk_items must be >= 1')
        pair = isinstance(source, (tuple, list)) and len(source) == 2
        if pair and isinstance(self._rows(source[0]), _lib.Features):
            loc, (H, W) = self._rows(source[0]), source[1]
            H, W = int(H), int(W)
            rows = loc.shape[0]
            if H < 1 or W < 1 or rows < 1 or rows % (H * W):
                raise ValueError('%d location rows are not a whole number of %d x %d maps' % (rows, H, W))
            n = rows // (H * W)
            self.handle.map_reserve(side, n, H, W)
            for i0 in range(0, n, chunk):
                self.handle.map_put(loc, i0 * H * W, i0, min(chunk, n - i0))
            return self
        if pair:
            bank, records = source[0], _lib.sample_records(source[1])
            n = len(records)
        else:
            bank, records = None, np.ascontiguousarray(source, dtype=np.float32)
            n = len(records)
        if n < 1:
            raise ValueError('the source holds no items')
        model = self.model
        e = model._ensure_engine(max(1, min(32, n)) if model._engine is None else model._engine.batch)
        H, W, C = e.tower_locations_shape(side)
        self.handle.map_reserve(side, n, H, W)
        buf = _lib.Features.alloc(min(chunk, n) * H * W, C, device=self.device)
        try:
            for i0 in range(0, n, chunk):
                i1 = min(n, i0 + chunk)
                if bank is not None:
                    e.tower_locations_sampled(bank, records[i0:i1], side, buf)
                else:
                    e.tower_locations(side, records[i0:i1], dst=buf)
                self.handle.map_put(buf, 0, i0, i1 - i0)
        finally:
            buf.close()
        return self

    def _map_pairs(self, iv, ia):
        side = self.handle.map_side
        if side < 0:
            raise ValueError('set_maps comes first')
        n = len(iv) if iv is not None and np.ndim(iv) == 1 else -1
        if n < 1 or ia is None or np.ndim(ia) != 1 or len(ia) != n:
            raise ValueError('iv and ia must be two equally long, non-empty 1-d index arrays')
        items, queries = (iv, ia) if side == 0 else (ia, iv)
        queries = _lib._index32(queries, 'ia' if side == 0 else 'iv', n, self.handle.map_queries, 'pair')
        ptr, order = _lib.csr_by_item(items, self.handle.map_items)
        return ptr, order, queries[order]

    def maps(self, iv, ia, peaks=False):
        """The maps of the listed pairs (frame iv[q], second ia[q]) in the caller's order: (Q, H, W) margins over the locations of
        the map's side -- of frame iv[q] scored against second ia[q] (side 0), or of second ia[q] against frame iv[q] (side 1).
        peaks: (maps, peak (Q,), arg (Q,)) with the best location's margin and index y W + x (-1: every margin NaN)."""
        ptr, order, q = self._map_pairs(iv, ia)
        H, W = self.handle.map_hw
        m, pk, ar = self.handle.map_list(ptr, q, maps=True, peaks=bool(peaks))
        out = np.empty_like(m)
        out[order] = m
        out = out.reshape(len(q), H, W)
        if not peaks:
            return out
        peak, arg = np.empty_like(pk), np.empty_like(ar)
        peak[order], arg[order] = pk, ar
        return out, peak, arg

    def pair_peaks(self, iv, ia):
        """(peak, arg) of the listed pairs without their maps"""
        ptr, order, q = self._map_pairs(iv, ia)
        _, pk, ar = self.handle.map_list(ptr, q, maps=False, peaks=True)
        peak, arg = np.empty_like(pk), np.empty_like(ar)
        peak[order], arg[order] = pk, ar
        return peak, arg

    def peaks(self, block_bytes=256 << 20):
        """(S, arg), both (Nv, Na): the best-location margin of every (frame, second) pair and the location attaining it, downloaded
        in blocks of whole items of at most block_bytes; no map is stored anywhere"""
        h = self.handle
        if h.map_side < 0:
            raise ValueError('set_maps comes first')
        ni, nq = h.map_items, h.map_queries
        rows = max(1, int(block_bytes) // (8 * max(nq, 1)))
        S, arg = np.empty((ni, nq), np.float32), np.empty((ni, nq), np.int32)
        for i0 in range(0, ni, rows):
            i1 = min(ni, i0 + rows)
            S[i0:i1], arg[i0:i1] = h.map_peaks(i0, i1, 0, nq)
        return (S, arg) if h.map_side == 0 else (np.ascontiguousarray(S.T), np.ascontiguousarray(arg.T))

    def peak_ranks(self, truth=None, groups_v=None, groups_a=None):
        """ranks() under best-location scoring: the score of a (frame, second) pair is the maximum of its map"""
        h = self.handle
        if h.map_side < 0:
            raise ValueError('set_maps comes first')
        nv, na = (h.map_items, h.n_audio) if h.map_side == 0 else (h.n_vision, h.map_items)
        if truth is None:
            if nv != na:
                raise ValueError('truth=None pairs frame i with second i and needs Nv == Na, not %d and %d' % (nv, na))
            truth = (np.arange(nv, dtype=np.int32), np.arange(na, dtype=np.int32))
        if not isinstance(truth, (tuple, list)) or len(truth) != 2:
            raise ValueError('truth is None or the pair (truth_a, truth_v)')
        return h.map_ranks(truth[0], truth[1], groups_v, groups_a)

    def close(self):
        self.handle.close()


def upsample_map(m, size):
    """A map (..., H, W) -> (..., size[0], size[1]) for laying it over the frame it belongs to (28 x 28 -> 224 x 224): separable
    linear interpolation with half-pixel centres -- output pixel y samples the input at (y + 0.5) H / size[0] - 0.5 -- and the
    edges clamped.  Host NumPy, in float64; returned as float32 unless m is float64."""
    m = np.asarray(m)
    if isinstance(size, (int, np.integer)):
        size = (size, size)
    if m.ndim < 2 or m.shape[-1] < 1 or m.shape[-2] < 1 or m.dtype.kind != 'f':
        raise ValueError('m must be a float array (..., H, W)')
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError('size must be (height, width) >= 1')

    def taps(n_in, n_out):
        x = np.clip((np.arange(n_out) + 0.5) * n_in / n_out - 0.5, 0.0, n_in - 1.0)
        lo = np.floor(x).astype(np.int64)
        hi = np.minimum(lo + 1, n_in - 1)
        A = np.zeros((n_out, n_in))
        np.add.at(A, (np.arange(n_out), lo), 1.0 - (x - lo))
        np.add.at(A, (np.arange(n_out), hi), x - lo)
        return A

    out = taps(m.shape[-2], int(size[0])) @ m.astype(np.float64) @ taps(m.shape[-1], int(size[1])).T
    return out if m.dtype == np.float64 else out.astype(np.float32)


def retrieval_metrics(ranks, ks=(1, 5, 10)):
    """0-based ranks -> {'recall@k': mean(rank < k), 'median_rank': 1-based, 'mrr': mean(1 / (rank + 1)), 'n'}"""
    r = np.asarray(ranks)
    if r.ndim != 1 or len(r) < 1 or r.dtype.kind not in 'iu' or r.min() < 0:
        raise ValueError('ranks must be a non-empty 1-d array of non-negative integers')
    r = r.astype(np.int64)
    out = {'recall@%d' % k: float(np.mean(r < k)) for k in ks}
    out['median_rank'] = float(np.median(r + 1))
    out['mrr'] = float(np.mean(1.0 / (r + 1)))
    out['n'] = int(len(r))
    return out


def retrieval_records(clip_infos, fps=30):
    """One SAMPLE record per whole second s of every clip (avsample.ClipInfo rows, by clip id): audio_start = 48000 s, frame =
    min(int(s fps) + fps // 2, n_frames - 1) -- the middle of the second --, the centre crop of the resized frame, label 0 (the
    pair corresponds), no augmentation.  A clip shorter than a second gives one record at start 0, which the seconds kernel pads
    with zeros.  Returns (records, the clip id of each): the ids serve as the groups of PairScorer.ranks."""
    fps = int(fps)
    if fps < 1:
        raise ValueError('fps must be >= 1')
    rows = []
    for cid, c in enumerate(clip_infos):
        for s in range(max(1, int(c.samples) // T)):
            rows.append((cid, min(int(s * fps) + fps // 2, int(c.frames) - 1), T * s, (int(c.out_height) - CROP) // 2,
                         (int(c.out_width) - CROP) // 2))
    rec = np.zeros(len(rows), _lib.SAMPLE_RECORD)
    for i, (cid, frame, start, sx, sy) in enumerate(rows):
        rec['video_clip'][i] = rec['audio_clip'][i] = cid
        rec['frame'][i], rec['audio_start'][i] = frame, start
        rec['start_x'][i], rec['start_y'][i] = sx, sy
    rec['sat_first'], rec['saturation'] = 1, 1.0
    return rec, np.array([r[0] for r in rows], np.int32)


def cross_clip_pairs(groups, n, seed=0):
    """n (frame, second) index pairs whose items come from different clips, drawn with np.random.RandomState(seed): a frame
    uniformly, then a second uniformly among those of the other clips."""
    groups = np.asarray(groups)
    if len(np.unique(groups)) < 2:
        raise ValueError('cross-clip pairs need items of at least two clips')
    rng = np.random.RandomState(seed)
    iv = rng.randint(len(groups), size=int(n)).astype(np.int32)
    ia = np.empty(int(n), np.int32)
    for q, i in enumerate(iv):
        others = np.flatnonzero(groups != groups[i])
        ia[q] = others[rng.randint(len(others))]
    return iv, ia


def hard_negatives(scorer, groups, per_item):
    """(iv, ia, margin): for every frame its `per_item` highest-scoring seconds of other clips and for every second its `per_item`
    highest-scoring frames of other clips (scorer.topk without a truth; groups: the clip id of item i on both sides, Nv == Na),
    concatenated frames' lists first, the fillers of short lists dropped and a pair that both directions found kept once, where it
    first stands."""
    nv, na = scorer.shape
    groups = np.asarray(groups)
    if groups.ndim != 1 or len(groups) != nv or nv != na:
        raise ValueError('groups holds the clip of item i on both sides: %d frames and %d seconds need %d ids' % (nv, na, nv))
    (jv, mv), (ja, ma) = scorer.topk(per_item, None, groups, groups)
    k = jv.shape[1]
    iv = np.concatenate([np.repeat(np.arange(nv, dtype=np.int32), k), ja.reshape(-1)])
    ia = np.concatenate([jv.reshape(-1), np.repeat(np.arange(na, dtype=np.int32), k)])
    m = np.concatenate([mv.reshape(-1), ma.reshape(-1)])
    keep = np.flatnonzero((iv >= 0) & (ia >= 0))
    _, first = np.unique(iv[keep].astype(np.int64) * na + ia[keep], return_index=True)
    keep = keep[np.sort(first)]
    return iv[keep].astype(np.int32), ia[keep].astype(np.int32), m[keep]


VIDEO_FIELDS = ('video_clip', 'frame', 'start_x', 'start_y', 'flip', 'sat_first', 'saturation', 'brightness')
AUDIO_FIELDS = ('audio_clip', 'audio_start', 'u_gain')


def negative_records(records, iv, ia):
    """SAMPLE records of the pairs (iv[q], ia[q]) of item records (retrieval_records): the video fields of records[iv], the audio
    fields of records[ia], label 1 (not corresponding) -- ready for upload_batch_sampled / stage_batch_sampled."""
    records = _lib.sample_records(records)
    n = len(records)
    iv, ia = np.asarray(iv), np.asarray(ia)
    if iv.ndim != 1 or iv.shape != ia.shape or iv.dtype.kind not in 'iu' or ia.dtype.kind not in 'iu':
        raise ValueError('iv and ia must be two equally long 1-d index arrays')
    if len(iv) and (min(iv.min(), ia.min()) < 0 or max(iv.max(), ia.max()) >= n):
        raise ValueError('an index outside the %d records' % n)
    out = np.zeros(len(iv), _lib.SAMPLE_RECORD)
    for name in VIDEO_FIELDS:
        out[name] = records[name][iv]
    for name in AUDIO_FIELDS:
        out[name] = records[name][ia]
    out['label'] = 1
    return out


def _lists(idx, margin, groups):
    return {'index': idx, 'clip': np.where(idx >= 0, groups[np.maximum(idx, 0)], -1).astype(np.int32), 'margin': margin}


def evaluate_bank(model, bank, fps=30, ks=(1, 5, 10), batch_size=32, seed=0, return_ranks=False, topk=0, peak=False, maps_top=None):
    """Retrieval over every whole second of every clip of an avsample.ClipBank: retrieval_records -> both towers' outputs of each
    record on the GPU (Engine.tower_features_sampled) -> PairScorer.ranks with the clips as groups.  Returns {'frame_to_audio',
    'audio_to_frame': retrieval_metrics, 'avc_accuracy': accuracy at margin 0 on the true pairs against as many seeded cross-clip
    pairs, 'items', 'clips'}; with return_ranks also the two rank vectors.  topk > 0 adds 'lists': {'frame_to_audio', 'audio_to_frame':
    {'index' (n, topk) the retrieved items best first (-1: none), 'clip' their clip ids (-1), 'margin'}}, the truth pair kept.
    peak adds 'peak': {'frame_to_audio', 'audio_to_frame': retrieval_metrics of the same ranks under best-location scoring -- a
    pair's score is the maximum of the head over the frame's image locations (PairScorer.peak_ranks) --, 'rank_v2a',
    'rank_a2v' the rank vectors}.  maps_top (needs peak; an integer >= 0) adds 'maps': {'truth': {'map' (n, H, W), 'peak', 'arg'} of
    every true pair and, when maps_top > 0 (needs topk >= maps_top), 'top': the same with a leading (n, maps_top) for each frame's
    first maps_top retrieved seconds (an empty slot: NaN maps, peak -inf, arg -1)}."""
    if maps_top is not None and (not peak or int(maps_top) < 0 or int(maps_top) > int(topk)):
        raise ValueError('maps_top needs peak=True and 0 <= maps_top <= topk')
    topk = int(topk)
    if not 0 <= topk <= _lib.PAIRS_TOPK_MAX:
        raise ValueError('topk must be in [0, %d]' % _lib.PAIRS_TOPK_MAX)
    records, groups = retrieval_records(bank.clips, fps=fps)
    n = len(records)
    e = model._ensure_engine(max(1, min(batch_size, n)) if model._engine is None else model._engine.batch)
    V = _lib.Features.alloc(n, e.tower_dim(0), device=model.device)
    A = _lib.Features.alloc(n, e.tower_dim(1), device=model.device)
    scorer = None
    try:
        e.tower_features_sampled(bank, records, vis=V, aud=A)
        scorer = PairScorer(model).set_items(V, A)
        rv, ra = scorer.ranks(None, groups, groups)
        idx = np.arange(n, dtype=np.int32)
        pos = scorer.pairs(idx, idx)
        out = {'frame_to_audio': retrieval_metrics(rv, ks), 'audio_to_frame': retrieval_metrics(ra, ks), 'items': n,
               'clips': len(bank.clips)}
        if len(np.unique(groups)) >= 2:
            neg = scorer.pairs(*cross_clip_pairs(groups, n, seed))
            out['avc_accuracy'] = float((np.sum(pos > 0) + np.sum(neg <= 0)) / (2.0 * n))
        else:
            out['avc_accuracy'] = None
        if topk:
            (jv, mv), (ja, ma) = scorer.topk(topk, (idx, idx), groups, groups)
            out['lists'] = {'frame_to_audio': _lists(jv, mv, groups), 'audio_to_frame': _lists(ja, ma, groups)}
        if peak:
            scorer.set_maps(0, (bank, records), chunk_items=max(1, min(64, e.batch)))
            pv, pa = scorer.peak_ranks(None, groups, groups)
            out['peak'] = {'frame_to_audio': retrieval_metrics(pv, ks), 'audio_to_frame': retrieval_metrics(pa, ks),
                           'rank_v2a': pv, 'rank_a2v': pa}
        if maps_top is not None:
            m, pk, ar = scorer.maps(idx, idx, peaks=True)
            out['maps'] = {'truth': {'map': m, 'peak': pk, 'arg': ar}}
            K = int(maps_top)
            if K:
                j = out['lists']['frame_to_audio']['index'][:, :K]
                have = np.flatnonzero(j.reshape(-1) >= 0)
                tm = np.full((n * K,) + m.shape[1:], np.nan, np.float32)
                tp, ta = np.full(n * K, -np.inf, np.float32), np.full(n * K, -1, np.int32)
                if len(have):
                    tm[have], tp[have], ta[have] = scorer.maps(np.repeat(idx, K)[have], j.reshape(-1)[have], peaks=True)
                out['maps']['top'] = {'map': tm.reshape((n, K) + m.shape[1:]), 'peak': tp.reshape(n, K), 'arg': ta.reshape(n, K)}
    finally:
        if scorer is not None:
            scorer.close()
        V.close()
        A.close()
    return (out, rv, ra) if return_ranks else out
