"""Device time of the top-k lists of csrc/pairs.hip beside the rank mode, which runs the same accumulation and also
stores nothing: n x n pairs of random items, for each head width the rank mode, the top-k lists of both directions (the lists
kernel and the merge kernel of each: four launches) and the frames' merge kernel alone, at each k.  Times are l3_pairs_time's:
hipEvents around back-to-back launches on resident operands, one untimed launch first.  The kinds are timed in turn, --rounds
times over, so that a drift of the clock shows as a spread between the rounds and not as a difference between the kinds.  One JSON
line per (H, round).  --check compares the lists of the first and last --check rows of either direction with NumPy on those rows of
the matrix (diagonal truth, 4 items a clip), at the size that is timed.

    python scripts/pair_topk_throughput.py [--items 8192] [--heads 128 64] [--ks 10 64] [--reps 200] [--rounds 3] [--check 64]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

from l3embedding_amd import _lib  # noqa: E402

TILE, MIN_TILES = 64, 4          # topk_segments of csrc/pairs.hip, restated for the record only


def segments(nq, nc, k):
    qt, ct = -(-nq // TILE), -(-nc // TILE)
    return max(1, min(-(-(1024 if k <= 16 else 512) // qt), ct // MIN_TILES, ct, 256))


def scorer(n, H, seed=0):
    rng = np.random.RandomState(seed)
    nv, na = (360, 350) if H == 64 else (512, 512)
    p = _lib.Pairs(nv, na, H)
    p.set_head((rng.randn(nv + na, H) / np.sqrt(nv + na)).astype(np.float32), rng.randn(H).astype(np.float32),
               rng.randn(H, 2).astype(np.float32), rng.randn(2).astype(np.float32))
    p.set_vision(rng.randn(n, nv).astype(np.float32))
    p.set_audio(rng.randn(n, na).astype(np.float32))
    return p


def check(p, n, k, rows):
    from pairs_topk_ref import same_lists, topk_ref
    groups = (np.arange(n) // 4).astype(np.int32)
    diag = np.arange(n, dtype=np.int32)
    (iv, mv), (ia, ma) = p.topk(k, diag, diag, groups, groups)
    ok = True
    for lo in (0, n - rows):
        sl = slice(lo, lo + rows)
        ok = ok and same_lists((iv[sl], mv[sl]), topk_ref(p.matrix(lo, lo + rows, 0, n), k, diag[sl], groups[sl], groups))
        ok = ok and same_lists((ia[sl], ma[sl]), topk_ref(p.matrix(0, n, lo, lo + rows).T, k, diag[sl], groups[sl], groups))
    return bool(ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=8192)
    ap.add_argument('--heads', type=int, nargs='+', default=[128, 64])
    ap.add_argument('--ks', type=int, nargs='+', default=[10, 64])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--check', type=int, default=64, help='rows of either end and direction compared with NumPy; 0: none')
    args = ap.parse_args()
    n = args.items
    for H in args.heads:
        p = scorer(n, H)
        if args.check:
            print(json.dumps(dict(H=H, items=n, checked_rows=args.check, lists_equal_numpy={k: check(p, n, k, args.check) for k in args.ks})),
                  flush=True)
        p.time('ranks', reps=args.reps)          # the clock settles
        for r in range(args.rounds):
            rec = dict(H=H, items=n, round=r, reps=args.reps, segments={k: segments(n, n, k) for k in args.ks}, ranks_ms=p.time('ranks', reps=args.reps))
            for k in args.ks:
                rec['topk_both_k%d_ms' % k] = p.time('topk', k, reps=args.reps)
                rec['merge_one_k%d_ms' % k] = p.time('topk_merge', k, reps=args.reps)
                rec['topk_k%d_over_ranks' % k] = rec['topk_both_k%d_ms' % k] / rec['ranks_ms']
            print(json.dumps(rec), flush=True)
        p.close()


if __name__ == '__main__':
    main()
