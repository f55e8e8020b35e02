"""Device time of the sound localisation maps of csrc/locmap.hip: n frames of H x W image locations queried by n
seconds, head 128 -- the list mode over the diagonal (maps and peaks stored), the peaks mode over every (frame, second) pair and the
rank mode's counting pass.  Times are l3_pairs_map_time's: hipEvents around back-to-back launches on the resident map and query set,
one untimed launch first; the kinds are timed in turn, --rounds times over.  Beside them two yardsticks:

  model    the lane-operation model of profiles/r32_pair_scores.txt: 2.5 head lane operations per (location, query) pair at 16384
           lane operations per clock, and the pair kernel's own measured 0.5527 ms per 8192 x 8192 pairs scaled by the pair count
  before   the only route to the same numbers without these kernels: the location rows set as items (l3_pairs_set_vision_dev),
           l3_pairs_matrix in blocks to the host, NumPy max there.  Run on --before-frames frames (wall time, scaled to n for the
           record) and compared bit for bit with the peaks mode on those frames.

    python scripts/locmap_throughput.py [--items 1024] [--hw 28 28] [--reps 20] [--rounds 3] [--before-frames 32] [--chunk 64]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from l3embedding_amd import _lib  # noqa: E402

PAIR_MS_8192 = 0.5527          # profiles/r32_pair_scores.txt: margins of 8192 x 8192 pairs, H = 128, sclk 2381 MHz
LANE_OPS_PER_S = 16384 * 2381e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=1024)
    ap.add_argument('--hw', type=int, nargs=2, default=[28, 28])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--before-frames', type=int, default=32)
    ap.add_argument('--chunk', type=int, default=64)
    args = ap.parse_args()
    n, (H, W), head, C = args.items, args.hw, 128, 512
    L = H * W
    rng = np.random.RandomState(0)
    p = _lib.Pairs(C, C, head)
    p.set_head((rng.randn(2 * C, head) / np.sqrt(2 * C)).astype(np.float32), rng.randn(head).astype(np.float32),
               rng.randn(head, 2).astype(np.float32), rng.randn(2).astype(np.float32))
    p.set_audio(rng.randn(n, C).astype(np.float32))
    p.map_reserve(0, n, H, W)
    first = None
    t0 = time.time()
    for i0 in range(0, n, args.chunk):
        cnt = min(args.chunk, n - i0)
        f = _lib.Features(np.abs(rng.standard_normal((cnt * L, C)).astype(np.float32)))          # post-ReLU activations are >= 0
        p.map_put(f, 0, i0, cnt)
        if first is None:
            first = f
        else:
            f.close()
    print(json.dumps(dict(items=n, H=H, W=W, head=head, map_MB=n * L * head * 4 / 1e6, raw_locations_MB=n * L * C * 4 / 1e6,
                          put_wall_s=time.time() - t0, project_chunk_ms=p.time('project_vision', n_rows=min(args.chunk, n) * L, reps=10))), flush=True)
    pairs = float(n) * n * L
    tiles = -(-L // 64) * 64
    model = dict(lane_op_floor_ms=1e3 * pairs * 2.5 * head / LANE_OPS_PER_S, pair_kernel_scaled_ms=PAIR_MS_8192 * pairs / 8192.0 ** 2,
                 pair_kernel_scaled_whole_tiles_ms=PAIR_MS_8192 * float(n) * n * tiles / 8192.0 ** 2)
    print(json.dumps(dict(model=model)), flush=True)
    p.map_time('peaks', reps=2)          # the clock settles
    for r in range(args.rounds):
        rec = dict(round=r, reps=args.reps)
        for what in ('list', 'peaks', 'ranks'):
            rec[what + '_ms'] = p.map_time(what, reps=args.reps if what != 'list' else 10 * args.reps)
        rec['peaks_over_pair_kernel_scaled'] = rec['peaks_ms'] / model['pair_kernel_scaled_ms']
        print(json.dumps(rec), flush=True)
    # the route before: location rows as items, the matrix in blocks to the host, NumPy max
    nb = min(args.before_frames, n, args.chunk)
    t0 = time.time()
    S, arg = p.map_peaks(0, nb, 0, n)
    t_new = time.time() - t0
    t0 = time.time()
    p.set_vision(first, 0, nb * L)
    t_set = time.time() - t0
    Sb, Ab = np.empty((nb, n), np.float32), np.empty((nb, n), np.int32)
    rows = max(1, (256 << 20) // (4 * n) // L) * L          # whole frames a block
    for v0 in range(0, nb * L, rows):
        v1 = min(nb * L, v0 + rows)
        M = p.matrix(v0, v1, 0, n).reshape((v1 - v0) // L, L, n)
        Sb[v0 // L:v1 // L], Ab[v0 // L:v1 // L] = M.max(axis=1), M.argmax(axis=1)
    t_before = time.time() - t0
    same = bool(np.array_equal(S.view(np.uint32), Sb.view(np.uint32)) and np.array_equal(arg, Ab))
    print(json.dumps(dict(before_frames=nb, before_wall_s=t_before, of_which_projection_s=t_set, before_scaled_to_all_s=t_before * n / nb,
                          floats_to_host=nb * L * n, peaks_call_wall_s=t_new, same_bits_and_args=same)), flush=True)
    first.close()
    p.close()


if __name__ == '__main__':
    main()
