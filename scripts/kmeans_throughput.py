"""Device time of the k-means kernels of csrc/kmeans.hip at the sizes a user runs: the framewise US8K job (240 000 rows
of 512 floats) at K = 10, 50 and 1024 and the widest embedding (30 000 rows of 6144 floats) at K = 256.  Times are l3_kmeans_time's:
hipEvents around back-to-back rounds on resident rows, one untimed round first.  Per job: the assignment kernel, the update (run
sums, finish, norms), the sort by label, the inertia, one whole iteration and a k-means++ seeding of all K centres.

  assignment   2 n K' D flops with K' = K rounded up to the 128-centroid tile (what the matrix cores execute) and 2 n K D useful ones:
               their ratio is the padding cost at small K
  update       the bytes of rows it reads once, n D 4, per second, beside the 5.2 TB/s the streaming kernels reach
               (profiles/r06_traffic_by_layer.txt)
  knn route    what the library offered before: l3_knn_topk at k = 1 with the centroids as database (l3_knn_time what 0), the same
               bits.  --knn-route-only times nothing else, so the script also runs on a checkout that has no k-means.
  --torch      torch.matmul in row chunks + argmin + index_add_ on the same GPU for one whole iteration (torch's own events)

One JSON line per (job, round).

    python scripts/kmeans_throughput.py [--jobs 240000x512x10 ...] [--reps 3] [--rounds 2] [--torch] [--knn-route-only]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

STREAM_TBS = 5.2          # profiles/r06_traffic_by_layer.txt
TILE = 128


def torch_iteration(torch, X, xx, C, chunk):
    """one Lloyd iteration in torch: distances by matmul over row chunks, argmin, index_add_ of the rows, division -> (ms, new C)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    cc = (C * C).sum(1)
    labels = torch.empty(X.shape[0], dtype=torch.int64, device=X.device)
    for lo in range(0, X.shape[0], chunk):
        d = xx[lo:lo + chunk, None] + cc[None, :] - 2.0 * torch.matmul(X[lo:lo + chunk], C.T)
        labels[lo:lo + chunk] = torch.argmin(d, dim=1)
    sums = torch.zeros_like(C).index_add_(0, labels, X)
    counts = torch.bincount(labels, minlength=C.shape[0]).to(C.dtype)
    new = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1.0)[:, None], C)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', nargs='+', default=['240000x512x10', '240000x512x50', '240000x512x1024', '30000x6144x256'])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--chunk-rows', type=int, default=65536)
    ap.add_argument('--knn-route-only', action='store_true')
    args = ap.parse_args()
    if args.torch:
        import torch          # before libl3hip: one HIP runtime in the process
    from l3embedding_amd import _lib
    last = None
    for job in args.jobs:
        n, D, K = (int(v) for v in job.split('x'))
        if last != (n, D):
            X = np.random.default_rng(n + D).standard_normal((n, D), dtype=np.float32)
            last = (n, D)
        seeds = np.random.RandomState(K).permutation(n)[:K].astype(np.int64)
        knn = _lib.KNN(D, 'sqeuclidean')
        knn.set_database(X[seeds])
        knn.set_queries(X)
        if not args.knn_route_only:
            h = _lib.KMeans(D, K)
            h.set_rows(X)
            h.seed_rows(seeds)
        if args.torch:
            tx = torch.from_numpy(X).cuda()
            txx = (tx * tx).sum(1)
            tc = tx[torch.from_numpy(seeds).cuda()].clone()
            torch_iteration(torch, tx, txx, tc, args.chunk_rows)          # warm-up: rocBLAS picks its kernels
        padded = (K + TILE - 1) // TILE * TILE
        for rnd in range(args.rounds):
            rec = dict(job=job, round=rnd, knn_topk1_ms=round(knn.time('topk', k=1, reps=args.reps), 3))
            if not args.knn_route_only:
                t = {what: h.time(what, reps=args.reps) for what in ('assign', 'update', 'sort', 'inertia', 'iteration')}
                t['seed'] = h.time('seed', reps=1)
                h.seed_rows(seeds)
                rec.update({'%s_ms' % k: round(v, 3) for k, v in t.items()})
                rec.update(assign_executed_tflops=round(2.0 * n * padded * D / t['assign'] * 1e-9, 2),
                           assign_useful_tflops=round(2.0 * n * K * D / t['assign'] * 1e-9, 2), padding_factor=round(padded / K, 2),
                           assign_over_knn_topk1=round(t['assign'] / rec['knn_topk1_ms'], 3),
                           update_rows_tbs=round(4.0 * n * D / t['update'] * 1e-9, 3),
                           update_share_of_streaming=round(4.0 * n * D / t['update'] * 1e-9 / STREAM_TBS, 3),
                           seed_ms_per_centre=round(t['seed'] / max(1, K - 1), 4))
            if args.torch:
                tms, _ = torch_iteration(torch, tx, txx, tc, args.chunk_rows)
                rec.update(torch_iteration_ms=round(tms, 3))
                if not args.knn_route_only:
                    rec.update(torch_over_iteration=round(tms / t['iteration'], 3))
            print(json.dumps(rec), flush=True)
        knn.close()
        if not args.knn_route_only:
            h.close()
        if args.torch:
            del tx, txx, tc
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
