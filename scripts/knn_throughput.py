"""Device time of the nearest-neighbour top-k pass of csrc/knn.hip at the sizes a user runs: the framewise US8K job
(30 000 queries x 240 000 rows of 512 floats) and the widest embedding (8 000 x 64 000 x 6144), at k = 5 and 50.  Times are
l3_knn_time's: hipEvents around back-to-back passes (every segment's lists and their merge) on resident rows, one untimed pass
first.  The rate counts the 2 nq nc D flops of the dot products alone and is given as a share of the 157.3 TFLOP/s fp32 MFMA peak,
which bounds this kernel (the rows are read from HBM once per tile row: far from the bandwidth bound).  The matrix kernel over an
8192 x 8192 block is timed beside it: the same accumulation with the distances stored instead of selected from.
--torch runs the same job with torch.matmul over row chunks of the queries plus torch.topk on the same GPU (torch's own streams
and events); that run also produces the matrix chunks the kernel avoids.  --check compares the lists of the first and last
--check queries with NumPy on those rows of the matrix.  The kinds are timed in turn, --rounds times over, so a drift of the clock
shows as a spread between rounds.  One JSON line per (shape, k, round).

    python scripts/knn_throughput.py [--shapes 30000x240000x512 8000x64000x6144] [--ks 5 50] [--reps 3] [--rounds 2] [--torch] [--check 64]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

PEAK_TFLOPS = 157.3          # fp32 MFMA, MI355X


def rows(rng, n, D):
    return rng.standard_normal((n, D), dtype=np.float32)


def torch_pass(torch, Q, X, xx, k, chunk):
    """squared Euclidean top-k by matmul over row chunks: -> ms of one pass (events on the current stream)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for lo in range(0, Q.shape[0], chunk):
        q = Q[lo:lo + chunk]
        d = (q * q).sum(1, keepdim=True) + xx[None, :] - 2.0 * torch.matmul(q, X.T)
        torch.topk(d, k, dim=1, largest=False, sorted=True)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['30000x240000x512', '8000x64000x6144'])
    ap.add_argument('--ks', type=int, nargs='+', default=[5, 50])
    ap.add_argument('--metric', default='sqeuclidean')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--chunk-bytes', type=int, default=1 << 30)
    ap.add_argument('--check', type=int, default=0)
    args = ap.parse_args()
    if args.torch:
        import torch          # before libl3hip: one HIP runtime in the process
    from l3embedding_amd import _lib
    for shape in args.shapes:
        nq, nc, D = (int(v) for v in shape.split('x'))
        rng = np.random.default_rng(nq + D)
        Q, X = rows(rng, nq, D), rows(rng, nc, D)
        h = _lib.KNN(D, args.metric)
        h.set_database(X)
        h.set_queries(Q)
        flops = 2.0 * nq * nc * D
        if args.check:
            import knn_ref
            for k in args.ks:
                idx, dist = h.topk(k)
                ok = True
                for lo in (0, nq - args.check):
                    widx, wdist = knn_ref.topk_ref(h.matrix(lo, lo + args.check, 0, nc), k)
                    ok = ok and np.array_equal(idx[lo:lo + args.check], widx) and np.array_equal(dist[lo:lo + args.check], wdist)
                print(json.dumps(dict(shape=shape, k=k, check_rows=2 * args.check, lists_equal_numpy=bool(ok))), flush=True)
        if args.torch:
            tq, tx = torch.from_numpy(Q).cuda(), torch.from_numpy(X).cuda()
            txx = (tx * tx).sum(1)
            chunk = max(1, args.chunk_bytes // (4 * nc))
        for rnd in range(args.rounds):
            bq, bc = min(nq, 8192), min(nc, 8192)
            ms = h.time('matrix', reps=args.reps)
            print(json.dumps(dict(shape=shape, round=rnd, kind='matrix_block', block='%dx%d' % (bq, bc), ms=round(ms, 3),
                                  tflops=round(2.0 * bq * bc * D / ms * 1e-9, 2))), flush=True)
            for k in args.ks:
                ms = h.time('topk', k=k, reps=args.reps)
                rec = dict(shape=shape, round=rnd, kind='topk', k=k, ms=round(ms, 3), tflops=round(flops / ms * 1e-9, 2),
                           share_of_fp32_mfma_peak=round(flops / ms * 1e-9 / PEAK_TFLOPS, 4))
                if args.torch:
                    if rnd == 0:
                        torch_pass(torch, tq, tx, txx, k, chunk)          # warm-up: rocBLAS picks its kernels
                    tms = torch_pass(torch, tq, tx, txx, k, chunk)
                    rec.update(torch_matmul_topk_ms=round(tms, 3), torch_chunk_rows=chunk, torch_over_kernel=round(tms / ms, 3))
                print(json.dumps(rec), flush=True)
        h.close()
        if args.torch:
            del tq, tx, txx
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
