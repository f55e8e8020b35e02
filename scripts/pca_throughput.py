"""Device time of the principal-component kernels of csrc/pca.hip at the sizes a user runs: the framewise US8K set
(240 000 rows of 512 floats) and the widest embedding (60 000 x 6144).  Times are l3_pca_time's: hipEvents around back-to-back rounds
on resident rows, one untimed round first.  The scatter's rate is given twice: over the flops the matrix cores issue (U tiles of 128 x
128 on or above the diagonal, 2 * 128 * 128 * n each: the lower halves of the diagonal tiles and the padding of a ragged D are issued
too) and over the n D (D + 1) flops of the entries that are needed; the projection's over its 2 n D k.  Both as a share of the 157.3
TFLOP/s fp32 MFMA peak.  The nearest-neighbour matrix kernel over an 8192 x 8192 block of the same rows is timed beside them as the
yardstick of a like tile (profiles/r35_knn.txt).  --eigh times numpy.linalg.eigh on the host at those widths (a random symmetric
matrix; no GPU), --fit the wall time of a whole PCA.fit from host rows.  One JSON line per measurement.

    python scripts/pca_throughput.py [--shapes 240000x512 60000x6144] [--ks 64 256] [--reps 3] [--rounds 2] [--eigh 512] [--fit]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PEAK_TFLOPS = 157.3          # fp32 MFMA, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='*', default=['240000x512', '60000x6144'])
    ap.add_argument('--ks', type=int, nargs='+', default=[64, 256])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--eigh', type=int, nargs='*', default=[])
    ap.add_argument('--fit', action='store_true')
    args = ap.parse_args()
    for D in args.eigh:
        rng = np.random.default_rng(D)
        A = rng.standard_normal((D, D))
        t0 = time.perf_counter()
        np.linalg.eigh(A + A.T)
        print(json.dumps(dict(kind='host_eigh', D=D, seconds=round(time.perf_counter() - t0, 3))), flush=True)
    if not args.shapes:
        return
    from l3embedding_amd import _lib, pca
    for shape in args.shapes:
        n, D = (int(v) for v in shape.split('x'))
        rng = np.random.default_rng(n + D)
        X = rng.standard_normal((n, D), dtype=np.float32)
        X += 1.0
        h = _lib.PCA(D)
        h.set_rows(X)
        m64, m32 = h.mean()
        T = -(-D // 128)
        tiles = T * (T + 1) // 2
        issued, needed = 2.0 * 128 * 128 * n * tiles, float(n) * D * (D + 1)
        S = h.scatter()
        col = np.zeros(D)
        for lo in range(0, n, 16384):          # trace(S) against a float64 pass over the rows: a sanity check at the size timed
            xc = (X[lo:lo + 16384] - m32[None, :]).astype(np.float64)
            col += np.einsum('ij,ij->j', xc, xc)
        print(json.dumps(dict(shape=shape, kind='check', splits=_lib.pca_splits(n, D), symmetric=bool(np.array_equal(S, S.T)),
                              diag_rel_err=float(np.max(np.abs(np.diag(S) - col) / col)))), flush=True)
        del S
        knn = _lib.KNN(D, 'sqeuclidean')
        block = min(n, 8192)
        knn.set_database(X[:block])
        knn.set_queries(X[:block])
        for rnd in range(args.rounds):
            ms = knn.time('matrix', reps=args.reps)
            print(json.dumps(dict(shape=shape, round=rnd, kind='knn_matrix_block', block='%dx%d' % (block, block), ms=round(ms, 3),
                                  tflops=round(2.0 * block * block * D / ms * 1e-9, 2))), flush=True)
            print(json.dumps(dict(shape=shape, round=rnd, kind='mean', ms=round(h.time('mean', reps=args.reps), 3))), flush=True)
            for kind in ('scatter', 'scatter_tiles'):
                ms = h.time(kind, reps=args.reps)
                print(json.dumps(dict(shape=shape, round=rnd, kind=kind, tiles=tiles, ms=round(ms, 3), issued_tflops=round(issued / ms * 1e-9, 2),
                                      needed_tflops=round(needed / ms * 1e-9, 2),
                                      issued_share_of_fp32_mfma_peak=round(issued / ms * 1e-9 / PEAK_TFLOPS, 4))), flush=True)
            for k in args.ks:
                W = np.ascontiguousarray(rng.standard_normal((k, D), dtype=np.float32) / np.float32(np.sqrt(D)))
                h.set_model(m32, W)
                ms = h.time('transform', reps=args.reps)
                flops = 2.0 * n * D * k
                print(json.dumps(dict(shape=shape, round=rnd, kind='transform', k=k, ms=round(ms, 3), tflops=round(flops / ms * 1e-9, 2),
                                      share_of_fp32_mfma_peak=round(flops / ms * 1e-9 / PEAK_TFLOPS, 4))), flush=True)
        knn.close()
        h.close()
        if args.fit and D <= 1024:
            model = pca.PCA(50)
            t0 = time.perf_counter()
            model.fit(X)
            print(json.dumps(dict(shape=shape, kind='fit_wall', n_components=50, seconds=round(time.perf_counter() - t0, 3))), flush=True)
            model.close()
        del X


if __name__ == '__main__':
    main()
