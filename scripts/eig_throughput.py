"""Times of the top-k eigensolver (csrc/eig.hip, eigen.py, pca.PCA(solver='subspace')) at the sizes a user runs, beside the
full solver on the same rows in the same run.  Rows are embedding-like: max(0, N(0, 1) geomspace(4, 0.05, D) + 1) in float32.

Per shape n x D and k: the device time of apply, gram, mix and residual at m = k + oversample (l3_eig_time: hipEvents around
back-to-back rounds, one untimed round first); the float64 TFLOP/s the matrix cores ISSUE in apply (the padded tiles: 2 * 64 ceil(m /
64) * 64 ceil(D / 64) * 16 ceil(D / 16)) and the 2 m D^2 it needs; a whole PCA.fit with each solver (wall time from host rows, ending in
the model's upload, a device synchronise); and the eigen stage of the subspace fit split three ways: device (the calls of the
iteration times the device time of each), host (LAPACK and the control flow between the calls) and the rest of the time inside the
calls (transfers of the m x m matrices and the blocks, launches, synchronisation).  --crossover runs both solvers at k = 64 over a
list of widths on the same rows: the table pca.AUTO_MIN_D is read from.  One JSON line per measurement.

    python scripts/eig_throughput.py [--shapes 240000x512:50 60000x6144:50,256] [--crossover 512 1024 2048 4096 6144] [--rows 20000] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def rows_like_embeddings(n, D, seed):
    rng = np.random.default_rng(seed)
    scale = np.geomspace(4.0, 0.05, D).astype(np.float32)
    X = np.empty((n, D), np.float32)
    for lo in range(0, n, 8192):
        block = rng.standard_normal((min(n, lo + 8192) - lo, D), dtype=np.float32)
        np.maximum(block * scale + np.float32(1.0), np.float32(0.0), out=X[lo:lo + 8192])
    return X


def timed_fit(pca, X, k, solver):
    model = pca.PCA(k, solver=solver)
    t0 = time.perf_counter()
    model.fit(X)
    seconds = time.perf_counter() - t0
    out = (seconds, model.explained_variance_.copy(), model.solver_info_)
    model.close()
    return out


def stages(_lib, X, seconds_of):
    """wall time of the fit's stages before the eigensolver, on a handle of their own"""
    h = _lib.PCA(X.shape[1])
    t0 = time.perf_counter()
    h.set_rows(X)
    t1 = time.perf_counter()
    h.mean()
    t2 = time.perf_counter()
    h.scatter(download=False)
    t3 = time.perf_counter()
    seconds_of.update(upload_rows=round(t1 - t0, 4), mean=round(t2 - t1, 4), scatter_resident=round(t3 - t2, 4))
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='*', default=['240000x512:50', '60000x6144:50,256'])
    ap.add_argument('--crossover', type=int, nargs='*', default=[])
    ap.add_argument('--rows', type=int, default=20000, help='rows of the crossover table')
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    from l3embedding_amd import _lib, eigen, pca
    warm = rows_like_embeddings(600, 256, 0)          # code objects, the library's load, LAPACK's threads
    timed_fit(pca, warm, 8, 'subspace')
    timed_fit(pca, warm, 8, 'full')

    for spec in args.shapes:
        shape, ks = spec.split(':')
        n, D = (int(v) for v in shape.split('x'))
        X = rows_like_embeddings(n, D, n + D)
        full_seconds, full_var, _ = timed_fit(pca, X, max(int(k) for k in ks.split(',')), 'full')
        print(json.dumps(dict(shape=shape, kind='fit_full', seconds=round(full_seconds, 3))), flush=True)
        before = {}
        h = stages(_lib, X, before)
        print(json.dumps(dict(shape=shape, kind='stages_before_the_solver', seconds=before)), flush=True)
        for k in (int(v) for v in ks.split(',')):
            m = eigen.block_width(k, None, D)
            e = _lib.Eig(D, m)
            e.set_matrix_pca(h)
            e.set_block('V', np.random.default_rng(k).standard_normal((m, D)))
            e.apply()
            ms = {what: e.time(what, reps=args.reps) for what in _lib.EIG_TIMED}
            ms2 = {what: e.time(what, reps=args.reps) for what in _lib.EIG_TIMED}          # the same again: the spread
            e.close()
            pad = lambda v, t: -(-v // t) * t
            issued, needed = 2.0 * pad(m, 64) * pad(D, 64) * pad(D, 16), 2.0 * m * D * D
            print(json.dumps(dict(shape=shape, k=k, m=m, kind='device_ms', first={w: round(v, 4) for w, v in ms.items()},
                                  second={w: round(v, 4) for w, v in ms2.items()},
                                  apply_issued_f64_tflops=round(issued / ms['apply'] * 1e-9, 2), apply_needed_f64_tflops=round(needed / ms['apply'] * 1e-9, 2),
                                  apply_bytes_of_S_over_ms_TBps=round(8.0 * D * D * (pad(m, 64) // 64) / ms['apply'] * 1e-9, 3))), flush=True)
            for rnd in range(2):
                seconds, var, info = timed_fit(pca, X, k, 'subspace')
                calls = info['calls']
                device = (calls['apply'] * ms['apply'] + calls['gram'] * ms['gram'] + calls['mix'] * ms['mix'] + calls['residual'] * ms['residual']) * 1e-3
                print(json.dumps(dict(shape=shape, k=k, m=m, round=rnd, kind='fit_subspace', seconds=round(seconds, 3), products=info['products'],
                                      checks=info['checks'], refills=info['refills'], residual=float('%.3g' % info['residual']), calls=calls,
                                      eigen_stage_seconds=round(info['ops_seconds'] + info['host_seconds'], 4), device=round(device, 4),
                                      host_lapack=round(info['host_seconds'], 4), transfers_and_launches=round(info['ops_seconds'] - device, 4),
                                      full_over_subspace=round(full_seconds / seconds, 2),
                                      largest_relative_difference_of_variances=float('%.3g' % np.max(np.abs(var - full_var[:k]) / full_var[0])))), flush=True)
        h.close()
        del X

    for D in args.crossover:
        X = rows_like_embeddings(args.rows, D, D)
        row = dict(kind='crossover', D=D, rows=args.rows, k=64)
        for rnd in range(2):          # alternating: full, subspace, full, subspace
            row['full_%d' % rnd] = round(timed_fit(pca, X, 64, 'full')[0], 3)
            seconds, _, info = timed_fit(pca, X, 64, 'subspace')
            row['subspace_%d' % rnd], row['products'] = round(seconds, 3), info['products']
        row['subspace_faster'] = bool(max(row['subspace_0'], row['subspace_1']) < min(row['full_0'], row['full_1']))
        print(json.dumps(row), flush=True)
        del X


if __name__ == '__main__':
    main()
