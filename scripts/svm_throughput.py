"""Seconds per fit of the SVM classifier (classifier/train.py:79-166; l3embedding_amd/svm.py, csrc/svm.hip) on a synthetic
UrbanSound8K-shaped set: 10 classes of heavily overlapping Gaussian clusters (--overlap 0.04: nearly every row is a support
vector of some pair; sklearn takes 7.9 s at 5 000 rows, D = 512), RBF kernel, gamma 'auto', C = 1.  For each (D, rows):
SVC.fit without and with probability estimates, the outer iterations and local SMO updates per one-vs-one problem, and (--cpu-max rows and
below, when scikit-learn is installed) sklearn's SVC on the CPU with the same settings, for the speed-up.  One JSON line each.
Per-launch times: run a short configuration under `rocprofv3 --kernel-trace --stats`; the kernel-row launch's fraction of the
fp32 matrix-core peak follows from its time and 2 q n_p D flops per problem and outer iteration (kernel_row_flops_per_outer in the output).

    python scripts/svm_throughput.py [--widths 512 6144] [--rows 5000 10000] [--tol 1e-3] [--cpu-max 10000] [--no-proba]

--grid: the parameter search's grid over C instead (classifier/train.py:607-616), for each (D, rows) and --classes: seconds of one
svm.fit_grid over --costs with probability estimates (--platt device | host), seconds of one SVC(probability=True).fit per cost
(--grid-separate; on its own this also runs on a tree that has no fit_grid), and the launches and host waits of both counted from
what each path calls: a solver call is 4 launches and one wait per outer iteration of its slowest problem, a held-out decision
call 2 launches (1 in the grid's) and one wait, a device sigmoid fit one launch and one wait.

    python scripts/svm_throughput.py --grid [--grid-separate] --widths 512 --rows 200000 --classes 10 [--costs 0.1 1 10 100 1000]
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
from l3embedding_amd import svm as svm_module  # noqa: E402
from l3embedding_amd.svm import SVC  # noqa: E402


def synthetic(n, D, C=10, seed=0, overlap=0.04):
    r = np.random.RandomState(seed)
    centres = r.randn(C, D) * overlap
    y = np.arange(n) % C
    r.shuffle(y)
    X = (centres[y] + r.randn(n, D) / np.sqrt(D) * 2.5).astype(np.float32)
    return X, y.astype(np.int32)


def grid(args):
    """one JSON line per (D, rows): the grid over C in one pass and, with --grid-separate, one fit per cost"""
    for D in args.widths:
        for n in args.rows:
            X, y = synthetic(n, D, C=args.classes, overlap=args.overlap)
            P = args.classes * (args.classes - 1) // 2
            rec = dict(D=D, rows=n, classes=args.classes, kernel='rbf', tol=args.tol, ws=args.ws or 64, costs=args.costs)
            SVC(C=1.0, gamma='auto', tol=args.tol, ws_size=args.ws).fit(X[:256], y[:256])     # warm-up: handle, code objects
            params = dict(gamma='auto', tol=args.tol, probability=True, random_state=0, ws_size=args.ws)
            if args.grid_separate:
                t = time.perf_counter()
                models = [SVC(C=c, **params).fit(X, y) for c in args.costs]
                rec['separate_fits_s'] = time.perf_counter() - t
                outer = [int(m.n_outer_.max()) for m in models]
                # per fit: the solver (its sub-problems may run longer than the pairs counted here: a lower bound), then one
                # decision call (2 launches, one wait) per cross-validation sub-problem
                rec['separate_launches_min'] = sum(4 * o + 1 for o in outer) + 2 * 5 * P * len(models)
                rec['separate_host_waits_min'] = sum(o + 1 for o in outer) + 5 * P * len(models)
            if hasattr(svm_module, 'fit_grid'):
                svm_module.fit_grid(X[:256], y[:256], args.costs, platt=args.platt, **params)           # warm-up of the new launches
                t = time.perf_counter()
                models = svm_module.fit_grid(X, y, args.costs, platt=args.platt, max_entries=args.max_entries, **params)
                rec['fit_grid_s'] = time.perf_counter() - t
                rec['platt'] = args.platt
                outer = max(int(m.n_outer_.max()) for m in models)
                rec['grid_launches_min'] = 4 * outer + 1 + 1 + (1 if args.platt == 'device' else 0)
                rec['grid_host_waits_min'] = outer + 1 + 1 + (1 if args.platt == 'device' else 0)
                rec['outer_max_pairs'] = outer
                rec['n_support'] = [int(m.support_.size) for m in models]
            print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--widths', type=int, nargs='+', default=[512, 6144])
    ap.add_argument('--rows', type=int, nargs='+', default=[5000, 10000])
    ap.add_argument('--tol', type=float, default=1e-3)
    ap.add_argument('--ws', type=int, default=0, help='working-set size q (0: the library default)')
    ap.add_argument('--cpu-max', type=int, default=10000)
    ap.add_argument('--no-proba', action='store_true')
    ap.add_argument('--overlap', type=float, default=0.04, help='spread of the class centres (smaller: harder)')
    ap.add_argument('--grid', action='store_true', help='time the grid over C (svm.fit_grid) instead')
    ap.add_argument('--grid-separate', action='store_true', help='with --grid: also one SVC(probability=True).fit per cost')
    ap.add_argument('--costs', type=float, nargs='+', default=[0.1, 1, 10, 100, 1000])
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--platt', default='device', choices=['device', 'host'])
    ap.add_argument('--max-entries', type=int, default=None, help="fit_grid's budget on the rows of one solver call")
    args = ap.parse_args()
    if args.grid:
        return grid(args)
    for D in args.widths:
        for n in args.rows:
            X, y = synthetic(n, D, overlap=args.overlap)
            rec = dict(D=D, rows=n, classes=10, kernel='rbf', tol=args.tol, ws=args.ws or 64)
            m = SVC(C=1.0, gamma='auto', tol=args.tol, ws_size=args.ws).fit(X[:256], y[:256])     # warm-up: handle, code objects
            t = time.perf_counter()
            m = SVC(C=1.0, gamma='auto', tol=args.tol, ws_size=args.ws).fit(X, y)
            rec['gpu_fit_s'] = time.perf_counter() - t
            rec['outer_per_problem'] = [int(m.n_outer_.min()), float(m.n_outer_.mean()), int(m.n_outer_.max())]
            rec['updates_per_problem'] = [int(m.n_iter_.min()), float(m.n_iter_.mean()), int(m.n_iter_.max())]
            rows_p = 2 * n / 10
            rec['kernel_row_flops_per_outer'] = 2.0 * rec['ws'] * rows_p * D * 45
            rec['n_support'] = int(m.support_.size)
            if not args.no_proba:
                t = time.perf_counter()
                mp = SVC(C=1.0, gamma='auto', tol=args.tol, probability=True, random_state=0, ws_size=args.ws).fit(X, y)
                rec['gpu_fit_proba_s'] = time.perf_counter() - t
                rec['outer_per_problem_proba'] = int(mp.n_outer_.max())
            if n <= args.cpu_max:
                try:
                    from sklearn.svm import SVC as SkSVC
                except ImportError:
                    SkSVC = None
                if SkSVC is not None:
                    t = time.perf_counter()
                    SkSVC(C=1.0, gamma='auto', tol=args.tol, cache_size=2000).fit(X.astype(np.float64), y)
                    rec['cpu_sklearn_fit_s'] = time.perf_counter() - t
                    rec['speedup'] = rec['cpu_sklearn_fit_s'] / rec['gpu_fit_s']
            print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
