"""Wall times of RandomForestClassifier.oob_evaluate(FITTED_ROWS) beside evaluate(FITTED_ROWS) on one forest of 100
trees scored at the sizes 25 / 50 / 100, at forest_throughput.py's synthetic US8K-fold shapes (8 000 x 3584 stats, 200 000 x 512
framewise, 10 overlapping Gaussian classes).  Host clock around calls that end in a device synchronise, one run per figure after one
warm-up call of each at a single size; the out-of-bag call's time includes the host's redraw of the bootstrap multiplicities, which
is also timed alone.  The record is profiles/r26_forest_oob.txt.

    python scripts/forest_oob_throughput.py {stats|framewise} [trees] [sizes ...]
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np

from forest_search_throughput import CLASSES, SHAPES, data


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in SHAPES:
        raise SystemExit(__doc__)
    shape = sys.argv[1]
    trees = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    sizes = [int(a) for a in sys.argv[3:]] or [trees // 4, trees // 2, trees]
    from l3embedding_amd import forest
    from l3embedding_amd.forest import FITTED_ROWS, RandomForestClassifier
    n, D = SHAPES[shape]
    X, y = data(n, D)
    RandomForestClassifier(n_estimators=2, random_state=0).fit(X[:2000], y[:2000]).oob_evaluate(y=y[:2000])      # load the library, warm
    t0 = time.time(); m = RandomForestClassifier(n_estimators=trees, random_state=0).fit(X, y); fit = time.time() - t0
    m.evaluate(FITTED_ROWS, y=y, outputs=('predict', 'correct')), m.oob_evaluate(y=y, outputs=('predict', 'correct'))
    t0 = time.time(); inside = m.evaluate(FITTED_ROWS, y=y, prefixes=sizes, outputs=('predict', 'correct')); t_eval = time.time() - t0
    t0 = time.time(); outside = m.oob_evaluate(y=y, prefixes=sizes, outputs=('predict', 'correct')); t_oob = time.time() - t0
    t0 = time.time(); forest.bootstrap_counts(forest.tree_seeds(0, trees), n); t_draw = time.time() - t0
    t0 = time.time(); m.oob_evaluate(prefixes=sizes, outputs=('sums', 'n_oob')); t_sums = time.time() - t0
    print('%s: %d rows x %d, %d classes, %d trees (%d nodes) fitted in %.3f s; sizes %s' % (shape, n, D, CLASSES, trees, m.estimators_['left'].size,
                                                                                          fit, sizes))
    print('  evaluate(FITTED_ROWS) predict + correct          %.4f s   training accuracy %s' % (t_eval, [round(float(c) / n, 4) for c in inside['correct']]))
    print('  oob_evaluate(FITTED_ROWS) predict + correct      %.4f s   out-of-bag accuracy %s' % (t_oob, [round(float(c) / n, 4) for c in outside['correct']]))
    print('    of it the host\'s redraw of the multiplicities   %.4f s (timed alone)' % t_draw)
    print('  oob_evaluate(FITTED_ROWS) sums + n_oob           %.4f s' % t_sums)


if __name__ == '__main__':
    main()
