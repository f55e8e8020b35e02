"""Fit and predict times of the random forest (l3embedding_amd.forest) at synthetic US8K-fold shapes: 200 000 x 512
(framewise) and 8 000 x 3584 (stats), 10 overlapping Gaussian classes, 100 trees; per level the nodes searched, those of them searched
by the wide kernel, and the wall time.  `sklearn_<shape> [trees]` times sklearn's RandomForestClassifier(n_jobs=16) on the same data.
The record is profiles/r22_forest.txt.

    python scripts/forest_throughput.py {framewise|stats|sklearn_framewise|sklearn_stats} [trees]
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np

SHAPES = {'framewise': (200000, 512), 'stats': (8000, 3584)}

def data(n, D, C=10, seed=0):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, C, n)
    X = rs.standard_normal((n, D)).astype(np.float32)
    X += (rs.standard_normal((C, D)).astype(np.float32) * np.float32(0.35))[y]
    return X, y

what = sys.argv[1]
shape = what.replace('sklearn_', '')
n, D = SHAPES[shape]
t0 = time.time(); X, y = data(n, D); print('%s: data %d x %d in %.1f s' % (what, n, D, time.time() - t0), flush=True)
if what.startswith('sklearn'):
    import sklearn
    from sklearn.ensemble import RandomForestClassifier as SK
    trees = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    t0 = time.time(); m = SK(n_estimators=trees, n_jobs=16, random_state=0).fit(X, y); dt = time.time() - t0
    t0 = time.time(); m.predict_proba(X[:20000]); dp = time.time() - t0
    print('sklearn %s n_jobs=16: fit of %d trees %.2f s, predict_proba of %d rows %.3f s, nodes per tree %.0f, depth %d' % (
        sklearn.__version__, trees, dt, min(n, 20000), dp, np.mean([e.tree_.node_count for e in m.estimators_]),
        max(e.tree_.max_depth for e in m.estimators_)), flush=True)
    sys.exit(0)

from l3embedding_amd.forest import RandomForestClassifier, tree_seeds, bootstrap_counts
t0 = time.time(); seeds = tree_seeds(0, 100); boot = bootstrap_counts(seeds, n); print('host draws (seeds, bootstrap) %.3f s' % (time.time() - t0))
RandomForestClassifier(n_estimators=2, random_state=0).fit(X[:2000], y[:2000])          # load the library, warm the kernels
for wide_min in ([0] if shape == 'framewise' else [0, 33, 17]):
    m = RandomForestClassifier(n_estimators=100, random_state=0, wide_min_rows=wide_min)
    t0 = time.time(); m.fit(X, y); dt = time.time() - t0
    nodes, wide, ms = m.level_stats_
    print('fit of 100 trees, wide_min_rows %d: %.3f s wall (levels %.3f s), %d levels, %d nodes (%.0f per tree)' % (
        wide_min or 65, dt, ms.sum() / 1e3, nodes.size, m.estimators_['left'].size, m.estimators_['left'].size / 100.0), flush=True)
    print('level: nodes searched, of them wide, ms')
    for i in range(nodes.size):
        print('  %3d %9d %8d %9.3f' % (i, nodes[i], wide[i], ms[i]))
    probe = X[:20000] if n >= 20000 else X
    m.predict_proba(probe[:100])
    t0 = time.time(); p = m.predict_proba(probe); dp = time.time() - t0
    print('predict_proba of %d rows: %.3f s; train accuracy on them %.4f' % (probe.shape[0], dp, (p.argmax(1) == y[:probe.shape[0]]).mean()), flush=True)
