"""Times of the random forest's one-pass parameter search over n_estimators (classifier.train_rf_search) against the
loop of train_rf over the same grid, at forest_throughput.py's synthetic US8K-fold shapes (200 000 x 512 framewise, 8 000 x 3584
stats, 10 overlapping Gaussian classes) with a 20 000-row validation part and a 20 008-row test part in files of 41 rows, and of
RandomForestClassifier.evaluate against predict_proba on the same rows and trees.  Host clock around calls that end in a device
synchronise; the two sides alternate in one process after a warm-up of each.  The record is profiles/r23_forest_search.txt.

    python scripts/forest_search_throughput.py search {framewise|stats} [repeats] [grid ...]     (a) search against loop
    python scripts/forest_search_throughput.py evaluate {framewise|stats} [trees]                (b) evaluate against predict_proba
    python scripts/forest_search_throughput.py once {framewise|stats} [grid ...]                 one search, for rocprofv3 --kernel-trace
"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np

SHAPES = {'framewise': (200000, 512), 'stats': (8000, 3584)}
N_VALID, N_TEST, FILE_ROWS, CLASSES = 20000, 20008, 41, 10


def data(n, D, C=CLASSES, seed=0):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, C, n)
    X = rs.standard_normal((n, D)).astype(np.float32)
    X += (rs.standard_normal((C, D)).astype(np.float32) * np.float32(0.35))[y]
    return X, y


def splits(shape):
    n, D = SHAPES[shape]
    X, y = data(n + N_VALID + N_TEST, D)
    starts = np.arange(0, N_TEST, FILE_ROWS)
    files = np.stack((starts, starts + FILE_ROWS), axis=1)
    test_y = y[n + N_VALID:][starts]          # a file's class: its first row's
    return (dict(features=X[:n], labels=y[:n]), dict(features=X[n:n + N_VALID], labels=y[n:n + N_VALID]),
            dict(features=X[n + N_VALID:], labels=test_y, file_idxs=files))


def spread(times):
    return 'min %.3f  median %.3f  max %.3f s over %d runs' % (min(times), float(np.median(times)), max(times), len(times))


def main():
    what, shape = sys.argv[1], sys.argv[2]
    from l3embedding_amd import classifier
    from l3embedding_amd.forest import FITTED_ROWS, RandomForestClassifier
    t0 = time.time()
    train, valid, test = splits(shape)
    print('%s %s: data %d + %d + %d rows x %d in %.1f s' % (what, shape, len(train['labels']), N_VALID, N_TEST, SHAPES[shape][1], time.time() - t0),
          flush=True)
    out = tempfile.mkdtemp()
    RandomForestClassifier(n_estimators=2, random_state=0).fit(train['features'][:2000], train['labels'][:2000]).evaluate(
        train['features'][:2000])          # load the library, warm the kernels

    def search(grid):
        return classifier.train_rf_search(train, valid, test, out, n_estimators_grid=grid, num_classes=CLASSES, random_state=0)

    def loop(grid):
        return classifier.train_param_search(train, valid, test, out, train_func=classifier.train_rf, search_space={'n_estimators': list(grid)},
                                             train_with_valid=False, num_classes=CLASSES, random_state=0)

    if what == 'once':
        grid = [int(a) for a in sys.argv[3:]] or [100, 500, 1000]
        t0 = time.time(); got = search(grid); print('one search over %s: %.3f s, chosen %s' % (grid, time.time() - t0, got[2]['search_params_best_values']))
    elif what == 'search':
        repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
        grid = [int(a) for a in sys.argv[4:]] or [100, 500, 1000]
        small = [max(1, g // 50) for g in grid]
        small = sorted(set(small))
        search(small), loop(small)          # a warm-up of each
        times = {'search': [], 'loop': []}
        for r in range(repeats):
            for name, run in (('search', search), ('loop', loop)):
                t0 = time.time(); got = run(grid); times[name].append(time.time() - t0)
                print('  run %d %-6s %.3f s  valid accuracy %s  chosen %s' % (r, name, times[name][-1], [round(float(got[2]['search'][(g,)]['accuracy']), 4) for g in grid],
                                                                              got[2]['search_params_best_values']), flush=True)
        for name in ('search', 'loop'):
            print('%-6s over %s: %s' % (name, grid, spread(times[name])))
        print('search / loop (medians): %.3f' % (np.median(times['search']) / np.median(times['loop'])))
    elif what == 'evaluate':
        trees = int(sys.argv[3]) if len(sys.argv) > 3 else 100
        m = RandomForestClassifier(n_estimators=trees, random_state=0).fit(train['features'], train['labels'])
        nodes = m.estimators_['left'].size
        leaves = int((m.estimators_['left'] < 0).sum())
        probe = valid['features']
        m.predict_proba(probe[:256]), m.evaluate(probe[:256], outputs=('proba',))
        rows = {'predict_proba': [], 'evaluate proba': [], 'evaluate predict': [], 'evaluate predict at 3 sizes': []}
        sizes = sorted({max(1, trees // 10), max(1, trees // 2), trees})
        for r in range(5):
            t0 = time.time(); a = m.predict_proba(probe); rows['predict_proba'].append(time.time() - t0)
            t0 = time.time(); b = m.evaluate(probe, outputs=('proba',))['proba'][0]; rows['evaluate proba'].append(time.time() - t0)
            t0 = time.time(); m.evaluate(probe); rows['evaluate predict'].append(time.time() - t0)
            t0 = time.time(); m.evaluate(probe, prefixes=sizes); rows['evaluate predict at 3 sizes'].append(time.time() - t0)
            assert np.array_equal(a, b)
        t0 = time.time(); m.evaluate(FITTED_ROWS); fitted = time.time() - t0
        print('%d trees, %d nodes (%d leaves); %d rows scored (wall, upload and download included):' % (trees, nodes, leaves, len(probe)))
        for k, v in rows.items():
            print('  %-28s %s' % (k, spread(v)))
        print('  evaluate predict of the %d fitted rows, resident: %.3f s' % (len(train['labels']), fitted))
        # the depth of the walks: node gathers per (row, tree), counted on the host for 256 rows
        depth = walk_depth(m.estimators_, probe[:256])
        print('  node gathers per (row, tree), leaf included: mean %.2f, max %d' % (depth.mean(), depth.max()))
    else:
        raise SystemExit(__doc__)


def walk_depth(f, X):
    """(rows, trees) the nodes a row reads in each tree, its leaf included"""
    n, off = len(X), f['tree_off']
    out = np.zeros((n, off.size - 1), np.int64)
    at = np.arange(n)
    for t in range(off.size - 1):
        node = np.full(n, off[t], np.int64)
        while True:
            out[:, t] += 1
            left = f['left'][node]
            inner = left >= 0
            if not inner.any():
                break
            out[~inner, t] -= 1
            feat = np.where(inner, f['feature'][node], 0)
            node = np.where(inner, off[t] + np.where(X[at, feat] <= f['threshold'][node], left, f['right'][node]), node)
    return out


if __name__ == '__main__':
    main()
