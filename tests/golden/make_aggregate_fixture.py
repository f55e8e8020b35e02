"""ref_aggregate.npz: the reference's own aggregate_metrics (classifier/metrics.py:49-78) on fold metrics of the kinds the classifiers
report -- scalars (accuracy, loss, average_class_accuracy) and a list per fold (class_accuracy) -- over 2, 5 and 10 folds; the
10-fold case has a class without examples in one fold (NaN), as compute_metrics reports it.

Run where the reference is checked out, at generation time only:

    python tests/golden/make_aggregate_fixture.py /path/to/reference

metrics.py is imported by path and executed unmodified (it needs only NumPy and logging); only the .npz travels.  Per case n:
`n<n>_in_<key>` holds the folds' values, stacked, and `n<n>_out_<key>` the seven statistics in the order of STATS.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STATS = ('mean', 'var', 'min', '25_%ile', '75_%ile', 'median', 'max')
KEYS = ('accuracy', 'loss', 'class_accuracy', 'average_class_accuracy')
FOLD_COUNTS = (2, 5, 10)


def fold_metrics(n, num_classes=10):
    r = np.random.RandomState(100 + n)
    folds = []
    for i in range(n):
        per_class = [float(v) for v in r.uniform(0.2, 1.0, size=num_classes)]
        if n == 10 and i == 3:
            per_class[7] = float('nan')
        folds.append({'accuracy': np.float64(r.uniform(0.5, 0.9)), 'loss': float(r.uniform(0.1, 2.0)), 'class_accuracy': per_class,
                      'average_class_accuracy': np.mean(per_class)})
    return folds


def main(reference):
    spec = importlib.util.spec_from_file_location('ref_classifier_metrics', os.path.join(reference, 'classifier', 'metrics.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for n in FOLD_COUNTS:
        folds = fold_metrics(n)
        with np.errstate(all='ignore'):
            aggregated = ref.aggregate_metrics(folds)
        assert tuple(aggregated) == KEYS
        for k in KEYS:
            out['n%d_in_%s' % (n, k)] = np.array([f[k] for f in folds], np.float64)
            out['n%d_out_%s' % (n, k)] = np.array([aggregated[k][s] for s in STATS], np.float64)
    np.savez(os.path.join(HERE, 'ref_aggregate.npz'), **out)


if __name__ == '__main__':
    main(sys.argv[1])
