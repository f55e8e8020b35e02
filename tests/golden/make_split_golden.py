"""Writes tests/golden/stratified_split.npz: sklearn's StratifiedShuffleSplit(n_splits=1, test_size=ratio, random_state=seed) on small
label vectors, the fixtures usc.stratified_shuffle_split is compared with index for index (tests/test_param_split_host.py).
Generated with scikit-learn 1.7.2 (recorded in the file as `sklearn_version`).

Per case k: case<k>_labels (class c repeated count_c times, shuffled by np.random.RandomState(1)), case<k>_ratio, case<k>_seed,
case<k>_train, case<k>_valid.  Per refusal k: refusal<k>_labels, refusal<k>_ratio, refusal<k>_message (sklearn's ValueError).

    python tests/golden/make_split_golden.py
"""
import os

import numpy as np
import sklearn
from sklearn.model_selection import StratifiedShuffleSplit

# (class counts, ratio, seeds)
CASES = [
    ((7, 5, 2), 0.15, (0, 11)),                       # 11 / 3 rows: one class is absent from the validation part
    ((40,) * 10, 0.15, (20171021, 3)),                # 340 / 60 rows
    ((3, 3, 3, 3), 0.34, (5, 6)),                     # 7 / 5 rows: equal remainders, so ties are drawn
    ((13, 2, 29, 6, 50), 0.15, (7, 8)),               # 85 / 15 rows
    ((2, 2), 0.5, (1, 2)),                            # 2 / 2 rows
]
REFUSALS = [
    ((4, 1, 4), 0.3),                                 # a class of one member
    ((2, 2, 2, 2), 0.15),                             # n_valid = ceil(1.2) = 2 < 4 classes
]


def labels_of(counts):
    y = np.repeat(np.arange(len(counts)), counts)
    return y[np.random.RandomState(1).permutation(y.size)]


def main():
    out = dict(sklearn_version=sklearn.__version__)
    k = 0
    for counts, ratio, seeds in CASES:
        y = labels_of(counts)
        for seed in seeds:
            splitter = StratifiedShuffleSplit(n_splits=1, test_size=ratio, random_state=seed)
            train, valid = next(splitter.split(np.zeros((y.size, 1)), y))
            out.update({'case%d_labels' % k: y, 'case%d_ratio' % k: ratio, 'case%d_seed' % k: seed,
                        'case%d_train' % k: train.astype(np.int64), 'case%d_valid' % k: valid.astype(np.int64)})
            print('case %d: counts %s ratio %s seed %d -> %d / %d rows, validation classes %s' % (
                k, counts, ratio, seed, train.size, valid.size, np.unique(y[valid]).tolist()))
            k += 1
    out['n_cases'] = k
    for k, (counts, ratio) in enumerate(REFUSALS):
        y = labels_of(counts)
        try:
            next(StratifiedShuffleSplit(n_splits=1, test_size=ratio, random_state=0).split(np.zeros((y.size, 1)), y))
        except ValueError as e:
            out.update({'refusal%d_labels' % k: y, 'refusal%d_ratio' % k: ratio, 'refusal%d_message' % k: str(e)})
            print('refusal %d: counts %s ratio %s -> %s' % (k, counts, ratio, e))
        else:
            raise SystemExit('sklearn accepted refusal case %d' % k)
    out['n_refusals'] = len(REFUSALS)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'stratified_split.npz')
    np.savez_compressed(path, **out)
    print('wrote', path)


if __name__ == '__main__':
    main()
