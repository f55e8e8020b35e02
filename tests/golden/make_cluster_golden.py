"""Writes tests/golden/cluster_golden.npz: scikit-learn's scores and k-means inertias that tests/test_cluster_host.py compares with.
Run by hand where scikit-learn is installed (python tests/golden/make_cluster_golden.py); the tests read the file and never import
scikit-learn.  The version used is recorded in the file.

  pairs_a, pairs_b (10, 300)   ten pairs of labelings: equal, permuted, refined, independent, one-sided and wholly trivial ones
  nmi, ari (10)                normalized_mutual_info_score (arithmetic mean) and adjusted_rand_score of each pair
  blob_params (3, 4)           (K, D, rows per cluster, spread) of the blob fixtures of cluster_ref.blobs (seed 5)
  blob_inertia (3, 8)          KMeans(K, init='k-means++', n_init=1, algorithm='lloyd', random_state=s).fit(X).inertia_, s = 0 .. 7
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import KMeans
from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_ref as R  # noqa: E402

BLOBS = [(6, 16, 100, 2.0), (10, 32, 60, 3.0), (20, 24, 40, 2.5)]
N = 300


def label_pairs():
    rng = np.random.RandomState(11)
    base = rng.randint(0, 5, N)
    noisy = base.copy()
    flip = rng.rand(N) < 0.2
    noisy[flip] = rng.randint(0, 5, int(flip.sum()))
    pairs = [
        (base, base),                                        # equal
        (base, (base + 2) % 5),                              # the same partition under other names
        (base, base * 2 + rng.randint(0, 2, N)),             # a refinement
        (base, rng.randint(0, 5, N)),                        # independent
        (base, noisy),                                       # a fifth of the rows reassigned
        (base, np.zeros(N, np.int64)),                       # one side trivial
        (np.zeros(N, np.int64), np.zeros(N, np.int64)),      # both trivial
        (np.arange(N), base),                                # every row its own cluster
        (rng.randint(0, 12, N), rng.randint(0, 3, N)),       # unequal numbers of groups
        (np.repeat(np.arange(3), N // 3), np.repeat(np.arange(6), N // 6)),          # nested blocks
    ]
    return np.array([a for a, _ in pairs], np.int64), np.array([b for _, b in pairs], np.int64)


def main():
    a, b = label_pairs()
    nmi = np.array([normalized_mutual_info_score(y, x) for x, y in zip(a, b)], np.float64)
    ari = np.array([adjusted_rand_score(y, x) for x, y in zip(a, b)], np.float64)
    inertia = np.zeros((len(BLOBS), 8), np.float64)
    for f, (K, D, per, spread) in enumerate(BLOBS):
        X, _ = R.blobs(K, D, per, spread)
        for s in range(8):
            inertia[f, s] = KMeans(K, init='k-means++', n_init=1, algorithm='lloyd', random_state=s).fit(X.astype(np.float64)).inertia_
    out = os.path.join(HERE, 'cluster_golden.npz')
    np.savez(out, pairs_a=a, pairs_b=b, nmi=nmi, ari=ari, blob_params=np.array(BLOBS, np.float64), blob_inertia=inertia,
             sklearn_version=np.array(sklearn.__version__))
    print(out, sklearn.__version__)
    print(nmi, ari, inertia, sep='\n')


if __name__ == '__main__':
    main()
