"""Writes tests/golden/tsne_golden.npz: the KL divergences scikit-learn's t-SNE reaches on the quality fixtures of the t-SNE tests
(tests/tsne_ref.py `blobs`: three Gaussian blobs of 100 points in 16 dimensions, dataset seeds 1, 2, 3), from which the tests take
their bar on the library's final KL: mean + 3 std of `barnes_hut` over 8 seeds per dataset.  Run it where scikit-learn is installed:

    python tests/golden/make_tsne_golden.py

The tests read only the .npz.  Recorded per dataset: the 8 KL values of method='barnes_hut' (kl_barnes_hut), the 8 of method='exact'
(kl_exact, for the record), the 1-NN label accuracy of every map (acc_*), and the sum of the fixture's rows (x_sum), which pins the
fixture the values belong to."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import tsne_ref as R          # noqa: E402

DATASETS = (1, 2, 3)
SEEDS = tuple(range(8))
PERPLEXITY = 20.0


def main():
    import sklearn
    from sklearn.manifold import TSNE
    out = dict(datasets=np.array(DATASETS), seeds=np.array(SEEDS), perplexity=PERPLEXITY, sklearn_version=np.array(sklearn.__version__))
    for method in ('barnes_hut', 'exact'):
        kl, acc = np.zeros((len(DATASETS), len(SEEDS))), np.zeros((len(DATASETS), len(SEEDS)))
        for a, ds in enumerate(DATASETS):
            X, labels = R.blobs(ds)
            for b, seed in enumerate(SEEDS):
                model = TSNE(n_components=2, perplexity=PERPLEXITY, method=method, init='random', learning_rate='auto', random_state=seed)
                Y = model.fit_transform(X)
                kl[a, b], acc[a, b] = model.kl_divergence_, R.one_nn_accuracy(Y, labels)
            print(method, ds, kl[a].round(4), acc[a].min())
        out['kl_' + method], out['acc_' + method] = kl, acc
    out['x_sum'] = np.array([float(R.blobs(ds)[0].astype(np.float64).sum()) for ds in DATASETS])
    np.savez(os.path.join(HERE, 'tsne_golden.npz'), **out)


if __name__ == '__main__':
    main()
