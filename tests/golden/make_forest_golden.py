"""Writes tests/golden/forest_*.npz: sklearn.ensemble.RandomForestClassifier's test accuracy on small synthetic sets over several
seeds, the fixtures of tests/test_forest_host.py and tests/test_forest_gpu.py.  Generated with scikit-learn 1.7.2 (recorded in each
file as `sklearn_version`); its defaults are 0.19's for everything train_rf (classifier/train.py:169-227) leaves at its default: Gini,
bootstrap, max_features sqrt(D) ('sqrt' now, 'auto' then), trees grown out.

The histogram forest of l3embedding_amd.forest cannot reproduce sklearn's trees (forest.py's header), so it is judged against
sklearn's own spread from seed to seed: each set records `sklearn_accuracy`, the test accuracy of N_SEEDS fits that differ only in
random_state, and the tests ask for an accuracy of at least mean - 3 std of those.

Two sets: `gauss`, the overlapping Gaussian class clusters of make_svm_golden.py, and `relu`, the same shifted and clipped at zero so
that about 80 % of the entries are exact zeros, as pooled ReLU embeddings are: most candidate cuts of a column then fall on one value.

    python tests/golden/make_forest_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20240923
N_SEEDS = 8
N_TREES = 40


def clusters(rs, n_classes, n_train, n_test, D, spread=1.6):
    """make_svm_golden.py's Gaussian class clusters"""
    centres = rs.randn(n_classes, D) * spread / np.sqrt(D) * 3.0
    y = np.arange(n_train + n_test) % n_classes
    rs.shuffle(y)
    X = centres[y] + rs.randn(y.size, D)
    X = (X / np.sqrt(D) * 4.0).astype(np.float32)
    return X[:n_train], y[:n_train].astype(np.int32), X[n_train:], y[n_train:].astype(np.int32)


def shifted_and_clipped(X, Xt, zeros=0.8):
    """max(x - q, 0) with q the `zeros` quantile of the training entries"""
    q = np.float32(np.quantile(X, zeros))
    return np.maximum(X - q, np.float32(0)), np.maximum(Xt - q, np.float32(0))


def write(name, X, y, Xt, yt):
    import sklearn
    from sklearn.ensemble import RandomForestClassifier
    acc = np.array([(RandomForestClassifier(n_estimators=N_TREES, random_state=s).fit(X, y).predict(Xt) == yt).mean()
                    for s in range(N_SEEDS)])
    out = dict(X=X, y=y, Xt=Xt, yt=yt, n_estimators=N_TREES, sklearn_accuracy=acc, sklearn_version=sklearn.__version__,
               zero_fraction=float((X == 0).mean()))
    path = os.path.join(HERE, 'forest_%s.npz' % name)
    np.savez_compressed(path, **out)
    print('%s: sklearn accuracy %.4f +- %.4f over %d seeds (bar %.4f), %.0f %% zeros; wrote %s (%d bytes)' % (
        name, acc.mean(), acc.std(), N_SEEDS, acc.mean() - 3 * acc.std(), 100 * out['zero_fraction'], path, os.path.getsize(path)))


def main():
    rs = np.random.RandomState(SEED)
    X, y, Xt, yt = clusters(rs, 10, 800, 400, 64)
    write('gauss', X, y, Xt, yt)
    Xc, Xtc = shifted_and_clipped(X, Xt)
    write('relu', Xc, y, Xtc, yt)


if __name__ == '__main__':
    main()
