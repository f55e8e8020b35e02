"""Writes tests/golden/svm_*.npz: sklearn.svm.SVC results on small synthetic sets, the fixtures of tests/test_svm_host.py and
tests/test_svm_gpu.py.  Generated with scikit-learn 1.7.2 (recorded in each file as `sklearn_version`); gamma='auto' is passed
explicitly because 1.7.2's default ('scale') differs from 0.19's ('auto' = 1 / n_features).  1.7.2's SVC follows 0.19's for
everything recorded here: libsvm's C-SVC, ovo decision values, the ovr transform, predict_proba.

Each set records, per kernel: the ovo and ovr decision values of the test rows, predict, predict_proba, dual_coef_, support_,
intercept_, probA_, probB_, the calibration distance: the largest difference of the ovo decision values between a fit at the
fixture's tol and one at tol / 100 (how far sklearn's own answer moves with the stopping tolerance), and the probability spread:
the largest difference of predict_proba between this fit and six with other random_state values (other cross-validation folds).

    python tests/golden/make_svm_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20240611
TOL = 1e-3


def clusters(rs, n_classes, n_train, n_test, D, spread=1.6):
    """Gaussian class clusters that overlap, so that every pair keeps bounded and free support vectors"""
    centres = rs.randn(n_classes, D) * spread / np.sqrt(D) * 3.0
    y = np.arange(n_train + n_test) % n_classes
    rs.shuffle(y)
    X = centres[y] + rs.randn(y.size, D)
    X = (X / np.sqrt(D) * 4.0).astype(np.float32)
    return X[:n_train], y[:n_train].astype(np.int32), X[n_train:], y[n_train:].astype(np.int32)


def fit_record(X, y, Xt, kernel, C, tol, degree=3, coef0=0.0):
    from sklearn.svm import SVC
    common = dict(C=C, kernel=kernel, degree=degree, gamma='auto', coef0=coef0, probability=True, random_state=SEED,
                  cache_size=500)
    m = SVC(tol=tol, decision_function_shape='ovo', **common).fit(X.astype(np.float64), y)
    tight = SVC(tol=tol / 100, decision_function_shape='ovo', **common).fit(X.astype(np.float64), y)
    Xt64 = Xt.astype(np.float64)
    ovo, ovo_tight = m.decision_function(Xt64), tight.decision_function(Xt64)
    m.decision_function_shape = 'ovr'
    rec = dict(ovo=ovo, ovo_tight=ovo_tight, ovr=m.decision_function(Xt64), predict=m.predict(Xt64),
               proba=m.predict_proba(Xt64), dual_coef=m.dual_coef_, support=m.support_.astype(np.int32),
               n_support=m.n_support_.astype(np.int32), intercept=m.intercept_, probA=m.probA_, probB=m.probB_,
               calib=float(np.max(np.abs(ovo - ovo_tight))), C=C, tol=tol, degree=degree, coef0=coef0)
    # how far other cross-validation folds move sklearn's own probabilities (libsvm draws them from rand())
    others = [SVC(tol=tol, **dict(common, random_state=s)).fit(X.astype(np.float64), y).predict_proba(Xt64) for s in range(6)]
    rec['proba_spread'] = float(max(np.max(np.abs(q - rec['proba'])) for q in others))
    return rec


def write(name, X, y, Xt, yt, kernels, C):
    import sklearn
    out = dict(X=X, y=y, Xt=Xt, yt=yt, kernels=np.array(kernels), sklearn_version=sklearn.__version__)
    for k in kernels:
        rec = fit_record(X, y, Xt, k, C, TOL, coef0=0.0 if k != 'poly' else 1.0)
        for key, v in rec.items():
            out['%s_%s' % (k, key)] = np.asarray(v)
        print('%s %s: %d SVs, calibration distance %.3g, probability spread %.3g' % (name, k, rec['support'].size, rec['calib'],
                                                                                      rec['proba_spread']))
    path = os.path.join(HERE, 'svm_%s.npz' % name)
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


def main():
    rs = np.random.RandomState(SEED)
    write('c4', *clusters(rs, 4, 800, 300, 64), kernels=['linear', 'poly', 'rbf', 'sigmoid'], C=1.0)
    write('c2', *clusters(rs, 2, 300, 120, 16), kernels=['rbf', 'linear'], C=10.0)
    write('c12', *clusters(rs, 12, 480, 120, 32), kernels=['rbf'], C=1.0)


if __name__ == '__main__':
    main()
