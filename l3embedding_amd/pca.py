"""Principal components of a frozen embedding on the GPU: fit, projection, whitening and the way back.

`PCA.fit` computes the column means and the scatter matrix S = sum of xc xc^T of the centred rows on the device (csrc/pca.hip: float64
sums in one fixed order for the mean, the fp32 matrix cores in chains of 256 rows folded into float64 for S), then
`numpy.linalg.eigh(S / (n - 1))` on the host in float64 (`solver='full'`, the default).  That step is on the host on purpose: at D = 512
it takes hundredths of a second and is as exact as LAPACK.  For D = 6144 it takes many seconds, and `solver='subspace'` instead finds
the k leading pairs by block subspace iteration on S where it lies (eigen.py over csrc/eig.hip's float64 matrix-core products; only
m x m problems, m = k + oversample, go to the host).  A fit is a function of its rows alone (and of `random_state` for the subspace
solver): there are no float atomics and the split of the rows does not depend on the device, so two fits give the same bits on any
GPU.

`transform` centres at `mean_` and projects onto `components_` with the dot product of the nearest-neighbour kernels (one ascending
float32 fused-multiply-add chain over D per entry), times `1 / sqrt(explained_variance_)` when whitening.  With `to_device=True` the
result is a `usc.DeviceFeatures`, which `knn.NearestNeighbors`, `cluster.KMeans`, `tsne.TSNE` and the classifiers take as it is.  Rows
are float32 NumPy arrays or `usc.DeviceFeatures`; there is no silent conversion and no CPU fallback.
"""
import numpy as np

from . import _lib, eigen as _eigen
from .knn import _rows
from .usc import DeviceFeatures

BLOCK = 65536          # host rows of one block of transform() / inverse_transform()
SOLVERS = ('full', 'subspace', 'auto')
# solver='auto' takes the subspace solver from this many features on (and k + oversample <= D // 4).  profiles/r39_pca_subspace.txt has
# the crossover table this is read from: the smallest D of {512, 1024, 2048, 4096, 6144} at which the subspace fit at k = 64 was faster
# than the full one in the same run.
AUTO_MIN_D = 1024


def sign_rule(components):
    """each row of `components` (k, D) with the sign that makes its entry of largest magnitude positive, the lowest index among equal
    magnitudes; a row of zeros stays as it is"""
    w = np.array(components, copy=True)
    for c in range(w.shape[0]):
        if w[c, int(np.argmax(np.abs(w[c])))] < 0:          # (argmax gives the first among equals)
            w[c] = -w[c]
    return w


def eigen(covariance):
    """(variances (D) float64 descending, negative round-off clipped to 0; components (D, D) float64, row c the c-th axis under the
    sign rule) of a symmetric float64 matrix, by numpy.linalg.eigh"""
    lam, vec = np.linalg.eigh(covariance)
    order = np.argsort(-lam, kind='stable')
    return np.maximum(lam[order], 0.0), sign_rule(vec[:, order].T)


def count_for(ratio, share):
    """the fewest leading components whose variance ratios sum to at least `share`"""
    return int(min(len(ratio), np.searchsorted(np.cumsum(ratio), share, side='left') + 1))


def check_n_components(n_components):
    if n_components is None:
        return None
    if isinstance(n_components, bool):
        raise ValueError('n_components must be None, an integer >= 1 or a fraction in (0, 1), not %r' % (n_components,))
    if isinstance(n_components, (int, np.integer)):
        if n_components < 1:
            raise ValueError('n_components must be at least 1, not %d' % n_components)
        return int(n_components)
    if isinstance(n_components, (float, np.floating)) and 0.0 < n_components < 1.0:
        return float(n_components)
    raise ValueError('n_components must be None, an integer >= 1 or a fraction in (0, 1), not %r' % (n_components,))


class PCA(object):
    """Principal component analysis on the GPU.  n_components: None (every one of the D axes is kept), an integer k <= D, or a fraction in (0, 1): the fewest leading components whose explained variance ratios sum to it.  whiten: the
    projections are divided by the components' standard deviations (a kept component of zero variance is refused).  solver: 'full'
    (numpy.linalg.eigh of the whole covariance on the host), 'subspace' (the n_components leading pairs by block subspace iteration on
    the device: an integer n_components, block width n_components + oversample, residuals below tol times the largest eigenvalue within
    max_iter products or eigen.NotConverged, the start drawn from random_state) or 'auto' (the rule of solver_for)."""

    def __init__(self, n_components=None, whiten=False, device=0, keep_covariance=False, solver='full', oversample=None, tol=1e-9, max_iter=500,
                 random_state=0):
        self.n_components = check_n_components(n_components)
        self.whiten, self.device, self.keep_covariance = bool(whiten), int(device), bool(keep_covariance)
        if solver not in SOLVERS:
            raise ValueError('solver must be one of %s, not %r' % (SOLVERS, solver))
        if solver == 'subspace' and not isinstance(self.n_components, int):
            raise ValueError("solver='subspace' needs an integer n_components, not %r: how many components a share of the variance takes "
                             "is not known without the whole spectrum (use solver='full')" % (n_components,))
        if oversample is not None and (isinstance(oversample, bool) or not isinstance(oversample, (int, np.integer)) or oversample < 0):
            raise ValueError('oversample must be None or an integer >= 0, not %r' % (oversample,))
        if not tol > 0.0 or isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
            raise ValueError('tol must be positive and max_iter an integer >= 1, not %r and %r' % (tol, max_iter))
        self.solver, self.oversample = solver, None if oversample is None else int(oversample)
        self.tol, self.max_iter, self.random_state = float(tol), int(max_iter), random_state
        self.solver_info_ = None
        self.components_ = None
        self._h = None

    @classmethod
    def from_arrays(cls, mean, components, explained_variance=None, whiten=False, device=0):
        """a fitted model of given arrays (read from a file): mean (D) and components (k, D) float32; whitening needs the k
        variances"""
        m, w = np.asarray(mean), np.asarray(components)
        if m.dtype != np.float32 or w.dtype != np.float32:
            raise ValueError('mean and components must be float32 (there is no silent conversion), not %s and %s' % (m.dtype, w.dtype))
        if w.ndim != 2 or m.ndim != 1 or w.shape[1] != m.shape[0] or not 1 <= w.shape[0] <= w.shape[1]:
            raise ValueError('need mean (D) and components (1 <= k <= D, D), not %s and %s' % (m.shape, w.shape))
        self = cls(int(w.shape[0]), whiten=whiten, device=device)
        self.mean_, self.components_ = np.ascontiguousarray(m), np.ascontiguousarray(w)
        self.explained_variance_ = self.explained_variance_ratio_ = None
        self.n_components_ = int(w.shape[0])
        self.n_samples_ = None
        if explained_variance is not None:
            ev = np.asarray(explained_variance, np.float64).reshape(-1)
            if ev.shape != (w.shape[0],):
                raise ValueError('explained_variance must hold %d entries, not %d' % (w.shape[0], ev.size))
            self.explained_variance_ = ev
        self.scale_ = self._scale()
        return self

    def _scale(self):
        """float32(1 / sqrt(variance)) of the kept components when whitening, else None"""
        if not self.whiten:
            return None
        if self.explained_variance_ is None:
            raise ValueError('whiten=True needs the explained variances of the components')
        ev = self.explained_variance_[:self.n_components_]
        zero = np.flatnonzero(~(ev > 0.0))
        if zero.size:
            raise ValueError('whiten=True: component %d has the explained variance %r, and a division by its square root is not defined '
                             '(keep fewer components)' % (int(zero[0]), float(ev[zero[0]])))
        return (1.0 / np.sqrt(ev)).astype(np.float32)

    # ---- the device handle ----
    def close(self):
        """frees the device copy of the fitted rows and the model; the next call uploads the model again"""
        if getattr(self, '_h', None) is not None:
            self._h.close()
            self._h = None

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_h'] = None          # a model is pickled with its arrays, not with device memory
        return state

    def __setstate__(self, state):
        # (a model pickled before there was a choice of solver has none of these: it behaves as 'full')
        self.__dict__.update(dict(solver='full', oversample=None, tol=1e-9, max_iter=500, random_state=0, solver_info_=None))
        self.__dict__.update(state)

    def solver_for(self, D):
        """the solver a fit of rows of D features takes: 'auto' is 'subspace' when n_components is an integer, n_components + oversample
        <= min(D // 4, the library's widest block) and D >= AUTO_MIN_D, and 'full' otherwise"""
        if self.solver != 'auto':
            return self.solver
        if not isinstance(self.n_components, int) or D < AUTO_MIN_D:
            return 'full'
        oversample = _eigen.default_oversample(self.n_components) if self.oversample is None else self.oversample
        return 'subspace' if self.n_components + oversample <= min(D // 4, _lib.EIG_MAX_M) else 'full'

    def _check_fitted(self):
        if self.components_ is None:
            raise ValueError('fit comes first')

    def _handle(self):
        """the l3_pca handle with the model resident; rebuilt on first use after unpickling or close()"""
        self._check_fitted()
        if self._h is None:
            h = _lib.PCA(self.components_.shape[1], device=self.device)
            try:
                h.set_model(self.mean_, self.components_, self.scale_)
            except Exception:
                h.close()
                raise
            self._h = h
        return self._h

    def _finish(self, n, mean32, S):
        """the model from the scatter matrix S of n rows about mean32: the host's part of a fit"""
        D = S.shape[0]
        covariance = S / float(n - 1)
        variance, axes = eigen(covariance)
        total = float(variance.sum())
        ratio = variance / total if total > 0.0 else np.zeros_like(variance)
        if self.n_components is None:
            k = D
        elif isinstance(self.n_components, float):
            k = count_for(ratio, self.n_components)
        else:
            k = self.n_components
            if k > D:
                raise ValueError('n_components = %d, but the rows have only %d features' % (k, D))
        self.n_components_, self.n_samples_ = k, int(n)
        self.mean_ = mean32
        self.explained_variance_, self.explained_variance_ratio_ = variance[:k], ratio[:k]
        self.scale_ = self._scale()          # (refuses before the components are set: a refused fit leaves no model)
        self.components_ = np.ascontiguousarray(axes[:k].astype(np.float32))
        if self.keep_covariance:
            self.covariance_ = covariance

    def _finish_subspace(self, n, mean32, h, m):
        """the model from the scatter matrix that the handle h holds on the device, by block subspace iteration of width m: the k
        leading eigenpairs, and the total variance from the trace"""
        k = self.n_components
        eig = _lib.Eig(h.D, m, device=self.device)
        try:
            eig.set_matrix_pca(h)
            theta, vectors, info = _eigen.top_eigh(eig, k, oversample=m - k, tol=self.tol, max_iter=self.max_iter, random_state=self.random_state)
            trace = eig.trace()
        finally:
            eig.close()
        variance = np.maximum(theta / float(n - 1), 0.0)
        total = trace / float(n - 1)
        ratio = variance / total if total > 0.0 else np.zeros_like(variance)
        self.n_components_, self.n_samples_ = k, int(n)
        self.mean_ = mean32
        self.explained_variance_, self.explained_variance_ratio_ = variance, ratio
        self.solver_info_ = info
        self.scale_ = self._scale()          # (refuses before the components are set: a refused fit leaves no model)
        self.components_ = np.ascontiguousarray(sign_rule(vectors).astype(np.float32))

    def fit(self, X):
        """X: (n >= 2, D) float32 rows or a usc.DeviceFeatures.  The rows stay on the device until close()."""
        rows = _rows(X, 'X')
        n, D = rows.shape
        if n < 2:
            raise ValueError('principal components need at least 2 rows, not %d' % n)
        if isinstance(self.n_components, int) and self.n_components > D:
            raise ValueError('n_components = %d, but the rows have only %d features' % (self.n_components, D))
        subspace = self.solver_for(D) == 'subspace'
        m = _eigen.block_width(self.n_components, self.oversample, D) if subspace else None          # (refused before the device)
        if subspace and m > _lib.EIG_MAX_M:
            raise ValueError('k + oversample = %d exceeds the %d vectors of a block of the subspace solver (use the full solver)' % (m, _lib.EIG_MAX_M))
        self.close()
        self.components_ = None
        self.solver_info_ = None
        h = _lib.PCA(D, device=self.device)
        try:
            h.set_rows(rows)
            _, mean32 = h.mean()
            if subspace:
                S = h.scatter(download=self.keep_covariance)
                self._finish_subspace(n, mean32, h, m)
                if self.keep_covariance:
                    self.covariance_ = S / float(n - 1)
            else:
                S = h.scatter()
                self._finish(n, mean32, S)
            h.set_model(self.mean_, self.components_, self.scale_)
        except Exception:
            h.close()
            self.components_ = None
            raise
        self._h = h
        return self

    def _other(self, X, what, width):
        rows = _rows(X, what)
        if rows.shape[1] != width:
            raise ValueError('%s has %d features per row; expecting %d' % (what, rows.shape[1], width))
        return rows

    def _project(self, X, what, to_device, forward):
        self._check_fitted()
        rows = self._other(X, what, self.components_.shape[1] if forward else self.components_.shape[0])
        if to_device and not isinstance(rows, _lib.Features):
            raise ValueError('to_device=True needs %s on the device (a usc.DeviceFeatures)' % what)
        h = self._handle()
        call = h.transform if forward else h.inverse
        if isinstance(rows, _lib.Features):
            got = call(rows, to_device=to_device)
            return DeviceFeatures.from_handle(got) if to_device else got
        return np.concatenate([call(rows[lo:lo + BLOCK]) for lo in range(0, rows.shape[0], BLOCK)])

    def transform(self, X, to_device=False):
        """(n, n_components_) float32: the rows centred at mean_ and projected onto components_ (whitened when whiten).  With
        to_device (X a usc.DeviceFeatures) a new DeviceFeatures on the same GPU, which the caller closes, and no host copy."""
        return self._project(X, 'X', to_device, True)

    def fit_transform(self, X, to_device=False):
        return self.fit(X).transform(X, to_device=to_device)

    def inverse_transform(self, Y, to_device=False):
        """(n, D) float32: the rows of the input space that the projections Y (n, n_components_) stand for"""
        return self._project(Y, 'Y', to_device, False)
