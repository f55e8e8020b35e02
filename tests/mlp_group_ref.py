"""Stand-ins for _lib.MLP and _lib.MLPGroup without a GPU, built on the float64 step of tests/mlp_ref.py, and the small data sets
of the group tests (tests/test_mlp_group_host.py, tests/test_mlp_group_gpu.py).  A group here is a list of the single models, so
that "the group equals the loop" on these stand-ins tests the driver around the handle (classifier.fit_mlp_grid /
train_mlp_search), not the kernels; keep_best stores float32 copies, as the device snapshot and the trip through model.h5 both do."""
import numpy as np

import mlp_ref as ref
from l3embedding_amd import _lib


class RefMLP(object):
    """_lib.MLP in float64 NumPy: Glorot weights from the seed, mlp_ref.epoch per epoch"""

    def __init__(self, D, C, batch, weight_decay=1e-5, seed=0, device=0):
        self.D, self.C, self.batch, self.weight_decay = int(D), int(C), int(batch), float(weight_decay)
        rs = np.random.RandomState(int(seed) % (2 ** 32))
        self.W = []
        for shape in _lib.mlp_shapes(self.D, self.C):
            limit = np.sqrt(6.0 / sum(shape)) if len(shape) == 2 else 0.0
            self.W.append(rs.uniform(-1, 1, shape) * limit)
        self.W = [w.astype(np.float32).astype(np.float64) for w in self.W]
        self.m = [np.zeros_like(w) for w in self.W]
        self.v = [np.zeros_like(w) for w in self.W]
        self.n_train = self.n_valid = 0

    def set_data(self, X, y, Xv=None, yv=None):
        self.X, self.y = np.asarray(X, np.float64), np.asarray(y, np.int64)
        self.Xv = None if Xv is None or len(Xv) == 0 else np.asarray(Xv, np.float64)
        self.yv = None if self.Xv is None else np.asarray(yv, np.int64)
        self.n_train, self.n_valid = len(self.X), 0 if self.Xv is None else len(self.Xv)

    def epoch(self, perm, lr, t0):
        lr = float(np.float32(lr))
        self.W, stats = ref.epoch(self.W, self.m, self.v, self.X, self.y, np.asarray(perm), lr, t0, self.batch,
                                  float(np.float32(self.weight_decay)), self.Xv, self.yv)
        return dict(loss=float(stats['loss']), acc=float(stats['acc']), val_loss=float(stats.get('val_loss', np.nan)),
                    val_acc=float(stats.get('val_acc', np.nan)))

    def predict(self, X):
        _, _, z = ref.forward(self.W, np.asarray(X, np.float64))
        return ref.softmax(z).astype(np.float32)

    def get_weights(self):
        return [w.astype(np.float32) for w in self.W]

    def set_weights(self, weights):
        self.W = [np.asarray(w, np.float32).astype(np.float64) for w in weights]

    def close(self):
        pass


def make_group(single):
    """the _lib.MLPGroup made of `single` handles (a class with _lib.MLP's interface), one per member"""

    class Group(object):
        made = []          # every group constructed, for the tests to look at

        def __init__(self, D, num_classes, batch, weight_decays, seeds, device=0):
            if not 1 <= len(weight_decays) <= _lib.MLP_MAX_MEMBERS or len(seeds) != len(weight_decays):
                raise ValueError('1 to 16 members, a seed each')
            self.members = [single(D, num_classes, batch, weight_decay=w, seed=s, device=device) for w, s in zip(weight_decays, seeds)]
            self.n_members, self.kept, self.uploads, self.epochs_run = len(self.members), {}, 0, []
            Group.made.append(self)

        def set_data(self, X, y, Xv=None, yv=None):
            self.uploads += 1
            self.X, self.Xv = np.asarray(X), None if Xv is None else np.asarray(Xv)
            for m in self.members:
                m.set_data(X, y, Xv, yv)
            self.n_train, self.n_valid = len(X), 0 if Xv is None else len(Xv)

        def epoch(self, perm, lrs, t0, live=None):
            live = [True] * self.n_members if live is None else list(live)
            self.epochs_run.append(live)
            nan = dict(loss=np.nan, acc=np.nan, val_loss=np.nan, val_acc=np.nan)
            return [m.epoch(perm, lr, t0) if alive else dict(nan) for m, lr, alive in zip(self.members, lrs, live)]

        def keep_best(self, members):
            for i in members:
                self.kept[i] = self.members[i].get_weights()

        def restore_best(self, members):
            for i in members:
                self.members[i].set_weights(self.kept[i])

        def predict(self, X):
            return np.stack([m.predict(X) for m in self.members])

        def predict_resident(self, valid=False):
            return self.predict(self.Xv if valid else self.X)

        def get_weights(self, member):
            return self.members[member].get_weights()

        def close(self):
            pass

    return Group


def clusters(D=600, C=10, n=500, nv=70, nt=90, seed=3, spread=1.5):
    """Gaussian class clusters -> (X, y, Xv, yv, Xt, yt), float32 rows and int32 labels"""
    r = np.random.RandomState(seed)
    centers = r.randn(C, D) * spread
    out = []
    for count in (n, nv, nt):
        y = r.randint(0, C, count).astype(np.int32)
        out += [(centers[y] + r.randn(count, D)).astype(np.float32), y]
    return tuple(out)


def splits(D=600, C=10, n=500, nv=70, files=9, frames=10, seed=3, spread=1.5):
    """(train, valid, test) as usc.get_split gives them: the test split has file_idxs and one label per file"""
    X, y, Xv, yv, Xt, _ = clusters(D, C, n, nv, files * frames, seed, spread)
    file_labels = np.arange(files) % C
    r = np.random.RandomState(seed + 1)
    centers = np.random.RandomState(seed).randn(C, D) * spread
    Xt = (centers[np.repeat(file_labels, frames)] + r.randn(files * frames, D)).astype(np.float32)
    return ({'features': X, 'labels': y}, {'features': Xv, 'labels': yv},
            {'features': Xt, 'labels': file_labels, 'file_idxs': [(i * frames, (i + 1) * frames) for i in range(files)]})


def same(a, b):
    """deep equality of metrics: dicts, lists, tuples, arrays and numbers, NaN equal to NaN, floats bit for bit"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, str) or a is None:
        return a == b
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'))
