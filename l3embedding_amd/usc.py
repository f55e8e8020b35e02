"""Fold reading and preprocessing of the downstream sound-classification sets (UrbanSound8K, ESC-50, DCASE 2013): the
reference's data/usc/folds.py:16-112 and data/usc/features.py:52-150,243-253, restated without scipy and sklearn.

Quirks kept on purpose:
  * feature files are read in `os.listdir` order, and `filenames` lists every file of the fold, skipped ones included;
  * the US8K augmented-file skip ('_' in the name) applies to the valid and test folds only: get_train_folds reads with
    augment=True;
  * the summary statistics are min, max, median, mean, var, skew, excess kurtosis (scipy.stats defaults, bias=True);
  * the scalers use sklearn's arithmetic: population variance, and a zero variance / zero range scales by 1;
  * the training rows are shuffled (np.random.permutation, the global NumPy state) after standardisation.

preprocess_split_data(..., device=<index>) runs the passes over the (n, D) matrices on the GPU (csrc/featprep.hip):
the splits' 'features' become DeviceFeatures, which classifier.MLPModel takes without a trip through the host.

stratified_shuffle_split restates sklearn's StratifiedShuffleSplit(n_splits=1) in NumPy, index for index: the cut of the training
rows that the parameter search without a validation fold makes (classifier/train.py:408-423).

FoldBank reads every fold of a dataset once and puts the splits of any cross-validation fold together from them, on the GPU by one
copy kernel per split (l3_feat_assemble): what classifier.cross_validate runs on.
"""
import os

import numpy as np

from . import _lib

DATASET_NUM_FOLDS = {'us8k': 10, 'esc50': 5, 'dcase2013': 2}


def load_feature_file(feature_filepath):
    """One feature file -> (X, y): X the frames (or one vector), y an int when the file holds a single label for the clip,
    else the array as stored (data/usc/folds.py:16-21)."""
    with np.load(feature_filepath) as npz:
        frames, label = npz['X'], npz['y']
    if isinstance(label, np.ndarray) and label.ndim == 0:
        label = int(label)
    return frames, label


def _is_augmented_us8k(fold_dir, name):
    # US8K's augmented copies carry '_' in their file names (data/usc/folds.py:35-37); only the training folds read them
    return 'us8k' in fold_dir and '_' in name


def _row_ranges(counts):
    """[[start, end), ...] of consecutive blocks of the given sizes"""
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    return np.stack((ends - np.asarray(counts, dtype=np.int64), ends), axis=1)


def get_fold(feature_dir, fold_idx, augment=False):
    """Fold `fold_idx` (0-based, directory fold<fold_idx + 1>) -> {'features', 'labels', 'file_idxs', 'filenames'}
    (data/usc/folds.py:24-62).  Files in os.listdir order; 'filenames' lists the whole directory, skipped files included."""
    fold_dir = os.path.join(feature_dir, 'fold%d' % (fold_idx + 1))
    names = os.listdir(fold_dir)
    wanted = [n for n in names if augment or not _is_augmented_us8k(fold_dir, n)]
    loaded = [load_feature_file(os.path.join(fold_dir, n)) for n in wanted]
    frames = [x for x, _ in loaded]
    labels = [lab for _, lab in loaded]
    per_file = isinstance(labels[0], int) or np.ndim(labels[0]) == 0
    return {
        'features': np.vstack(frames),
        'labels': np.array(labels) if per_file else np.concatenate(labels),
        'file_idxs': _row_ranges([x.shape[0] if x.ndim > 1 else 1 for x in frames]),
        'filenames': names,
    }


def get_valid_fold_idx(test_fold_idx, num_folds):
    """the fold before the test fold, wrapping around (data/usc/folds.py:78-79)"""
    return (test_fold_idx + num_folds - 1) % num_folds


def _no_training_fold(num_folds, test_fold_idx, valid):
    # dcase2013 has two folds: a test and a validation fold leave none (the reference fails inside np.vstack)
    return ValueError('No training fold left: {} folds, test fold {}, validation fold held out: {}; use the parameter '
                      'search without a validation fold'.format(num_folds, test_fold_idx + 1, valid))


def get_train_folds(feature_dir, test_fold_idx, num_folds, valid=True):
    """Every fold but the test fold (and the validation fold when `valid`), augmented files included, stacked; each fold's
    file_idxs continue after the rows of the folds before it (data/usc/folds.py:82-112)."""
    held_out = {test_fold_idx}
    if valid:
        held_out.add(get_valid_fold_idx(test_fold_idx, num_folds))
    folds = [get_fold(feature_dir, i, augment=True) for i in range(num_folds) if i not in held_out]
    if not folds:
        raise _no_training_fold(num_folds, test_fold_idx, valid)
    first_row = np.cumsum([0] + [f['features'].shape[0] for f in folds[:-1]])
    return {
        'features': np.vstack([f['features'] for f in folds]),
        'labels': np.concatenate([f['labels'] for f in folds]),
        'file_idxs': np.vstack([f['file_idxs'] + off for f, off in zip(folds, first_row)]),
        'filenames': [name for f in folds for name in f['filenames']],
    }


def _num_folds(dataset_name):
    num_folds = DATASET_NUM_FOLDS.get(dataset_name)
    if num_folds is None:
        raise ValueError('unknown dataset {!r}: one of {}'.format(dataset_name, ', '.join(sorted(DATASET_NUM_FOLDS))))
    return num_folds


def get_split(feature_dir, test_fold_idx, dataset_name, valid=True):
    """-> (train, valid or None, test) for one cross-validation fold (data/usc/folds.py:65-75)"""
    num_folds = _num_folds(dataset_name)
    train = get_train_folds(feature_dir, test_fold_idx, num_folds, valid=valid)
    held = get_fold(feature_dir, get_valid_fold_idx(test_fold_idx, num_folds)) if valid else None
    return train, held, get_fold(feature_dir, test_fold_idx)


class FoldBank(object):
    """Every fold of a dataset read once and kept, so that the splits of all cross-validation folds come from one pass over the
    files: split() gives what get_split gives, with 'features' put together from the kept folds -- on GPU `device` by one copy
    kernel per split (DeviceFeatures.assemble; the download has the bits of get_split's array), or with device=None in NumPy.

    Per fold it keeps what get_fold(..., augment=True) reads: the rows of all files in os.listdir order (one DeviceFeatures, or
    one array), and on the host each file's label, its row range, the directory listing and which files are US8K augmented
    copies.  A validation or test fold leaves those copies out, so it is put together from the other files' row ranges and its
    file_idxs are numbered as get_fold(augment=False) numbers them.

    Memory: the bank holds the dataset once and a split assembled from it holds up to all of it again; close the splits'
    DeviceFeatures when a fold is done, and the bank (close(), or a with block) at the end."""

    def __init__(self, feature_dir, dataset_name, device=0):
        self.feature_dir, self.dataset_name = feature_dir, dataset_name
        self.device = None if device is None else int(device)
        self.num_folds = _num_folds(dataset_name)
        self.folds = []
        try:
            for i in range(self.num_folds):
                self.folds.append(self._read_fold(i))
        except Exception:
            self.close()
            raise

    def _read_fold(self, fold_idx):
        fold_dir = os.path.join(self.feature_dir, 'fold%d' % (fold_idx + 1))
        names = os.listdir(fold_dir)
        loaded = [load_feature_file(os.path.join(fold_dir, n)) for n in names]
        frames = [x for x, _ in loaded]
        features = np.vstack(frames)
        if self.device is not None:
            features = DeviceFeatures(features, self.device)
        return {
            'features': features,
            'labels': [lab for _, lab in loaded],
            'file_idxs': _row_ranges([x.shape[0] if x.ndim > 1 else 1 for x in frames]),
            'filenames': names,
            'augmented': np.array([_is_augmented_us8k(fold_dir, n) for n in names], dtype=bool),
        }

    @staticmethod
    def _labels(labels):
        # get_fold's rule, decided by the first file it reads
        per_file = isinstance(labels[0], int) or np.ndim(labels[0]) == 0
        return np.array(labels) if per_file else np.concatenate(labels)

    def _segments(self, fold_idx, augment):
        """-> (row ranges of the fold's matrix that make up the part, its labels, its file_idxs)"""
        fold = self.folds[fold_idx]
        keep = np.ones(len(fold['filenames']), dtype=bool) if augment else ~fold['augmented']
        ranges = fold['file_idxs'][keep]
        labels = self._labels([lab for lab, k in zip(fold['labels'], keep) if k])
        # neighbouring files are one range
        starts = np.flatnonzero(np.r_[True, ranges[1:, 0] != ranges[:-1, 1]])
        runs = [(int(ranges[a, 0]), int(ranges[b - 1, 1])) for a, b in zip(starts, np.r_[starts[1:], len(ranges)])]
        return [(fold['features'], lo, hi) for lo, hi in runs], labels, _row_ranges(ranges[:, 1] - ranges[:, 0])

    def _assemble(self, segments):
        if self.device is not None:
            return DeviceFeatures.assemble(segments, device=self.device)
        return np.concatenate([x[lo:hi] for x, lo, hi in segments])

    def split(self, test_fold_idx, valid=True):
        """-> (train, valid or None, test) as get_split(feature_dir, test_fold_idx, dataset_name, valid) returns them; 'features' is a
        new DeviceFeatures (a new array with device=None) that the caller owns"""
        self._open()
        held_out = {test_fold_idx}
        if valid:
            held_out.add(get_valid_fold_idx(test_fold_idx, self.num_folds))
        train_folds = [i for i in range(self.num_folds) if i not in held_out]
        if not train_folds:
            raise _no_training_fold(self.num_folds, test_fold_idx, valid)
        held_folds = ([get_valid_fold_idx(test_fold_idx, self.num_folds)] if valid else []) + [test_fold_idx]
        train_parts = [self._segments(i, True) for i in train_folds]
        first_row = np.cumsum([0] + [int(idxs[-1, 1]) for _, _, idxs in train_parts[:-1]])
        splits = [{
            'labels': np.concatenate([labels for _, labels, _ in train_parts]),
            'file_idxs': np.vstack([idxs + off for (_, _, idxs), off in zip(train_parts, first_row)]),
            'filenames': [name for i in train_folds for name in self.folds[i]['filenames']],
        }]
        segments = [[seg for segs, _, _ in train_parts for seg in segs]]
        for i in held_folds:
            segs, labels, idxs = self._segments(i, False)
            splits.append({'labels': labels, 'file_idxs': idxs, 'filenames': list(self.folds[i]['filenames'])})
            segments.append(segs)
        try:
            for d, segs in zip(splits, segments):
                d['features'] = self._assemble(segs)
        except Exception:
            for d in splits:          # what was assembled before the failure; the bank itself is untouched
                if isinstance(d.get('features'), DeviceFeatures):
                    d['features'].close()
            raise
        return (splits[0], splits[1], splits[2]) if valid else (splits[0], None, splits[1])

    def _open(self):
        if self.folds is None:
            raise ValueError('the FoldBank is closed')

    def close(self):
        for fold in self.folds or []:
            if isinstance(fold['features'], DeviceFeatures):
                fold['features'].close()
        self.folds = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- scalers with sklearn.preprocessing's arithmetic ----------------------------------------------------------------------------
def _handle_zeros(scale):
    scale = np.array(scale, copy=True)
    scale[scale == 0.0] = 1.0
    return scale


class StandardScaler(object):
    """sklearn.preprocessing.StandardScaler(): mean_, var_ (population), scale_ = sqrt(var_) with 0 -> 1."""

    def fit(self, X):
        X = np.asarray(X)
        return self._fitted(X.mean(axis=0, dtype=np.float64), X.var(axis=0, dtype=np.float64), X.shape[0])

    def _fitted(self, mean, var, n):
        self.mean_ = mean
        self.var_ = var
        self.scale_ = _handle_zeros(np.sqrt(self.var_))
        self.n_samples_seen_ = n
        return self

    def transform(self, X):
        X = np.array(X, dtype=np.result_type(np.asarray(X).dtype, np.float32), copy=True)
        X -= self.mean_          # in place, in the input's float type, as sklearn does
        X /= self.scale_
        return X

    def fit_transform(self, X):
        return self.fit(X).transform(X)


class MinMaxScaler(object):
    """sklearn.preprocessing.MinMaxScaler(feature_range=(0, 1)): X * scale_ + min_, a zero range scaling by 1."""

    def __init__(self, feature_range=(0, 1)):
        self.feature_range = feature_range

    def fit(self, X):
        X = np.asarray(X)
        return self._fitted(np.min(X, axis=0), np.max(X, axis=0))

    def _fitted(self, data_min, data_max):
        self.data_min_ = data_min
        self.data_max_ = data_max
        self.data_range_ = self.data_max_ - self.data_min_
        lo, hi = self.feature_range
        self.scale_ = (hi - lo) / _handle_zeros(self.data_range_)
        self.min_ = lo - self.data_min_ * self.scale_
        return self

    def transform(self, X):
        X = np.array(X, copy=True)
        X *= self.scale_
        X += self.min_
        return X

    def fit_transform(self, X):
        return self.fit(X).transform(X)


# ---- data/usc/features.py ---------------------------------------------------------------------------------------------------
def sample_non_overlap_file(X, chunk_size=10):
    """every chunk_size-th frame, starting with the first (data/usc/features.py:52-57)"""
    return np.asarray(X)[::chunk_size]


def remove_data_overlap(data, chunk_size=10):
    """In place: keep every chunk_size-th frame of each file and renumber file_idxs (data/usc/features.py:60-73)."""
    kept = [sample_non_overlap_file(data['features'][s:e], chunk_size) for s, e in data['file_idxs']]
    data['file_idxs'] = _row_ranges([len(k) for k in kept])
    data['features'] = np.vstack(kept)


def compute_stats_features(embeddings):
    """min, max, median, mean, var, skew, excess kurtosis over axis 0 (scipy.stats.skew / kurtosis with bias=True)"""
    x = np.asarray(embeddings)
    mean = np.mean(x, axis=0)
    var = np.var(x, axis=0)
    d = x.astype(np.float64) - x.mean(axis=0, dtype=np.float64)
    m2 = (d ** 2).mean(axis=0)
    m3 = (d ** 3).mean(axis=0)
    m4 = (d ** 4).mean(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        # a constant column (m2 == 0 up to rounding): skew 0 and kurtosis -3, as the scipy of the reference's era returned
        # (scipy >= 1.9 returns NaN there)
        zero = m2 <= (np.finfo(np.float64).resolution * x.mean(axis=0, dtype=np.float64)) ** 2
        skew = np.where(zero, 0.0, m3 / m2 ** 1.5)
        kurt = np.where(zero, -3.0, m4 / m2 ** 2 - 3.0)
    return np.concatenate((np.min(x, axis=0), np.max(x, axis=0), np.median(x, axis=0), mean, var,
                           skew.astype(mean.dtype), kurt.astype(mean.dtype)))


def framewise_to_stats(data):
    """In place: one row of summary statistics per file, file i owning row i (data/usc/features.py:76-85)."""
    rows = [compute_stats_features(data['features'][s:e]) for s, e in data['file_idxs']]
    data['features'] = np.vstack(rows)
    data['file_idxs'] = _row_ranges(np.ones(len(rows), dtype=np.int64))


def expand_framewise_labels(data):
    """In place: each file's label repeated once per frame of the file (data/usc/features.py:88-94)."""
    spans = [e - s for s, e in data['file_idxs']]
    n = min(len(spans), len(data['labels']))
    data['labels'] = np.repeat(np.asarray(data['labels'])[:n], spans[:n], axis=0)


def _present(*splits):
    return [d for d in splits if d]


def _require_float32(X):
    if X.dtype != np.float32:
        raise ValueError('the device path preprocesses float32 features; these are {} (there is no silent conversion: cast '
                         'them, or preprocess on the host with device=None)'.format(X.dtype))


class DeviceFeatures(object):
    """A split's feature matrix on the GPU (an l3_feat handle, _lib.Features): what preprocess_split_data(device=...) leaves in
    data['features'].  It holds no host copy; to_host() / rows() download."""

    def __init__(self, X, device=0):
        X = np.asarray(X)
        _require_float32(X)
        self.device = int(device)
        self.handle = _lib.Features(X if X.ndim == 2 else X.reshape(len(X), -1), device=self.device)

    @classmethod
    def from_handle(cls, handle):
        """the DeviceFeatures that owns an existing _lib.Features"""
        self = cls.__new__(cls)
        self.device, self.handle = handle.device, handle
        return self

    @classmethod
    def assemble(cls, segments, device=0):
        """a new matrix on `device` from the rows [lo, hi) of each (DeviceFeatures, lo, hi), in order, copied there by one kernel
        (_lib.Features.assemble); the sources stay as they are"""
        return cls.from_handle(_lib.Features.assemble([(f.handle, lo, hi) for f, lo, hi in segments], device=device))

    def split(self, rows_a, rows_b=None):
        """X[rows_a] and X[rows_b] as two new DeviceFeatures on this GPU, which the caller owns and closes, written by one kernel
        (_lib.Features.split); this matrix stays as it is.  rows_b None: -> (DeviceFeatures, None)"""
        a, b = self.handle.split(rows_a, rows_b)
        return type(self).from_handle(a), (None if b is None else type(self).from_handle(b))

    @property
    def shape(self):
        return self.handle.shape

    def __len__(self):
        return self.shape[0]

    def rows(self, lo, hi):
        """rows [lo, hi) as a NumPy array"""
        return self.handle.download(lo, hi)

    def to_host(self):
        return self.handle.download()

    def close(self):
        self.handle.close()


def non_overlap_rows(file_idxs, chunk_size=10):
    """remove_data_overlap as an index table: the rows it keeps, in order, and the renumbered file_idxs"""
    kept = [np.arange(s, e, chunk_size, dtype=np.int64) for s, e in file_idxs]
    return np.concatenate(kept), _row_ranges([len(k) for k in kept])


def _preprocess_on_device(train_data, valid_data, test_data, feature_mode, non_overlap, chunk_size, use_min_max, device):
    """preprocess_split_data's stages in its order with the (n, D) passes on the GPU; labels, file_idxs, the D-sized scaler
    arithmetic and the draw of the permutation stay on the host, in the host path's own expressions"""
    everything = _present(train_data, valid_data, test_data)
    for d in everything:          # before anything is uploaded or replaced
        if isinstance(d['features'], DeviceFeatures):
            if d['features'].device != int(device):
                raise ValueError('a split\'s features are on device {}, the preprocessing runs on device {}'.format(
                    d['features'].device, device))
        else:
            _require_float32(np.asarray(d['features']))
    for d in everything:          # a resident split (FoldBank.split) is preprocessed where it is
        if not isinstance(d['features'], DeviceFeatures):
            d['features'] = DeviceFeatures(d['features'], device)
    feats = [d['features'].handle for d in everything]
    if non_overlap:
        for d, f in zip(everything, feats):
            rows, d['file_idxs'] = non_overlap_rows(d['file_idxs'], chunk_size)
            f.gather(rows)

    unit_range = MinMaxScaler()
    if use_min_max:
        unit_range._fitted(*train_data['features'].handle.minmax())
        for f in feats:
            f.affine32(unit_range.scale_, unit_range.min_)

    if feature_mode == 'stats':
        for d, f in zip(everything, feats):
            f.file_stats(d['file_idxs'])
            d['file_idxs'] = _row_ranges(np.ones(len(d['file_idxs']), dtype=np.int64))
    else:
        for d in _present(train_data, valid_data):
            expand_framewise_labels(d)

    mean, var = train_data['features'].handle.moments()
    stdizer = StandardScaler()._fitted(mean, var, len(train_data['features']))
    for f in feats:
        f.standardize(stdizer.mean_, stdizer.scale_)

    order = np.random.permutation(len(train_data['labels']))
    new_position = np.empty_like(order)
    new_position[order] = np.arange(order.size)
    train_data['features'].handle.gather(order)
    train_data['labels'] = train_data['labels'][order]
    train_data['file_idxs'] = [new_position[s:e] for s, e in train_data['file_idxs']]
    return unit_range, stdizer


def preprocess_split_data(train_data, valid_data, test_data, feature_mode='framewise', non_overlap=False,
                          non_overlap_chunk_size=10, use_min_max=False, device=None):
    """data/usc/features.py:97-150, in place on the splits (valid_data may be None) -> (min-max scaler, standardiser).

    Order: thin overlapping frames; min-max scaling (fitted on train, when asked); per-frame labels or per-file statistics;
    standardisation fitted on train; then one np.random.permutation of the training rows (the global NumPy state), after which
    train_data['file_idxs'] is a list holding, per file, the new positions of its rows.

    device: None runs everything in NumPy on the host.  A GPU index runs the same stages with the passes over the feature
    matrices on that GPU (float32 features only; NumPy arrays are uploaded, DeviceFeatures on that GPU -- FoldBank.split -- are
    used where they are, and one on another GPU is a ValueError): every split's 'features' is then a DeviceFeatures, min-max scaled values are
    the host path's bits, and the standardiser's mean_ / var_ agree with the host's to the rounding of a float64 sum."""
    if feature_mode not in ('framewise', 'stats'):
        raise ValueError("feature_mode must be 'framewise' or 'stats', not {!r}".format(feature_mode))
    if device is not None:
        return _preprocess_on_device(train_data, valid_data, test_data, feature_mode, non_overlap, non_overlap_chunk_size,
                                     use_min_max, device)
    everything = _present(train_data, valid_data, test_data)
    if any(isinstance(d['features'], DeviceFeatures) for d in everything):
        raise ValueError('a split\'s features are on a GPU (DeviceFeatures) and device is None: name the device, or download them')
    if non_overlap:
        for d in everything:
            remove_data_overlap(d, chunk_size=non_overlap_chunk_size)

    unit_range = MinMaxScaler()
    if use_min_max:
        unit_range.fit(train_data['features'])
        for d in everything:
            d['features'] = unit_range.transform(d['features'])

    if feature_mode == 'stats':
        for d in everything:
            framewise_to_stats(d)
    else:
        for d in _present(train_data, valid_data):       # the test split keeps one label per file
            expand_framewise_labels(d)

    stdizer = StandardScaler().fit(train_data['features'])
    for d in everything:
        d['features'] = stdizer.transform(d['features'])

    order = np.random.permutation(len(train_data['labels']))
    new_position = np.empty_like(order)
    new_position[order] = np.arange(order.size)
    train_data['features'] = train_data['features'][order]
    train_data['labels'] = train_data['labels'][order]
    train_data['file_idxs'] = [new_position[s:e] for s, e in train_data['file_idxs']]
    return unit_range, stdizer


def _approximate_mode(class_counts, n_draws, rng):
    """sklearn.utils.extmath._approximate_mode: how many of n_draws rows each class gets -- the floor of its proportional share,
    then one more for the classes with the largest remainders, equal remainders drawn with rng.choice(replace=False)"""
    continuous = class_counts / class_counts.sum() * n_draws
    floored = np.floor(continuous)
    need_to_add = int(n_draws - floored.sum())
    if need_to_add > 0:
        remainder = continuous - floored
        for value in np.sort(np.unique(remainder))[::-1]:
            inds, = np.where(remainder == value)
            add_now = min(len(inds), need_to_add)
            floored[rng.choice(inds, size=add_now, replace=False)] += 1
            need_to_add -= add_now
            if need_to_add == 0:
                break
    return floored.astype(int)


def stratified_shuffle_split(labels, valid_ratio=0.15, random_state=None):
    """sklearn 1.7's StratifiedShuffleSplit(n_splits=1, test_size=valid_ratio, random_state=random_state) over `labels`
    -> (train_idx, valid_idx), int64, the indices sklearn gives for the same integer seed: n_valid = ceil(valid_ratio * n) rows
    validate, each class is shared out between the two parts in proportion (_approximate_mode), and every draw comes from one
    np.random.RandomState(random_state) in sklearn's order -- the remainder ties of the train counts, then of the validation counts,
    one permutation per class in class order, one of the train list, one of the validation list.

    random_state must be given (the reference passes none, so its split differs from run to run; here every draw has a seed).
    ValueError where sklearn raises one: a ratio outside (0, 1), a class of fewer than two members, fewer train or validation rows
    than classes."""
    if random_state is None:
        raise ValueError('stratified_shuffle_split needs a random_state: every draw of this project comes from an explicit seed')
    labels = np.asarray(labels)
    if labels.ndim != 1:
        raise ValueError('labels must be one class per row, not an array of {} dimensions'.format(labels.ndim))
    if not 0.0 < valid_ratio < 1.0:
        raise ValueError('valid_ratio={} should be a float in the (0, 1) range'.format(valid_ratio))
    n = labels.shape[0]
    n_valid = int(np.ceil(valid_ratio * n))
    n_train = n - n_valid
    if n_train == 0:
        raise ValueError('With n_samples={} and valid_ratio={}, the resulting train set will be empty.'.format(n, valid_ratio))
    classes, y_indices = np.unique(labels, return_inverse=True)
    n_classes = classes.shape[0]
    class_counts = np.bincount(y_indices)
    if np.min(class_counts) < 2:
        raise ValueError('The least populated class in y has only 1 member, which is too few. The minimum number of groups for any '
                         'class cannot be less than 2.')
    if n_train < n_classes:
        raise ValueError('The train_size = %d should be greater or equal to the number of classes = %d' % (n_train, n_classes))
    if n_valid < n_classes:
        raise ValueError('The test_size = %d should be greater or equal to the number of classes = %d' % (n_valid, n_classes))
    class_indices = np.split(np.argsort(y_indices, kind='mergesort'), np.cumsum(class_counts)[:-1])

    rng = np.random.RandomState(random_state)
    n_i = _approximate_mode(class_counts, n_train, rng)
    t_i = _approximate_mode(class_counts - n_i, n_valid, rng)
    train, valid = [], []
    for i in range(n_classes):
        shuffled = class_indices[i].take(rng.permutation(class_counts[i]), mode='clip')
        train.append(shuffled[:n_i[i]])
        valid.append(shuffled[n_i[i]:n_i[i] + t_i[i]])
    train = rng.permutation(np.concatenate(train).astype(np.int64))
    valid = rng.permutation(np.concatenate(valid).astype(np.int64))
    return train, valid
