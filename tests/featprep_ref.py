"""Row-order restatements of the fold-preprocessing arithmetic (include/l3hip.h, "Fold preprocessing") and the error
bounds its tests use.  Everything here is NumPy on the host; tests/test_featprep_host.py checks each restatement against
usc.compute_stats_features / StandardScaler / MinMaxScaler, tests/test_featprep_gpu.py checks the kernels against them.

u = 2^-53 is the unit roundoff of float64.  The bounds are first-order in u (the omitted terms are below 1e-13 of the bound at
every size used here).

Scaler fit.  NumPy adds the n rows one after the other, the device adds chunks of CHUNK rows in row order and then the chunks'
sums in chunk order.  Either sum is within (n - 1) u sum|x| of the exact one, so the two means differ by at most
    mean_bound = 2 (n - 1) u sum|x| / n.
Each side then forms d = fl(x - mean) (relative error u), d * d (u more, 3 u on the square in all), adds n of them ((n - 1) u of
the sum of squares) and divides (u): each variance is within (n + 3) u V of V(mean) = sum (x - mean)^2 / n, and V(mean) itself
moves by (mean - exact mean)^2 <= (mean_bound / 2)^2 with the mean's error.  So the two variances differ by at most
    var_bound = 2 (n + 3) u V + (mean_bound / 2)^2.

Skew and kurtosis.  Both sides hold the same float64 mean, d and m2 (the same operations in the same order).  NumPy forms d^3 and
d^4 with pow (taken as 1 ulp = 2 u), the kernel as (d d) d (2 u) and (d d)(d d) (3 u); each side then adds F terms ((F - 1) u of
sum|term|) and divides by F (u).  With A3 = mean|d|^3:
    |m3 - m3'| <= (2 F + 4) u A3            |m4 - m4'| <= (2 F + 5) u m4.
The denominators are pow(m2, 1.5) against m2 sqrt(m2) (2 u each) and m2 m2 on both sides (u each); the quotient adds u per side and
the subtraction of 3 another u |kurtosis| per side:
    skew_bound = (2 F + 4) u A3 / m2^1.5 + 6 u |skew|
    kurt_bound = (2 F + 5) u m4 / m2^2 + 4 u (kurtosis + 3) + 2 u |kurtosis|,
to which the comparison adds half a float32 ulp of the device's value for its cast (the host side is compared in float64).
"""
import numpy as np

from l3embedding_amd import usc

CHUNK = 256          # L3_FEAT_CHUNK_ROWS
LDS_ROWS = 64        # L3_FEAT_STATS_LDS_ROWS
U = 2.0 ** -53


def seq_sum(rows, dtype):
    """the rows added one after the other in `dtype`"""
    acc = np.zeros(rows.shape[1], dtype)
    for r in rows:
        acc = acc + r.astype(dtype)
    return acc


def seq_moments(x):
    """StandardScaler.fit's mean_ and var_ with the rows added in order (NumPy's own order)"""
    n = x.shape[0]
    mean = seq_sum(x, np.float64) / n
    d = x.astype(np.float64) - mean
    return mean, seq_sum(d * d, np.float64) / n


def chunked_moments(x, chunk=CHUNK):
    """l3_feat_moments: chunks of `chunk` rows in row order, the chunks' sums in chunk order"""
    n = x.shape[0]

    def total(rows):
        acc = np.zeros(rows.shape[1], np.float64)
        for lo in range(0, n, chunk):
            acc = acc + seq_sum(rows[lo:lo + chunk], np.float64)
        return acc

    mean = total(x) / n
    d = x.astype(np.float64) - mean
    return mean, total(d * d) / n


def moments_bounds(x, var):
    """(mean_bound, var_bound) of the module docstring for the matrix x whose variance is `var`"""
    n = x.shape[0]
    mean_bound = 2.0 * (n - 1) * U * np.abs(x.astype(np.float64)).sum(axis=0) / n
    return mean_bound, 2.0 * (n + 3) * U * var + (0.5 * mean_bound) ** 2


def affine32(x, scale, shift):
    """l3_feat_affine32: two float32 roundings"""
    return (x * scale.astype(np.float32)).astype(np.float32) + shift.astype(np.float32)


def standardize(x, mean, scale):
    """l3_feat_standardize: each step in float64, rounded to float32"""
    t = (x.astype(np.float64) - mean).astype(np.float32)
    return (t.astype(np.float64) / scale).astype(np.float32)


def median32(x):
    """the middle element, or fl32(fl32(a + b) / 2) of the two middle ones"""
    s = np.sort(x, axis=0)
    F = x.shape[0]
    if F % 2:
        return s[F // 2]
    with np.errstate(over='ignore'):
        return (s[F // 2 - 1] + s[F // 2]) / np.float32(2)


def central_moments64(x):
    """float64 mean in row order, d = fl64(x) - mean and NumPy's m2, m3, m4 (d ** 3 and d ** 4 through pow), in row order"""
    F = x.shape[0]
    mean = seq_sum(x, np.float64) / F
    d = x.astype(np.float64) - mean
    return mean, d, seq_sum(d ** 2, np.float64) / F, seq_sum(d ** 3, np.float64) / F, seq_sum(d ** 4, np.float64) / F


def skew_kurt64(x):
    """usc.compute_stats_features' skew and excess kurtosis before the cast to float32, with their bounds:
    -> (skew, kurtosis, skew_bound, kurt_bound, zero), all float64 (zero: the columns the zero rule sets to 0 and -3)"""
    F = x.shape[0]
    mean, d, m2, m3, m4 = central_moments64(x)
    with np.errstate(divide='ignore', invalid='ignore'):
        zero = m2 <= (np.finfo(np.float64).resolution * mean) ** 2
        skew = np.where(zero, 0.0, m3 / m2 ** 1.5)
        kurt = np.where(zero, -3.0, m4 / m2 ** 2 - 3.0)
        a3 = seq_sum(np.abs(d) ** 3, np.float64) / F
        skew_bound = np.where(zero, 0.0, (2 * F + 4) * U * a3 / m2 ** 1.5 + 6 * U * np.abs(skew))
        kurt_bound = np.where(zero, 0.0, (2 * F + 5) * U * m4 / m2 ** 2 + 4 * U * (kurt + 3.0) + 2 * U * np.abs(kurt))
    return skew, kurt, skew_bound, kurt_bound, zero


def stats_row(x):
    """compute_stats_features(x) restated in row order: the seven blocks of one file, float32"""
    F = np.float32(x.shape[0])
    with np.errstate(over='ignore', invalid='ignore'):
        mean = seq_sum(x, np.float32) / F
        t = x - mean
        var = seq_sum(t * t, np.float32) / F
    skew, kurt = skew_kurt64(x)[:2]
    return np.concatenate((x.min(axis=0), x.max(axis=0), median32(x), mean, var, skew.astype(np.float32), kurt.astype(np.float32)))


def host_pipeline(train, valid, test, feature_mode, non_overlap, chunk_size, use_min_max, stdizer=None):
    """usc.preprocess_split_data on the host, in place, with the standardiser given (the device's own) instead of a fitted one"""
    everything = [d for d in (train, valid, test) if d]
    if non_overlap:
        for d in everything:
            usc.remove_data_overlap(d, chunk_size=chunk_size)
    unit_range = usc.MinMaxScaler()
    if use_min_max:
        unit_range.fit(train['features'])
        for d in everything:
            d['features'] = unit_range.transform(d['features'])
    if feature_mode == 'stats':
        for d in everything:
            usc.framewise_to_stats(d)
    else:
        for d in everything[:-1]:
            usc.expand_framewise_labels(d)
    if stdizer is None:
        stdizer = usc.StandardScaler().fit(train['features'])
    for d in everything:
        d['features'] = stdizer.transform(d['features'])
    order = np.random.permutation(len(train['labels']))
    new_position = np.empty_like(order)
    new_position[order] = np.arange(order.size)
    train['features'] = train['features'][order]
    train['labels'] = train['labels'][order]
    train['file_idxs'] = [new_position[s:e] for s, e in train['file_idxs']]
    return unit_range, stdizer


def make_splits(seed, D=130, files=(14, 9, 11), num_classes=4, constant_column=True):
    """a synthetic (train, valid, test) set: files of 1 .. 40 frames, float32, one label per file"""
    r = np.random.RandomState(seed)
    out = []
    for n_files in files:
        counts = r.randint(1, 41, size=n_files)
        counts[:3] = (1, 2, 31)
        x = (r.randn(int(counts.sum()), D) * r.uniform(0.1, 3.0, size=D) + r.uniform(-2, 2, size=D)).astype(np.float32)
        if constant_column:
            x[:, D // 2] = np.float32(0.625)
        out.append({'features': x, 'labels': r.randint(0, num_classes, size=n_files), 'file_idxs': usc._row_ranges(counts),
                    'filenames': ['f%d' % i for i in range(n_files)]})
    return out


def copy_splits(splits):
    return [None if d is None else {k: (v.copy() if isinstance(v, np.ndarray) else list(v)) for k, v in d.items()} for d in splits]
