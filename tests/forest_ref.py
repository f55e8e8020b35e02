"""The NumPy oracle of the level-wise histogram forest (l3embedding_amd/forest.py, csrc/forest.hip): cuts, codes,
draws, split search, partition and numbering, prediction.  Plain loops over trees, nodes and drawn features; integer counts in int64 and
the one float64 formula of a split's worth, so the GPU forest equals it exactly.  Written from the design, not from the library: it
shares no code with l3embedding_amd.
"""
import numpy as np

MAX_CUTS = 255
GOLD = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
TREE_ARRAYS = ('tree_off', 'left', 'right', 'feature', 'threshold', 'bin', 'counts', 'n_distinct')


# ---- 3. draws ------------------------------------------------------------------------------------------------------------------------
def fmix64(z):
    """splitmix64's finaliser on uint64 arrays (the products wrap)"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def draw_features(seed, node, D, K):
    """Floyd's subset sampling: for i, j in enumerate(range(D - K, D)): t = rand(j + 1); take j if t is already chosen, else t, with
    rand(n) = ((h >> 32) n) >> 32 and h the mixer of (seed, node, i) -> K distinct features in draw order"""
    with np.errstate(over='ignore'):
        a = fmix64(np.array([seed], np.uint64) * GOLD + np.array([node], np.uint64))
        h = fmix64(a + (np.arange(K, dtype=np.uint64) + np.uint64(1)) * GOLD)
    j = np.arange(D - K, D, dtype=np.uint64)
    t = ((h >> np.uint64(32)) * (j + np.uint64(1))) >> np.uint64(32)
    picks = []
    for ji, ti in zip(j.tolist(), t.tolist()):
        picks.append(ji if ti in picks else ti)
    return picks


def tree_seeds(random_state, n_estimators):
    return np.random.RandomState(random_state).randint(np.iinfo(np.int32).max, size=n_estimators)


def bootstrap(seed, n):
    return np.bincount(np.random.RandomState(int(seed)).randint(0, n, n), minlength=n)


# ---- 1. cuts, 2. codes ------------------------------------------------------------------------------------------------------------
def sample_rows(n, bin_sample, random_state):
    if n <= bin_sample:
        return np.arange(n)
    return np.sort(np.random.RandomState(random_state).choice(n, bin_sample, replace=False))


def column_cuts(values):
    """the cuts of one sampled column -> float32 array of at most 255 strictly increasing thresholds"""
    s = np.sort(np.asarray(values, np.float32))
    S = s.size
    positions = range(1, S) if S <= 256 else [(j * S) // 256 for j in range(1, 256)]
    cuts = []
    for p in positions:
        if s[p - 1] < s[p]:
            t = np.float32((np.float64(s[p - 1]) + np.float64(s[p])) / 2)
            if t >= s[p]:
                t = s[p - 1]
            cuts.append(t)
    return np.array(cuts, np.float32)


def make_cuts(X, bin_sample=4096, random_state=None):
    """-> (cuts (D, 255) float32, zero beyond ncuts; ncuts (D))"""
    X = np.asarray(X, np.float32)
    rows = sample_rows(X.shape[0], bin_sample, random_state)
    cuts, ncuts = np.zeros((X.shape[1], MAX_CUTS), np.float32), np.zeros(X.shape[1], np.int32)
    for f in range(X.shape[1]):
        c = column_cuts(X[rows, f])
        cuts[f, :c.size], ncuts[f] = c, c.size
    return cuts, ncuts


def make_codes(X, cuts, ncuts):
    """code[f][i] = the number of cuts of f below X[i][f] -> (D, N) uint8"""
    X = np.asarray(X, np.float32)
    return np.stack([np.searchsorted(cuts[f, :ncuts[f]], X[:, f], side='left') for f in range(X.shape[1])]).astype(np.uint8)


# ---- 4. split search, 5. partition and numbering ------------------------------------------------------------------------------------
def best_split(codes, ncuts, y, w, rows, picks, C, min_samples_leaf):
    """-> (feature, bin, rows going left) of the best candidate of the node, or None: the largest proxy, the earlier draw on ties, then
    the lower bin"""
    best, found = -1.0, None
    n = rows.size
    for f in picks:
        nc = int(ncuts[f])
        if nc == 0:
            continue
        c = codes[f, rows].astype(np.int64)
        hist = np.zeros((256, C), np.int64)
        np.add.at(hist, (c, y[rows]), w[rows])
        left = np.cumsum(hist, axis=0)
        left_rows = np.cumsum(np.bincount(c, minlength=256))
        total = left[-1]
        L, R = left[:nc], total - left[:nc]
        valid = (left_rows[:nc] >= min_samples_leaf) & (n - left_rows[:nc] >= min_samples_leaf)
        if not valid.any():
            continue
        with np.errstate(divide='ignore', invalid='ignore'):          # an invalid bin may have an empty side
            proxy = ((L * L).sum(axis=1).astype(np.float64) / L.sum(axis=1).astype(np.float64)
                     + (R * R).sum(axis=1).astype(np.float64) / R.sum(axis=1).astype(np.float64))
        proxy = np.where(valid, proxy, -1.0)
        b = int(np.argmax(proxy))          # the first of the largest: the lower bin on ties
        if proxy[b] > best:
            best, found = proxy[b], (f, b)
    if found is None:
        return None
    return found[0], found[1], codes[found[0], rows] <= found[1]


def grow_tree(codes, ncuts, cuts, y, w, seed, C, K, max_depth=None, min_samples_split=2, min_samples_leaf=1):
    """one tree, level by level -> dict of its arrays (TREE_ARRAYS without tree_off)"""
    D = codes.shape[0]
    y = np.asarray(y, np.int64)
    w = np.asarray(w, np.int64)
    nodes = [dict(rows=np.flatnonzero(w > 0))]
    frontier, depth = [0], 0
    while frontier:
        split = []
        for i in frontier:
            node = nodes[i]
            rows = node['rows']
            node['counts'] = np.bincount(y[rows], weights=w[rows], minlength=C).astype(np.int64)          # exact: integers below 2^53
            node['found'] = None
            n = rows.size
            if (max_depth is not None and depth >= max_depth) or n < min_samples_split or n < 2 * min_samples_leaf:
                continue
            if (node['counts'] > 0).sum() <= 1:
                continue
            node['found'] = best_split(codes, ncuts, y, w, rows, draw_features(seed, i, D, K), C, min_samples_leaf)
            if node['found'] is not None:
                split.append(i)
        frontier = []
        for i in split:          # children numbered in parent order, left before right
            f, b, goes_left = nodes[i]['found']
            rows = nodes[i]['rows']
            nodes[i]['left'] = len(nodes)
            nodes.append(dict(rows=rows[goes_left]))
            nodes.append(dict(rows=rows[~goes_left]))
            frontier += [len(nodes) - 2, len(nodes) - 1]
        depth += 1
    m = len(nodes)
    out = dict(left=np.full(m, -1, np.int32), right=np.full(m, -1, np.int32), feature=np.full(m, -1, np.int32),
               threshold=np.zeros(m, np.float32), bin=np.full(m, -1, np.int32), counts=np.zeros((m, C), np.int32),
               n_distinct=np.zeros(m, np.int32))
    for i, node in enumerate(nodes):
        out['counts'][i], out['n_distinct'][i] = node['counts'], node['rows'].size
        if node.get('found') is not None:
            f, b, _ = node['found']
            out['left'][i], out['right'][i] = node['left'], node['left'] + 1
            out['feature'][i], out['bin'][i], out['threshold'][i] = f, b, cuts[f, b]
    return out


def fit_forest(X, y, n_estimators, random_state, n_classes, max_features=None, max_depth=None, min_samples_split=2,
               min_samples_leaf=1, bin_sample=4096):
    """-> the forest as flat arrays (TREE_ARRAYS); y holds class indices below n_classes"""
    X = np.asarray(X, np.float32)
    n, D = X.shape
    K = max(1, int(np.sqrt(D))) if max_features is None else max_features
    cuts, ncuts = make_cuts(X, bin_sample, random_state)
    codes = make_codes(X, cuts, ncuts)
    trees = [grow_tree(codes, ncuts, cuts, y, bootstrap(seed, n), int(seed), n_classes, K, max_depth, min_samples_split,
                       min_samples_leaf) for seed in tree_seeds(random_state, n_estimators)]
    out = {k: np.concatenate([t[k] for t in trees]) for k in TREE_ARRAYS[1:]}
    out['tree_off'] = np.concatenate(([0], np.cumsum([t['left'].size for t in trees]))).astype(np.int64)
    return out


# ---- 6. prediction ------------------------------------------------------------------------------------------------------------------
def predict_proba(forest, X):
    """every row walks the trees in order on the raw float32 features; each leaf adds counts / their sum in float64; / n_trees"""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    off = forest['tree_off']
    p = np.zeros((n, forest['counts'].shape[1]), np.float64)
    at = np.arange(n)
    for t in range(off.size - 1):
        node = np.full(n, off[t], np.int64)
        while True:
            left = forest['left'][node]
            inner = left >= 0
            if not inner.any():
                break
            feat = np.where(inner, forest['feature'][node], 0)
            goes_left = X[at, feat] <= forest['threshold'][node]
            node = np.where(inner, off[t] + np.where(goes_left, left, forest['right'][node]), node)
        c = forest['counts'][node].astype(np.int64)
        p += c.astype(np.float64) / c.sum(axis=1, keepdims=True).astype(np.float64)
    return p / np.float64(off.size - 1)



# ---- a toy feature tree for the fold drivers --------------------------------------------------------------------------------------
def write_fold_tree(root, dataset='esc50', folds=5, D=12, C=3, files=3, frames=5, seed=0):
    """features/<dataset>/l3/synthetic/fold1..foldN/*.npz as usc_generate writes them (X frames, y the class) -> that directory"""
    import os
    r = np.random.RandomState(seed)
    centres = r.randn(C, D) * 1.5
    fdir = os.path.join(root, 'features', dataset, 'l3', 'synthetic')
    for f in range(folds):
        d = os.path.join(fdir, 'fold%d' % (f + 1))
        os.makedirs(d)
        for c in range(C):
            for k in range(files):
                np.savez(os.path.join(d, '%d-%d-%d.npz' % (f, c, k)), X=(centres[c] + r.randn(frames, D)).astype(np.float32), y=np.array(c))
    return fdir
