"""The random forest on the GPU (csrc/forest.hip through l3embedding_amd/forest.py) against its NumPy oracle (tests/forest_ref.py):
the trees are the oracle's exactly -- children, feature, bin, the threshold's bits, the per-class counts, the distinct-row counts --
and predict_proba agrees to 1e-12, on the smallest shapes at which each mechanism can break; both node searches give
the same trees; NumPy rows and usc.DeviceFeatures give the same bits; both fixture sets meet sklearn's own seed-to-seed spread."""
import functools
import os
import pickle

import numpy as np
import pytest

import forest_ref as R
from l3embedding_amd import classifier, usc
from l3embedding_amd.forest import RandomForestClassifier

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 7


def _data(n, D, C, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, C, n)
    return (rs.randn(C, D)[y] * 0.8 + rs.randn(n, D)).astype(np.float32), y


def _ties():
    X, y = _data(300, 5, 3, 2)
    X[:, 1] = 0.5               # a constant column: no cut
    X[:, 3] = X[:, 2]           # two identical columns: equal candidates, the earlier draw wins
    return X, y


# name -> (data, n_classes, n_estimators, the forest's arguments)
CASES = {
    'one_row': (lambda: _data(1, 4, 1, 0), 1, 2, {}),
    'one_class': (lambda: _data(40, 6, 1, 1), 1, 2, {}),
    'ties': (_ties, 3, 3, {}),
    'sampled_cuts': (lambda: _data(700, 70, 10, 3), 10, 3, dict(bin_sample=512)),          # S > 256, multiplicities > 1
    'fifty_classes': (lambda: _data(2000, 33, 50, 4), 50, 2, {}),                          # the 51 KB histogram, D % 4 != 0
    'one_tree': (lambda: _data(260, 9, 4, 8), 4, 1, {}),
    'seven_trees': (lambda: _data(600, 12, 4, 0), 4, 7, {}),                               # nodes of 63, 64 and 65 rows
    'bounded': (lambda: _data(700, 70, 10, 5), 10, 3, dict(max_depth=4, min_samples_leaf=3)),
    'split_of_six': (lambda: _data(500, 8, 5, 6), 5, 3, dict(min_samples_split=6, max_features=8)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (X, y, the oracle's forest): computed once, shared by the tests, never written to"""
    make, C, T, kw = CASES[name]
    X, y = make()
    ref = R.fit_forest(X, y, T, SEED, C, max_features=kw.get('max_features'), max_depth=kw.get('max_depth'),
                       min_samples_split=kw.get('min_samples_split', 2), min_samples_leaf=kw.get('min_samples_leaf', 1),
                       bin_sample=kw.get('bin_sample', 4096))
    for a in (X, y) + tuple(ref.values()):
        a.setflags(write=False)
    return X, y, ref


def _fit(name, X=None, **more):
    _, C, T, kw = CASES[name]
    Xc, y, _ = _case(name)
    return RandomForestClassifier(n_estimators=T, random_state=SEED, **dict(kw, **more)).fit(Xc if X is None else X, y)


def _assert_trees_equal(got, want):
    for k in R.TREE_ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if k == 'threshold':
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert a.shape == b.shape, k
        assert np.array_equal(a, b), '%s differs first at %s' % (k, np.argwhere(a != b)[0])


@pytest.mark.parametrize('name', sorted(CASES))
def test_trees_are_the_oracles(gpu_required, name):
    X, y, ref = _case(name)
    m = _fit(name)
    _assert_trees_equal(m.estimators_, ref)
    probe = X[:256]
    got = m.predict_proba(probe)
    assert got.dtype == np.float64 and np.abs(got - R.predict_proba(ref, probe)).max() <= 1e-12
    assert np.abs(got.sum(axis=1) - 1).max() < 1e-12
    if name in ('one_row', 'one_class'):          # the root is a leaf
        assert ref['left'].size == CASES[name][2] and np.all(ref['left'] == -1)
    if name == 'ties':
        assert not np.any(ref['feature'] == 1) and np.any(ref['feature'] >= 0)
    if name == 'bounded':
        leaf = ref['left'] < 0
        assert ref['n_distinct'][leaf].min() >= 3 and len(m.level_stats_[0]) == 5
    if name == 'sampled_cuts':
        assert R.bootstrap(R.tree_seeds(SEED, 3)[0], 700).max() > 1


@pytest.mark.parametrize('name', ['seven_trees', 'fifty_classes', 'sampled_cuts', 'bounded'])
def test_both_searches_give_the_same_trees(gpu_required, name):
    """wide_min_rows 1: every node through the workgroup-per-(node, feature) search; n + 1: every node of at most 64 rows through
    the wave-per-node search"""
    X, _, ref = _case(name)
    if name == 'seven_trees':
        assert {63, 64, 65} <= set(ref['n_distinct'].tolist())          # both sides of the 64-row limit of the wave search
    for wide_min_rows in (1, X.shape[0] + 1):
        m = _fit(name, wide_min_rows=wide_min_rows)
        _assert_trees_equal(m.estimators_, ref)
        nodes, wide, _ = m.level_stats_
        assert nodes.sum() == ref['left'].size
        assert wide.sum() == (nodes.sum() if wide_min_rows == 1 else (ref['n_distinct'] > 64).sum())


def test_device_features_give_the_same_bits(gpu_required):
    X, _, ref = _case('sampled_cuts')
    dev = usc.DeviceFeatures(X, device=0)
    try:
        m = _fit('sampled_cuts', X=dev)
        _assert_trees_equal(m.estimators_, ref)
        assert np.array_equal(m.predict_proba(dev), _fit('sampled_cuts').predict_proba(X))
        assert np.array_equal(m.predict(dev), m.predict(X))
    finally:
        dev.close()


def test_pickle_round_trip(gpu_required):
    X, _, ref = _case('seven_trees')
    m = _fit('seven_trees')
    again = pickle.loads(pickle.dumps(m))
    assert again._h is None
    _assert_trees_equal(again.estimators_, ref)
    assert np.array_equal(again.predict_proba(X), m.predict_proba(X))
    # a forest uploaded from the oracle's arrays predicts as the oracle does
    again.estimators_, again._resident = {k: v.copy() for k, v in ref.items()}, False
    assert np.abs(again.predict_proba(X) - R.predict_proba(ref, X)).max() <= 1e-12


def test_bad_arguments_are_refused_before_any_launch(gpu_required):
    from l3embedding_amd import _lib
    X, y, ref = _case('one_tree')
    h = _lib.Forest(0)
    h.set_data(X)
    boot = np.ones((1, X.shape[0]), np.uint16)
    for labels, b, kw, msg in ((np.where(y == 0, 4, y), boot, {}, 'labels'), (y, boot * 0, {}, 'no row'), (y, boot, dict(max_features=10), 'max_features'),
                               (y, boot, dict(bin_rows=[3, 3]), 'bin_rows'), (y, boot, dict(bin_rows=[0, 260]), 'bin_rows')):
        with pytest.raises(_lib.L3Error, match=msg):
            h.fit(labels, b, [1], 4, **dict(dict(max_features=3), **kw))
    bad = {k: v.copy() for k, v in ref.items()}
    bad['left'][0] = 0          # a child must lie above its parent
    with pytest.raises(_lib.L3Error, match='child'):
        h.set_trees(bad, X.shape[1])
    bad = {k: v.copy() for k, v in ref.items()}
    bad['feature'][0] = X.shape[1]
    with pytest.raises(_lib.L3Error, match='feature'):
        h.set_trees(bad, X.shape[1])
    h.close()


@pytest.mark.parametrize('name', ['gauss', 'relu'])
def test_fixture_sets_meet_the_sklearn_bar(gpu_required, name):
    g = np.load(os.path.join(HERE, 'golden', 'forest_%s.npz' % name))
    acc = g['sklearn_accuracy']
    bar = float(acc.mean() - 3 * acc.std())
    m = RandomForestClassifier(n_estimators=int(g['n_estimators']), random_state=0).fit(g['X'], g['y'])
    got = float((m.predict(g['Xt']) == g['yt']).mean())
    print('%s: accuracy %.4f, sklearn %.4f +- %.4f, bar %.4f' % (name, got, acc.mean(), acc.std(), bar))
    assert got >= bar


def test_train_rf_gives_the_oracles_metrics(gpu_required, tmp_path):
    X, y, _ = _case('one_tree')
    files = np.array([[0, 20], [20, 45], [45, 60]])
    train, valid = dict(features=X[:160], labels=y[:160]), dict(features=X[160:200], labels=y[160:200])
    test = dict(features=X[200:], labels=np.array([0, 1, 2]), file_idxs=files)
    clf, tm, vm, sm = classifier.train_rf(train, valid, test, str(tmp_path), n_estimators=4, num_classes=4, random_state=5)
    want = R.fit_forest(X[:160], y[:160], 4, 5, 4)
    _assert_trees_equal(clf.estimators_, want)
    assert tm['loss'] == 0 and vm['loss'] == 0
    assert tm['accuracy'] == (R.predict_proba(want, X[:160]).argmax(axis=1) == y[:160]).mean()
    assert vm['accuracy'] == (R.predict_proba(want, X[160:200]).argmax(axis=1) == y[160:200]).mean()
    p = R.predict_proba(want, X[200:])
    per_file = np.array([p[s:e].mean(axis=0).argmax() for s, e in files])
    assert sm['accuracy'] == (per_file == test['labels']).mean()
    with open(os.path.join(str(tmp_path), 'model.pkl'), 'rb') as fh:
        assert np.array_equal(pickle.load(fh).predict(X), clf.predict(X))


@pytest.mark.parametrize('device', [None, 0])
def test_train_rf_fold_writes_the_fold(gpu_required, tmp_path, device):
    fdir = R.write_fold_tree(str(tmp_path))
    out = str(tmp_path / 'out')
    mdir = classifier.train_rf_fold(fdir, out, 1, preprocess_device=device, n_estimators=10)
    assert sorted(os.listdir(mdir)) == ['config.json', 'min_max_scaler.pkl', 'model.pkl', 'results.pkl', 'stdizer.pkl']
    with open(os.path.join(mdir, 'results.pkl'), 'rb') as fh:
        results = pickle.load(fh)
    assert results['train']['accuracy'] > 0.9 and results['test']['accuracy'] > 0.5 and results['valid']['loss'] == 0
