"""A group of MLP classifiers on the GPU (the l3_mlp_group handle, _lib.MLPGroup, classifier.train_mlp_search) against
the single model (_lib.MLP, the loop over classifier.train_mlp), bit for bit: a member's epochs, a live set with a hole, keep and
restore, prediction from host rows, a device matrix and the resident rows, the whole search, and argument validation.

The shapes are small and chosen where the indexing can go wrong: D = 600 is no multiple of 32 and the first layer's forward splits
K four ways at 64 rows; 500 rows in batches of 64 leave a last batch of 52; C is 10 and 50; every member has its own seed, rate and
weight decay.  The single models are trained once per class count and shared.

The search runs the reference's 3 x 3 grid for 6 epochs with patience 1 on data on which, in the float64 restatement
(tests/mlp_ref.py through tests/mlp_group_ref.py), the points run 6, 6, 6, 6, 6, 6, 4, 3, 6 epochs on the validation fold and
6, 6, 6, 6, 6, 6, 5, 3, 6 on the cut: the live set shrinks while other members train on.  (On the MI355X in float32 the cut runs
6, 6, 6, 6, 6, 6, 4, 4, 6: two val_loss values 1e-4 apart relative fall the other way; the test asserts only that the lengths differ.)"""
import os

import numpy as np
import pytest

import mlp_group_ref as G
from l3embedding_amd import _lib, classifier, usc

pytestmark = pytest.mark.gpu

D, N, NV, B, EPOCHS = 600, 500, 70, 64, 3
STEPS = -(-N // B)
LRS = [1e-3, 1e-4, 3e-3, 1e-5, 2e-3, 5e-4, 1e-2, 7e-4, 3e-4]
WDS = [1e-5, 1e-3, 1e-4, 0.0, 1e-2, 3e-5, 1e-4, 1e-3, 1e-5]
SEEDS = [11, 12, 13, 2 ** 40 + 5, 15, 16, 17, 18, 19]
_RS = np.random.RandomState(2)
PERMS = [_RS.permutation(N) for _ in range(EPOCHS)]          # one per epoch, the same for every model


def _data(C):
    return G.clusters(D=D, C=C, n=N, nv=NV, nt=90, seed=3)


_SOLO = {}


def _solo(C):
    """the nine single models of a class count, each trained EPOCHS epochs -> per member (statistics per epoch, weights after each
    epoch, probabilities of the test, training and validation rows after the last); computed once"""
    if C not in _SOLO:
        X, y, Xv, yv, Xt, _ = _data(C)
        runs = []
        for lr, wd, seed in zip(LRS, WDS, SEEDS):
            m = _lib.MLP(D, C, B, weight_decay=wd, seed=seed)
            m.set_data(X, y, Xv, yv)
            stats, weights = [], [m.get_weights()]
            for e in range(EPOCHS):
                stats.append(m.epoch(PERMS[e], lr, e * STEPS))
                weights.append(m.get_weights())
            runs.append((stats, weights, [m.predict(a) for a in (Xt, X, Xv)]))
            m.close()
        _SOLO[C] = runs
    return _SOLO[C]


def _group(C, members, on_device=False):
    X, y, Xv, yv, _, _ = _data(C)
    g = _lib.MLPGroup(D, C, B, [WDS[i] for i in members], [SEEDS[i] for i in members])
    if on_device:
        with_tail = usc.DeviceFeatures(np.vstack((X, Xv, X[:3])))          # the validation rows are a range of the same matrix
        g.set_data_dev(with_tail.handle, 0, N, y, with_tail.handle, N, N + NV, yv)
        with_tail.close()
    else:
        g.set_data(X, y, Xv, yv)
    return g


def _assert_weights(got, want):
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('members,C,on_device', [((0, 1, 2), 10, False), ((4,), 10, False), (tuple(range(9)), 10, False),
                                                 ((3, 4, 5), 50, False), ((6, 7, 8), 10, True)])
def test_a_member_equals_the_model_alone(gpu_required, members, C, on_device):
    solo = _solo(C)
    g = _group(C, members, on_device)
    for k, i in enumerate(members):
        _assert_weights(g.get_weights(k), solo[i][1][0])          # the Glorot draw of the member's seed
    for e in range(EPOCHS):
        stats = g.epoch(PERMS[e], [LRS[i] for i in members], e * STEPS)
        for k, i in enumerate(members):
            print('C %d member %d epoch %d: %r' % (C, i, e, stats[k]))
            assert stats[k] == solo[i][0][e], (i, e)
    for k, i in enumerate(members):
        _assert_weights(g.get_weights(k), solo[i][1][EPOCHS])
    g.close()


def test_a_live_set_with_a_hole(gpu_required):
    solo = _solo(10)
    members = (0, 1, 2)
    g = _group(10, members)
    lrs = [LRS[i] for i in members]
    assert g.epoch(PERMS[0], lrs, 0, live=[True, True, True]) == [solo[i][0][0] for i in members]
    for e in (1, 2):
        stats = g.epoch(PERMS[e], lrs, e * STEPS, live=[True, False, True])
        assert stats[0] == solo[0][0][e] and stats[2] == solo[2][0][e]
        assert all(np.isnan(v) for v in stats[1].values())
    _assert_weights(g.get_weights(0), solo[0][1][EPOCHS])
    _assert_weights(g.get_weights(2), solo[2][1][EPOCHS])
    _assert_weights(g.get_weights(1), solo[1][1][1])          # left as it was after its one epoch
    # one live member in the middle of the group: its second epoch is the single model's
    stats = g.epoch(PERMS[1], lrs, STEPS, live=[False, True, False])
    assert stats[1] == solo[1][0][1] and all(np.isnan(v) for k in (0, 2) for v in stats[k].values())
    _assert_weights(g.get_weights(1), solo[1][1][2])
    # no live member: nothing runs, every statistic is NaN, the weights stay
    stats = g.epoch(PERMS[0], lrs, 3 * STEPS, live=[False, False, False])
    assert all(np.isnan(v) for s in stats for v in s.values())
    _assert_weights(g.get_weights(0), solo[0][1][EPOCHS])
    g.close()


def test_keep_and_restore(gpu_required):
    solo = _solo(10)
    members = (0, 1, 2)
    g = _group(10, members)
    lrs = [LRS[i] for i in members]
    g.epoch(PERMS[0], lrs, 0)
    g.keep_best([0, 2])
    g.epoch(PERMS[1], lrs, STEPS)
    g.keep_best([1])
    g.keep_best([])
    g.epoch(PERMS[2], lrs, 2 * STEPS)
    for k in members:
        _assert_weights(g.get_weights(k), solo[k][1][3])          # a snapshot changes nothing
    g.restore_best([0])
    _assert_weights(g.get_weights(0), solo[0][1][1])
    _assert_weights(g.get_weights(1), solo[1][1][3])
    _assert_weights(g.get_weights(2), solo[2][1][3])
    g.restore_best([1, 2])
    _assert_weights(g.get_weights(1), solo[1][1][2])
    _assert_weights(g.get_weights(2), solo[2][1][1])
    # a later snapshot replaces the member's earlier one and no other member's
    g.epoch(PERMS[0], lrs, 3 * STEPS, live=[False, False, True])
    later = g.get_weights(2)
    assert not np.array_equal(later[0], solo[2][1][1][0])
    g.keep_best([2])
    g.epoch(PERMS[1], lrs, 4 * STEPS, live=[False, False, True])
    g.restore_best([0, 2])
    _assert_weights(g.get_weights(2), later)
    _assert_weights(g.get_weights(0), solo[0][1][1])
    g.close()


def test_group_prediction(gpu_required):
    solo = _solo(10)
    members = (0, 1, 2)
    X, y, Xv, yv, Xt, _ = _data(10)
    g = _group(10, members)
    for e in range(EPOCHS):
        g.epoch(PERMS[e], [LRS[i] for i in members], e * STEPS)
    on_host, on_train, on_valid = g.predict(Xt), g.predict_resident(), g.predict_resident(valid=True)
    feat = usc.DeviceFeatures(np.vstack((X[:7], Xt)))
    on_device = g.predict_dev(feat.handle, 7, 7 + len(Xt))
    feat.close()
    assert on_host.shape == (3, len(Xt), 10) and on_train.shape == (3, N, 10) and on_valid.shape == (3, NV, 10)
    for k in members:
        np.testing.assert_array_equal(on_host[k], solo[k][2][0])
        np.testing.assert_array_equal(on_device[k], solo[k][2][0])
        np.testing.assert_array_equal(on_train[k], solo[k][2][1])
        np.testing.assert_array_equal(on_valid[k], solo[k][2][2])
    # more rows than one staging block holds: the blocks are the single model's
    many = np.tile(Xt, (47, 1))[:4200]
    single = _lib.MLP(D, 10, B, weight_decay=WDS[1], seed=SEEDS[1])
    single.set_weights(solo[1][1][EPOCHS])
    np.testing.assert_array_equal(g.predict(many)[1], single.predict(many))
    single.close()
    g.close()


SEARCH = dict(batch_size=B, num_epochs=6, patience=1, num_classes=10, random_state=7)


def _read(path):
    with open(path, 'rb') as fh:
        return fh.read()


@pytest.mark.parametrize('valid_fold,train_with_valid,on_device', [(True, False, False), (True, True, False), (False, True, False),
                                                                   (False, False, False), (False, False, True), (True, True, True)])
def test_the_search_equals_the_loop(gpu_required, tmp_path, valid_fold, train_with_valid, on_device):
    outcomes = []
    for name in ('loop', 'group'):
        train, valid, test = G.splits(D=D, C=10, n=N, nv=NV, seed=3)
        made = []
        if on_device:
            for split in (train, valid, test):
                split['features'] = usc.DeviceFeatures(split['features'])
                made.append(split['features'])
        extra = {} if valid_fold else dict(split_random_state=11)
        d = str(tmp_path / name)
        os.makedirs(d)
        np.random.seed(5)          # the refit on train + valid shuffles them with NumPy's global state
        if name == 'loop':
            outcomes.append(classifier.train_param_search(train, valid if valid_fold else None, test, d, train_func=classifier.train_mlp,
                                                          search_space=classifier.MLP_SEARCH_SPACE, train_with_valid=train_with_valid,
                                                          **dict(SEARCH, **extra)))
        else:
            outcomes.append(classifier.train_mlp_search(train, valid if valid_fold else None, test, d, train_with_valid=train_with_valid,
                                                        **dict(SEARCH, **extra)))
        for f in made:
            f.close()
    loop, group = outcomes
    lengths = [len(m['loss_history']) for m in group[2]['search'].values()]
    print('epochs per point:', lengths, 'chosen', group[1]['search_params_best_values'])
    for part in (1, 2, 3):
        assert G.same(loop[part], group[part]), part
    assert loop[1]['search_params_best_values'] == group[1]['search_params_best_values']
    assert list(group[1]['search']) == list(loop[1]['search']) and group[2]['search_params'] == ['learning_rate', 'weight_decay']
    _assert_weights(group[0].get_weights(), loop[0].get_weights())
    assert len(set(lengths)) > 1 and min(lengths) < SEARCH['num_epochs'], lengths
    assert _read(os.path.join(str(tmp_path / 'loop'), 'history_csvlog.csv')) == _read(os.path.join(str(tmp_path / 'group'), 'history_csvlog.csv'))
    _assert_weights(classifier.kerasfile.load_dense_weights(os.path.join(str(tmp_path / 'group'), 'model.h5')), group[0].get_weights())


def test_argument_validation(gpu_required):
    """every refusal of the ABI; no case launches anything"""
    def code(fn):
        with pytest.raises(_lib.L3Error) as ei:
            fn()
        return str(ei.value)
    assert 'error -1' in code(lambda: _lib.MLPGroup(16, 10, 8, [], []))
    assert 'error -1' in code(lambda: _lib.MLPGroup(16, 10, 8, [0.0] * 17, [0] * 17))
    assert 'error -1' in code(lambda: _lib.MLPGroup(16, 65, 8, [0.0], [0]))
    assert 'error -1' in code(lambda: _lib.MLPGroup(16, 10, 0, [0.0], [0]))
    assert 'error -1' in code(lambda: _lib.MLPGroup(0, 10, 8, [0.0], [0]))
    assert 'error -1' in code(lambda: _lib.MLPGroup(16, 10, 8, [0.0, -1e-3], [0, 1]))
    assert 'error -1' in code(lambda: _lib.MLPGroup(16, 10, 8, [0.0, float('nan')], [0, 1]))
    lib = _lib.load()
    assert lib.l3_mlp_group_create(0, 16, 10, 8, 2, None, None, None) == -1
    g = _lib.MLPGroup(16, 10, 8, [0.0, 1e-4], [1, 2])
    X = np.zeros((4, 16), np.float32)
    y = np.zeros(4, np.int32)
    stats = np.zeros(8)
    lr, live, perm = np.full(2, 1e-3, np.float32), np.ones(2, np.int32), np.arange(4, dtype=np.int32)
    # before any data: L3_ESTATE
    assert lib.l3_mlp_group_epoch(g.h, perm.ctypes.data, lr.ctypes.data, live.ctypes.data, 0, stats.ctypes.data) == -4
    assert 'error -4' in code(lambda: g.predict_resident())
    assert 'error -4' in code(lambda: g.restore_best([0]))
    assert 'error -1' in code(lambda: g.set_data(X, np.array([0, 1, 10, 2])))
    assert 'error -1' in code(lambda: g.set_data(X, np.array([0, -1, 1, 2])))
    assert 'error -1' in code(lambda: g.set_data(X[:0], np.zeros(0, np.int32)))
    assert 'error -1' in code(lambda: g.set_data(X, y, X, np.array([0, 1, 2, 10])))
    assert lib.l3_mlp_group_set_data(g.h, X.ctypes.data, y.ctypes.data, 1 << 40, None, None, 0) == -1       # oversized: rejected unread
    assert lib.l3_mlp_group_set_data(g.h, X.ctypes.data, y.ctypes.data, (1 << 31) - 1, None, None, 0) == -3
    feat, narrow = usc.DeviceFeatures(X), usc.DeviceFeatures(X[:, :8])
    assert 'error -1' in code(lambda: g.set_data_dev(narrow.handle, 0, 4, y))
    assert lib.l3_mlp_group_set_data_dev(g.h, feat.handle.h, 0, 5, y.ctypes.data, None, 0, 0, None) == -1
    assert lib.l3_mlp_group_set_data_dev(g.h, feat.handle.h, 0, 4, y.ctypes.data, feat.handle.h, 3, 5, y.ctypes.data) == -1
    assert 'error -1' in code(lambda: g.predict_dev(narrow.handle))
    assert 'error -1' in code(lambda: g.predict_dev(feat.handle, 2, 5))
    g.set_data(X, np.array([0, 1, 2, 3]))
    assert 'error -4' in code(lambda: g.predict_resident(valid=True))          # no validation rows
    assert 'error -1' in code(lambda: g.epoch(np.array([0, 1, 2, 4]), lr, 0))
    assert 'error -1' in code(lambda: g.epoch(perm, lr, -1))
    assert lib.l3_mlp_group_epoch(g.h, perm.ctypes.data, lr.ctypes.data, None, 0, stats.ctypes.data) == -1
    assert lib.l3_mlp_group_epoch(g.h, perm.ctypes.data, None, live.ctypes.data, 0, stats.ctypes.data) == -1
    assert lib.l3_mlp_group_epoch(g.h, perm.ctypes.data, lr.ctypes.data, live.ctypes.data, 0, None) == -1
    with pytest.raises(ValueError):
        g.epoch(perm, [1e-3], 0)
    assert 'error -1' in code(lambda: g.keep_best([2]))
    assert 'error -1' in code(lambda: g.restore_best([5]))
    assert 'error -1' in code(lambda: g.get_weights(2))
    assert 'error -1' in code(lambda: g.get_weights(-1))
    flat = np.zeros(g.param_count() + 1, np.float32)
    assert lib.l3_mlp_group_get_weights(g.h, 0, flat.ctypes.data, flat.size) == -1
    assert lib.l3_mlp_group_set_weights(g.h, 0, None, flat.size - 1) == -1
    assert lib.l3_mlp_group_predict(g.h, None, 4, flat.ctypes.data) == -1
    assert lib.l3_mlp_group_predict(g.h, X.ctypes.data, 0, flat.ctypes.data) == -1
    assert lib.l3_mlp_group_predict_resident(g.h, 2, flat.ctypes.data) == -1
    assert lib.l3_mlp_group_keep_best(None, 1) == -1 and lib.l3_mlp_group_param_count(None) == -1
    with pytest.raises(ValueError):
        g.set_weights(0, [np.zeros((3, 3), np.float32)] * 6)
    feat.close()
    narrow.close()
    g.close()
