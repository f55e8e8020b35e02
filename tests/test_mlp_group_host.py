"""The MLP's parameter search fitted as one group of models, on the host (classifier.fit_mlp_grid / train_mlp_search /
train_mlp_search_fold, cli_mlp_search): _lib.MLP and _lib.MLPGroup replaced by the float64 stand-ins of
tests/mlp_group_ref.py, the search against the loop train_param_search(train_func=train_mlp) in every result, record and file, the
per-member checkpoint and early-stopping bookkeeping on scripted val_loss series, the command line, the fold's files.  The kernels
and the handle against the single model are tests/test_mlp_group_gpu.py."""
import inspect
import json
import os
import pickle

import numpy as np
import pytest

import forest_ref
import mlp_group_ref as G
from l3embedding_amd import _lib, classifier, cli_classifier, cli_mlp_search

RefGroup = G.make_group(G.RefMLP)


@pytest.fixture
def stand_ins(monkeypatch):
    monkeypatch.setattr(_lib, 'MLP', G.RefMLP)
    monkeypatch.setattr(_lib, 'MLPGroup', RefGroup)
    RefGroup.made = []


def _read(path):
    with open(path, 'rb') as fh:
        return fh.read()


def _small():
    return G.splits(D=24, C=4, n=150, nv=40, files=6, frames=5, seed=4, spread=0.05)


ARGS = dict(batch_size=8, num_epochs=6, patience=1, num_classes=4, random_state=7)


def _both(tmp_path, valid_fold, train_with_valid):
    """the loop and the group on the same splits -> (loop outcome, group outcome, loop directory, group directory)"""
    train, valid, test = _small()
    extra = {} if valid_fold else dict(split_random_state=11, valid_ratio=0.25)
    out = []
    for name in ('loop', 'group'):
        d = str(tmp_path / name)
        os.makedirs(d)
        np.random.seed(5)          # the refit on train + valid shuffles them with NumPy's global state
        if name == 'loop':
            out.append(classifier.train_param_search(train, valid if valid_fold else None, test, d, train_func=classifier.train_mlp,
                                                     search_space=classifier.MLP_SEARCH_SPACE, train_with_valid=train_with_valid,
                                                     **dict(ARGS, **extra)))
        else:
            out.append(classifier.train_mlp_search(train, valid if valid_fold else None, test, d, train_with_valid=train_with_valid,
                                                   **dict(ARGS, **extra)))
    return out[0], out[1], str(tmp_path / 'loop'), str(tmp_path / 'group')


@pytest.mark.parametrize('valid_fold', [True, False])
@pytest.mark.parametrize('train_with_valid', [False, True])
def test_the_search_equals_the_loop(stand_ins, tmp_path, valid_fold, train_with_valid):
    loop, group, loop_dir, group_dir = _both(tmp_path, valid_fold, train_with_valid)
    for part in (1, 2, 3):
        assert G.same(loop[part], group[part]), part
    assert list(group[2]['search']) == list(classifier.product(*classifier.MLP_SEARCH_SPACE.values()))
    assert group[1]['search_params'] == ['learning_rate', 'weight_decay']
    assert loop[1]['search_params_best_values'] == group[1]['search_params_best_values']
    for a, b in zip(loop[0].get_weights(), group[0].get_weights()):
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a, b)
    assert isinstance(group[0], classifier.MLPModel)
    # the points stop at different epochs, so the live set shrank while others went on
    lengths = [len(m['loss_history']) for m in group[2]['search'].values()]
    assert len(set(lengths)) > 1 and min(lengths) < ARGS['num_epochs'], lengths
    grid = RefGroup.made[0]
    assert grid.n_members == 9 and grid.uploads == 1 and any(not all(live) for live in grid.epochs_run)
    assert [sum(live[i] for live in grid.epochs_run) for i in range(9)] == lengths
    # the files: the log and the loss history are the loop's, model.h5 is the returned model
    assert _read(os.path.join(loop_dir, 'history_csvlog.csv')) == _read(os.path.join(group_dir, 'history_csvlog.csv'))
    with open(os.path.join(loop_dir, 'history_checkpoint.pkl'), 'rb') as a, open(os.path.join(group_dir, 'history_checkpoint.pkl'), 'rb') as b:
        assert G.same(pickle.load(a), pickle.load(b))
    assert sorted(os.listdir(group_dir)) == sorted(os.listdir(loop_dir)) == ['history_checkpoint.pkl', 'history_csvlog.csv', 'model.h5']
    for a, b in zip(classifier.kerasfile.load_dense_weights(os.path.join(group_dir, 'model.h5')), group[0].get_weights()):
        assert np.array_equal(a, b)


def test_the_grid_validates_on_the_tail_of_the_training_rows(stand_ins, tmp_path):
    """without validation data the last valid_split of the rows validate, as MLPModel.fit slices them: every point equals its
    train_mlp"""
    train, _, test = _small()
    points = [(1e-3, 1e-4), (1e-2, 1e-3), (1e-4, 1e-5)]
    d = str(tmp_path / 'group')
    os.makedirs(d)
    fitted = classifier.fit_mlp_grid(train, None, test, d, points, valid_split=0.2, **ARGS)
    assert RefGroup.made[0].n_train == 120 and RefGroup.made[0].n_valid == 30
    for (lr, wd), got in zip(points, fitted):
        want = classifier.train_mlp(train, None, test, str(tmp_path), learning_rate=lr, weight_decay=wd, valid_split=0.2, **ARGS)
        assert all(G.same(want[part], got[part]) for part in (1, 2, 3)), (lr, wd)
        assert 'class_accuracy' not in got[2] and len(got[1]['class_accuracy']) == 4
        assert all(np.array_equal(a, b) for a, b in zip(want[0].get_weights(), got[0].get_weights()))
    assert _read(os.path.join(d, 'history_csvlog.csv')) == _read(str(tmp_path / 'history_csvlog.csv'))
    with pytest.raises(ValueError, match='validation rows'):
        classifier.fit_mlp_grid(train, None, test, d, points, valid_split=0.0, **ARGS)
    with pytest.raises(ValueError, match='learning_rate and weight_decay'):
        classifier.train_mlp_search(train, None, test, d, search_space={'learning_rate': [1e-3], 'C': [1]}, split_random_state=1)


def test_more_points_than_a_group_holds(stand_ins, tmp_path):
    train, valid, test = _small()
    points = [(1e-3 * (1 + i), 1e-4) for i in range(_lib.MLP_MAX_MEMBERS + 2)]
    fitted = classifier.fit_mlp_grid(train, valid, test, str(tmp_path), points, **dict(ARGS, num_epochs=1))
    assert [g.n_members for g in RefGroup.made] == [16, 2] and len(fitted) == 18
    assert fitted[16][0].lr == points[16][0]


# ---- the bookkeeping on scripted series ---------------------------------------------------------------------------------------------
# val_loss per epoch, keyed by the weight decay that names the member
SERIES = {
    0.25: [0.9, 0.5, 0.5, 0.7, 0.8, 0.1],          # a tie at the minimum: the first one is kept; stops at the end of epoch 3
    0.5: [0.3, 0.4, 0.5, 0.1, 0.1, 0.1],           # never improves on its first epoch: stops at the end of epoch 2
    0.75: [0.9, 0.8, 0.7, 0.6, 0.5, 0.4],          # improves every epoch: runs to num_epochs
    1.0: [0.9, 0.8, 0.8, 0.7, 0.7, 0.9],           # a tie resets nothing, but the counter is tested before it is incremented
}


class ScriptedMLP(object):
    """_lib.MLP whose val_loss follows SERIES[weight_decay]; its weights hold the number of epochs run, so the returned weights name
    the epoch of the checkpoint"""

    def __init__(self, D, C, batch, weight_decay=0.0, seed=0, device=0):
        self.D, self.C, self.batch, self.wd, self.epochs = D, C, batch, float(np.float32(weight_decay)), 0

    def set_data(self, X, y, Xv=None, yv=None):
        self.n_train = len(X)

    def epoch(self, perm, lr, t0):
        assert t0 == self.epochs * -(-self.n_train // ARGS['batch_size'])
        self.epochs += 1
        return dict(loss=1.0 / self.epochs, acc=0.5, val_loss=SERIES[self.wd][self.epochs - 1], val_acc=0.25 * self.wd)

    def predict(self, X):
        p = np.zeros((len(X), self.C), np.float32)
        p[:, self.epochs % self.C] = 1.0
        return p

    def get_weights(self):
        return [np.full(s, self.epochs, np.float32) for s in _lib.mlp_shapes(self.D, self.C)]

    def set_weights(self, weights):
        self.epochs = int(weights[0].flat[0])

    def close(self):
        pass


def test_checkpoint_and_early_stopping_per_member(monkeypatch, tmp_path):
    Group = G.make_group(ScriptedMLP)
    Group.made = []
    monkeypatch.setattr(_lib, 'MLP', ScriptedMLP)
    monkeypatch.setattr(_lib, 'MLPGroup', Group)
    train, valid, test = _small()
    points = [(1e-3, wd) for wd in SERIES]
    d = str(tmp_path / 'group')
    os.makedirs(d)
    fitted = classifier.fit_mlp_grid(train, valid, test, d, points, **ARGS)
    ran = [len(run[2]['loss_history']) for run in fitted]
    kept = [int(run[0].get_weights()[0].flat[0]) for run in fitted]
    assert ran == [4, 3, 6, 6] and kept == [2, 1, 6, 4]          # epochs run; the 1-based epoch of the first minimum
    assert [run[2]['loss'] for run in fitted] == [0.5, 0.3, 0.4, 0.7]
    assert Group.made[0].epochs_run == [[True] * 4] * 3 + [[True, False, True, True]] + [[False, False, True, True]] * 2
    for (lr, wd), got in zip(points, fitted):
        want = classifier.train_mlp(train, valid, test, str(tmp_path), learning_rate=lr, weight_decay=wd, **ARGS)
        assert all(G.same(want[part], got[part]) for part in (1, 2, 3)), wd
        assert np.array_equal(want[0].get_weights()[0], got[0].get_weights()[0])
    assert _read(os.path.join(d, 'history_csvlog.csv')) == _read(str(tmp_path / 'history_csvlog.csv'))


# ---- the command line and the fold ---------------------------------------------------------------------------------------------------
def test_cli_mlp_search_flag_table():
    args = cli_mlp_search.parse_arguments(['feats', 'out', '3'])
    single = cli_classifier.parse_arguments(['-mt', 'mlp', '-ps', 'feats', 'out', '3'])
    assert set(single) - set(args) == {'model_type', 'parameter_search', 'C', 'tol', 'max_iterations', 'kernel', 'n_estimators'}
    assert all(single[k] == v for k, v in args.items())
    accepted = inspect.signature(classifier.train_mlp_search_fold).parameters
    assert 'parameter_search' not in accepted and 'model_type' not in accepted
    assert all(k in accepted or k in ('num_epochs', 'learning_rate', 'weight_decay') for k in args)
    args = cli_mlp_search.parse_arguments(['-e', '7', '-psnv', '-psss', '5', '-psvr', '0.2', '-pstwv', '-ppd', '0', '-eap', '3', 'f', 'o', '1'])
    assert args['num_epochs'] == 7 and not args['parameter_search_valid_fold'] and args['parameter_search_split_seed'] == 5
    assert args['parameter_search_valid_ratio'] == 0.2 and not args['parameter_search_train_with_valid'] and args['preprocess_device'] == 0
    assert args['patience'] == 3
    for argv in (['-mt', 'mlp', 'f', 'o', '1'], ['-ps', 'f', 'o', '1'], ['f', 'o'], ['-psnv', 'f', 'o', '1'], ['-npf', '2', 'f', 'o', '1']):
        with pytest.raises(SystemExit) as e:
            cli_mlp_search.parse_arguments(argv)
        assert e.value.code == 2


def test_train_mlp_search_fold_writes_trains_files(stand_ins, tmp_path):
    fdir = forest_ref.write_fold_tree(str(tmp_path))
    settings = dict(num_epochs=3, patience=1, learning_rate=1e-4, weight_decay=1e-5, train_batch_size=32)
    dirs = []
    for run in (lambda: classifier.train(fdir, str(tmp_path / 'loop'), 2, model_type='mlp', parameter_search=True, **settings),
                lambda: classifier.train_mlp_search_fold(fdir, str(tmp_path / 'group'), 2, **settings)):
        np.random.seed(3)          # usc.get_split shuffles the training rows with NumPy's global state
        dirs.append(run())
    assert os.path.relpath(dirs[1], str(tmp_path / 'group')).split(os.sep)[:9] == os.path.relpath(dirs[0], str(tmp_path / 'loop')).split(os.sep)[:9]
    assert os.path.relpath(dirs[1], str(tmp_path / 'group')).split(os.sep)[7:9] == ['mlp', 'fold2']
    files = ['config.json', 'history_checkpoint.pkl', 'history_csvlog.csv', 'min_max_scaler.pkl', 'model.h5', 'results.pkl', 'stdizer.pkl']
    assert sorted(os.listdir(dirs[0])) == sorted(os.listdir(dirs[1])) == files
    configs = []
    for d in dirs:
        with open(os.path.join(d, 'config.json')) as fh:
            configs.append(json.load(fh))
    assert list(configs[0]) == list(configs[1]) and 'model_part' not in configs[1]
    assert {k: v for k, v in configs[0].items() if k not in ('model_dir', 'output_dir')} == \
        {k: v for k, v in configs[1].items() if k not in ('model_dir', 'output_dir')}
    assert configs[1]['model_type'] == 'mlp' and configs[1]['parameter_search'] is True
    results = []
    for d in dirs:
        with open(os.path.join(d, 'results.pkl'), 'rb') as fh:
            results.append(pickle.load(fh))
    assert G.same(results[0], results[1])
    assert _read(os.path.join(dirs[0], 'history_csvlog.csv')) == _read(os.path.join(dirs[1], 'history_csvlog.csv'))
    # on a cut: refused without its seed before anything is written
    with pytest.raises(ValueError) as e:
        classifier.train_mlp_search_fold(fdir, str(tmp_path / 'none'), 1, parameter_search_valid_fold=False)
    assert str(e.value) == classifier.NO_SSS and not os.path.exists(str(tmp_path / 'none'))


def test_the_group_entries_are_declared_and_bound():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'l3hip.h')) as fh:
        header = fh.read()
    for name in ('create', 'destroy', 'param_count', 'set_data', 'set_data_dev', 'epoch', 'keep_best', 'restore_best', 'predict',
                 'predict_dev', 'predict_resident', 'get_weights', 'set_weights'):
        entry = 'l3_mlp_group_' + name
        assert entry in _lib.SIGNATURES and entry + '(' in header, entry
        args = header[header.index(entry + '('):].split(';', 1)[0]
        assert len(args.split(',')) == len(_lib.SIGNATURES[entry][1]), entry
