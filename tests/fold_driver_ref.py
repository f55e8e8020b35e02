"""What tests/golden/make_fold_driver_record.py and tests/test_fold_driver_record.py share: a seeded feature tree, deterministic
stand-ins for the native classifiers (_lib.MLP, svm.SVC, svm.fit_grid) that log every call they get, the table of cases and the
function that runs one case and records what it wrote, what the stand-ins received and where NumPy's global stream ended up.

Only public functions of l3embedding_amd.classifier and its documented seams are used, so the same code runs on any commit: the
record of one commit replayed on another shows whether the fold drivers and the searches still do the same thing in the same order.
Nothing here needs a GPU."""
import hashlib
import json
import os
import pickle

import numpy as np

from l3embedding_amd import classifier

D = 8
LOG = []          # the stand-ins' calls, in order; run_case empties it


def write_tree(root, seed=0):
    """<root>/features/esc50/l3/x/fold1 .. fold5: six files of 3 to 6 frames of D float32 per fold, one label per file, three classes
    that every fold holds twice (24 files in four training folds: 20 / 4 when 0.15 of them is cut off)."""
    feats = os.path.join(str(root), 'features', 'esc50', 'l3', 'x')
    r = np.random.RandomState(seed)
    for fold in range(1, 6):
        d = os.path.join(feats, 'fold%d' % fold)
        os.makedirs(d)
        for i in range(6):
            label = (fold + i) % 3
            X = (r.randn(r.randint(3, 7), D) + 0.5 * label).astype(np.float32)
            np.savez(os.path.join(d, 'clip%d.npz' % i), X=X, y=np.array(label))
    return feats


def _sha(a):
    return None if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _plain(v):
    """JSON types: NumPy values as Python ones, tuples as lists, any dictionary key as a string, a float that is not finite as its
    name (so that == compares NaN with NaN); a finite float survives JSON exactly"""
    if isinstance(v, dict):
        return {k if isinstance(k, str) else repr(_plain(k)): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return _plain(v.tolist())
    if isinstance(v, np.generic):
        return _plain(v.item())
    if isinstance(v, float) and not np.isfinite(v):
        return repr(v)
    return v


def _note(who, train=None, train_labels=None, valid=None, valid_labels=None, **kwargs):
    LOG.append({'call': who, 'train_rows': None if train is None else len(train), 'valid_rows': None if valid is None else len(valid),
                'features': [_sha(train), _sha(valid)], 'labels': [_sha(train_labels), _sha(valid_labels)],
                'kwargs': _plain(dict(sorted(kwargs.items())))})


def _row_scores(x, num_classes, state):
    """(n, num_classes) scores, a fixed function of the rows and one number of the model's"""
    x = np.asarray(x, np.float64)
    guess = (np.floor(np.abs(x[:, 0]) * 3.0 + state * 7.0) % 3).astype(np.int64)
    scores = np.full((len(x), num_classes), 0.1 / num_classes)
    scores[np.arange(len(x)), guess] += 0.6
    scores[np.arange(len(x)), (guess + 1) % num_classes] += 0.3 * np.tanh(np.abs(x).mean(axis=1))
    return scores


class FakeMLP(object):
    """_lib.MLP without a GPU: the losses of an epoch are a fixed function of the data, the permutation, the learning rate and the
    epochs so far (the validation loss falls for one epoch and then rises, so that the checkpoint is not the last epoch and early
    stopping ends the fit); the weights carry one number, which predict() reads back"""

    def __init__(self, D, C, batch, weight_decay=0.0, seed=0, device=0):
        self.D, self.C, self.batch, self.weight_decay = int(D), int(C), int(batch), float(weight_decay)
        self.state, self.epochs = 0.0, 0
        _note('MLP', batch=batch, weight_decay=weight_decay, seed=seed, device=device, D=D, C=C)

    def set_data(self, X, y, Xv, yv):
        self.mean = float(np.abs(np.asarray(X, np.float64)).mean())
        _note('MLP.set_data', X, y, Xv, yv, dtypes=[str(np.asarray(a).dtype) for a in (X, y)])

    def epoch(self, perm, lr, t0):
        _note('MLP.epoch', lr=lr, t0=t0, perm=_sha(np.asarray(perm, np.int64)))
        t = self.epochs
        self.epochs += 1
        self.state = float(np.float32(1000.0 * lr + 100.0 * self.weight_decay + 0.01 * t))
        tilt = 0.001 * float(np.asarray(perm)[0] % 7)
        return dict(loss=1.0 / (1 + t) + self.mean + tilt, acc=1.0 - 1.0 / (2 + t), val_loss=0.3 * abs(t - 1) + 50.0 * lr + tilt,
                    val_acc=0.5 + 0.01 * t)

    def predict(self, x):
        _note('MLP.predict', x, state=self.state)
        return _row_scores(x, self.C, self.state)

    def get_weights(self):
        return [np.full(s, self.state, np.float32) for s in classifier._lib.mlp_shapes(self.D, self.C)]

    def set_weights(self, weights):
        self.state = float(np.asarray(weights[0]).flat[0])

    def close(self):
        pass


class FakeSVC(object):
    """svm.SVC without a GPU, picklable: the fit keeps two numbers of its rows, and every score is a fixed function of them and of
    the rows scored"""

    def __init__(self, C=1.0, **params):
        self.C, self.params = C, dict(sorted(params.items()))

    def fit(self, X, y):
        _note('SVC.fit', X, y, C=self.C, **self.params)
        return self._fitted(X, y)

    def _fitted(self, X, y):
        self.classes_ = np.unique(np.asarray(y))
        self.state_ = float(np.tanh(np.abs(np.asarray(X, np.float64)).mean()) + np.log10(self.C) / 10.0)
        self.rows_ = len(y)
        return self

    def decision_function(self, X):
        _note('SVC.decision_function', X, C=self.C)
        return _row_scores(X, max(3, len(self.classes_)), self.state_)[:, :len(self.classes_)]

    def predict(self, X):
        _note('SVC.predict', X, C=self.C)
        return self.classes_[_row_scores(X, max(3, len(self.classes_)), self.state_)[:, :len(self.classes_)].argmax(axis=1)]

    def predict_proba(self, X):
        _note('SVC.predict_proba', X, C=self.C)
        p = _row_scores(X, max(3, len(self.classes_)), self.state_)[:, :len(self.classes_)]
        return p / p.sum(axis=1, keepdims=True)

    def evaluate(self, X, y=None, file_idxs=None, outputs=('predict',)):
        _note('SVC.evaluate', X, y, C=self.C, outputs=list(outputs), file_idxs=_sha(None if file_idxs is None else np.asarray(file_idxs, np.int64)))
        scores = _row_scores(X, max(3, len(self.classes_)), self.state_)[:, :len(self.classes_)]
        got = {}
        if 'predict' in outputs:
            got['predict'] = self.classes_[scores.argmax(axis=1)]
        if 'hinge_loss' in outputs:
            got['hinge_loss'] = float(np.mean(1.0 - scores[np.arange(len(scores)), np.searchsorted(self.classes_, y)]))
        if 'file_predict' in outputs:
            got['file_predict'] = np.array([self.classes_[scores[s:e].mean(axis=0).argmax()] for s, e in file_idxs])
        return got


def fake_fit_grid(X, y, Cs, platt='device', max_entries=None, **params):
    _note('fit_grid', X, y, Cs=list(Cs), platt=platt, max_entries=max_entries, **params)
    return [FakeSVC(C=c, **params)._fitted(X, y) for c in Cs]


def install(set_attribute=setattr):
    """the stand-ins in place of the native classifiers, through the seams the drivers look up when they are called; a test passes
    monkeypatch.setattr"""
    set_attribute(classifier._lib, 'MLP', FakeMLP)
    set_attribute(classifier, 'SVC', FakeSVC)
    set_attribute(classifier._svm, 'fit_grid', fake_fit_grid)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
VALID_FOLD = dict(parameter_search=True)
CUT = dict(parameter_search=True, parameter_search_valid_fold=False, parameter_search_split_seed=4)
MLP = dict(train_batch_size=8, num_epochs=5, patience=0)
PREPROCESSING = [
    dict(feature_mode='framewise', use_min_max=False, non_overlap=False),
    dict(feature_mode='stats', use_min_max=True, non_overlap=False),
    dict(feature_mode='framewise', use_min_max=True, non_overlap=True, non_overlap_chunk_size=2),
    dict(feature_mode='stats', use_min_max=False, non_overlap=True, non_overlap_chunk_size=2),
    dict(feature_mode='framewise', use_min_max=False, non_overlap=True, non_overlap_chunk_size=3),
]


def cases():
    """name -> (driver, model type, seed of the global stream, keyword arguments)"""
    out = {}
    for model_type, own in (('mlp', MLP), ('svm', dict(C=2.0))):
        searches = [('no search', {}),
                    ('valid fold', dict(VALID_FOLD, parameter_search_train_with_valid=False)),
                    ('valid fold, retrained', dict(VALID_FOLD, parameter_search_train_with_valid=True)),
                    ('cut', dict(CUT, parameter_search_train_with_valid=False)),
                    ('cut, retrained', dict(CUT, parameter_search_train_with_valid=True))]
        for k, ((name, search), prep) in enumerate(zip(searches, PREPROCESSING)):
            args = dict(search, fold_num=1 + k % 5, random_state=7 + k, preprocess_device=None, **prep)
            if model_type == 'mlp' or not search:          # the SVM's search sets C itself
                args.update(own)
            out['%s: %s' % (model_type, name)] = ('fold', model_type, 100 + k, args)
        for name, fold_seed in (('fold_seed 5', 5), ('fold_seed None', None)):
            args = dict(CUT if fold_seed is None else VALID_FOLD, parameter_search_train_with_valid=True, folds=[1, 3],
                        fold_seed=fold_seed, preprocess_device=None, feature_mode='stats', use_min_max=True,
                        **(own if model_type == 'mlp' else {}))
            out['%s: cross_validate, %s' % (model_type, name)] = ('cross_validate', model_type, 200, args)
    return out


def _load(path):
    with open(path, 'rb') as fh:
        return pickle.load(fh)


def _fold_record(fold_dir, tree, out_dir):
    with open(os.path.join(fold_dir, 'config.json')) as fh:
        config = json.load(fh)
    keys = list(config)
    for k in ('model_dir', 'username'):
        config.pop(k)
    config['features_dir'] = os.path.relpath(config['features_dir'], tree)
    config['output_dir'] = os.path.relpath(config['output_dir'], out_dir)
    return {'config': config, 'config_keys': keys, 'files': sorted(os.listdir(fold_dir)),
            'results': _plain(_load(os.path.join(fold_dir, 'results.pkl')))}


def run_case(case, tree, out_dir):
    """runs one of cases() on the tree into out_dir -> its whole record, in JSON types, with every path relative to one of the two
    (condensed() gives the form that is committed)"""
    driver, model_type, seed, args = case
    args = dict(args)
    out_dir = str(out_dir)
    del LOG[:]
    np.random.seed(seed)
    if driver == 'cross_validate':
        top = classifier.cross_validate(tree, str(out_dir), model_type=model_type, **args)
        results = _load(os.path.join(top, 'results.pkl'))
        fold_dirs = results.pop('fold_dirs')
        record = {'files': sorted(os.listdir(top)), 'results': _plain(results), 'folds': [_fold_record(d, tree, out_dir) for d in fold_dirs],
                  'fold_dirs': [os.path.relpath(os.path.dirname(d), out_dir) for d in fold_dirs]}
    else:
        fold_num = args.pop('fold_num')
        if model_type == 'mlp':
            fold_dir = classifier.train(tree, str(out_dir), fold_num, model_type='mlp', **args)
        else:
            fold_dir = classifier.train_svm_fold(tree, str(out_dir), fold_num, **args)
        record = {'folds': [_fold_record(fold_dir, tree, out_dir)], 'fold_dirs': [os.path.relpath(os.path.dirname(fold_dir), out_dir)]}
    state = np.random.get_state()
    record['numpy_state'] = hashlib.sha256(state[1].tobytes() + repr(state[2:]).encode()).hexdigest()
    record['calls'] = list(LOG)
    del LOG[:]
    return json.loads(json.dumps(record))


def _digest(part):
    return hashlib.sha256(json.dumps(part, sort_keys=True, separators=(',', ':')).encode()).hexdigest()


def _results_digest(results):
    shown = {part: results[part].get('accuracy') for part in ('train', 'valid', 'test') if isinstance(results.get(part), dict)}
    if isinstance(results.get('train'), dict) and 'search_params_best_values' in results['train']:
        shown['best'] = results['train']['search_params_best_values']
    return dict(shown, sha256=_digest(results))


def condensed(record):
    """A whole record in the form that tests/golden/fold_driver_record.json holds, small enough to read: every results.pkl and the
    log of the stand-ins' calls as the SHA-256 of their canonical JSON (equal digests: equal parts, floats and NaN included), next
    to what a reader wants to see of them -- the accuracies and the chosen point, and the order of the calls with their row
    counts (train+valid), a repeated block of calls written once with its count.  config.json, the key order, the files and the directories stay as they are."""
    out = dict(record, folds=[dict(f, results=_results_digest(f['results'])) for f in record['folds']])
    if 'results' in record:
        out['results'] = {'folds': record['results']['folds'], 'sha256': _digest(record['results'])}
    steps = ['%s %s+%s' % (c['call'], c['train_rows'], c['valid_rows']) if c['train_rows'] is not None else c['call']
             for c in record['calls']]
    order, i = [], 0
    while i < len(steps):          # a block of up to 8 calls that follows itself is written once, with its count
        size, times = 1, 1
        for b in range(1, 9):
            n = 1
            while steps[i + n * b:i + (n + 1) * b] == steps[i:i + b]:
                n += 1
            if n > 1 and n * b > size * times:
                size, times = b, n
        order.append(steps[i] if size * times == 1 else [times, steps[i:i + size]])
        i += size * times
    out['calls'] = {'count': len(record['calls']), 'order': order, 'sha256': _digest(record['calls'])}
    return out
