"""The downstream sound classifier trained on L3 embeddings: the reference's classifier/train.py (construct_mlp_model :230-257,
train_mlp :260-391, train_param_search :394-492, train :495-709 for model_type='mlp') and classifier/metrics.py:8-46.

The MLP trains on the GPU through the l3_mlp handle of libl3hip (csrc/mlp.hip); everything here is the Keras-shaped shell around
it.  Deviations from the reference, all deliberate:
  * the epoch shuffle is drawn from np.random.RandomState(random_state) (the reference's seeding is commented out, so its runs
    are not reproducible); the Glorot initialisation is seeded with random_state too;
  * the random start delay and the Google Sheets logging of train() are skipped; config.json has git_commit None;
  * the scalers are pickled with `pickle` (the reference uses sklearn's joblib; these are NumPy restatements, usc.py);
  * the random forest (train_rf, classifier/train.py:169-227) trains and predicts on the GPU as a level-wise histogram forest
    (forest.py, csrc/forest.hip), not as sklearn's exact-split trees: forest.py's header lists how it differs.  train_rf does not
    seed NumPy's and Python's global generators (the reference does; every draw here has its own RandomState), pickles the model
    with `pickle`, and takes usc.DeviceFeatures as they are.  train() and cross_validate still refuse 'rf'; train_rf_fold is the
    reference's train(model_type='rf') without a parameter search (with one it raises), and train_rf_search / train_rf_search_fold
    are its parameter search over n_estimators (:623-630) fitted in one pass: one forest of the largest size, whose first n trees
    are the forest of n trees (forest.py), scored at every size of the grid in one pass over each split
    (RandomForestClassifier.evaluate); every metric and the chosen size equal the loop's.  model_dir/model.pkl holds the returned
    model there (the loop over train_rf leaves the one it fitted last);
  * the parameter search without a validation fold (train_param_search :408-423, :470-479) cuts the training rows with
    usc.stratified_shuffle_split, a NumPy restatement of sklearn's StratifiedShuffleSplit, and only when the caller gives the
    split's seed (split_random_state / parameter_search_split_seed; the reference passes none, so its split differs from run to
    run): without a seed it raises as before.  Rows on the GPU are cut there (DeviceFeatures.split, one kernel) and stay there;
  * cross_validate runs every fold of a dataset in one call from folds read once (usc.FoldBank) and summarises them with
    aggregate_metrics (classifier/metrics.py:49-78); the reference runs one job per fold;
  * the SVM (train_svm, classifier/train.py:79-166) trains on the GPU (svm.py, csrc/svm.hip); its probability estimates draw the
    cross-validation fold permutation from np.random.RandomState(random_state) as the MLP's shuffle does (libsvm uses rand()),
    and the model is pickled with `pickle` (the reference uses joblib).  train() still runs only the MLP; train_svm_fold is
    the reference's train(model_type='svm'), and train_svm_search its parameter search over C with the whole grid fitted in
    one pass on the GPU (svm.fit_grid);
  * train_mlp_search / train_mlp_search_fold are the MLP's parameter search over learning rate and weight decay
    (classifier/train.py:638-651; MLP_SEARCH_SPACE) with the grid fitted as one group of models on the GPU (fit_mlp_grid over an
    _lib.MLPGroup: the rows resident once, every live point in the same seven launches per step, train_mlp's checkpoint and
    early-stopping rules per point): every metric, history, search record, the chosen point, the returned weights and
    history_csvlog.csv equal the loop of train_mlp over the grid bit for bit.  model_dir/model.h5 holds the returned model there
    (the loop leaves the checkpoint of the run it made last).  train(parameter_search=True) and cross_validate still run the loop;
  * train_knn / train_knn_search (and their folds, train_knn_fold / train_knn_search_fold) are not in the reference: a k-nearest-
    neighbour classifier on the frozen features (knn.py, csrc/knn.hip), with train_rf's conventions.  Nothing is trained, so the
    training metrics are leave-one-row-out; the search over k scores every size from one query at the largest.  train() and
    cross_validate refuse 'knn' as they refuse every type but the MLP.

How the file is put together: train, train_svm_fold, train_rf_fold and cross_validate pass their arguments, by name in one dict, to
one fold driver (_run_fold), and the model types differ in one function each (_mlp_part, _svm_part, _rf_part; train_rf_search_fold,
train_mlp_search_fold, train_knn_fold and train_knn_search_fold hand the driver their own, _rf_search_part, _mlp_search_part,
_knn_part and _knn_search_part).  train_param_search, train_svm_search,
train_rf_search and train_mlp_search are one search body (_search) with four ways to fit the grid.  A usc.DeviceFeatures is closed by whoever made it, through _closing: the
driver closes the fold's splits, a search the parts of its cut and its merged matrix, and nobody what a caller passed in.
"""
import contextlib
import datetime
import functools
import getpass
import json
import logging
import os
import pickle as pk
from itertools import product

import numpy as np

from . import _lib, callbacks, kerasfile
from . import svm as _svm
from .forest import FITTED_ROWS, RandomForestClassifier
from .knn import KNeighborsClassifier
from .svm import SVC, hinge_loss  # noqa: F401  (re-exported: the reference imports them into classifier/train.py)
from .usc import DeviceFeatures, FoldBank, get_split, preprocess_split_data, stratified_shuffle_split

LOGGER = logging.getLogger('classifier')

DATASET_NUM_CLASSES = {
    'us8k': 10,
    'esc50': 50,
    'dcase2013': 10,
}

ONLY_MLP = ('only the mlp classifier is built (model_type {!r}: the fold driver runs the MLP alone; classifier.train_svm trains '
            'the SVM on the GPU, and the random forest is not built)')
NO_SSS = ('the parameter search without a validation fold needs sklearn\'s StratifiedShuffleSplit, which is not built: '
          'search on the validation fold instead')
NO_RF_SEARCH = ('the parameter search of the random forest (over n_estimators, classifier/train.py:623-630) is not built: run '
                'train_rf_fold once per n_estimators instead')


class EarlyStopping(callbacks.Callback):
    """[3P] keras.callbacks.EarlyStopping of keras 2.0.x (monitor 'val_loss', mode min, min_delta 0): the wait counter is tested
    BEFORE it is incremented, so training stops at the end of the (patience + 1)-th epoch in a row without improvement."""

    def __init__(self, monitor='val_loss', patience=0, min_delta=0.0):
        self.monitor, self.patience, self.min_delta = monitor, int(patience), abs(min_delta)

    def on_train_begin(self, logs=None):
        self.wait = 0
        self.stopped_epoch = 0
        self.best = np.inf

    def on_epoch_end(self, epoch, logs=None):
        current = (logs or {}).get(self.monitor)
        if current is None:
            return
        if current + self.min_delta < self.best:
            self.best = current
            self.wait = 0
        else:
            if self.wait >= self.patience:
                self.stopped_epoch = epoch
                self.model.stop_training = True
            self.wait += 1


class MetricCallback(callbacks.Callback):
    """train.py:46-80: the per-epoch loss / accuracy series train_mlp reports."""

    SERIES = (('train_loss', 'loss'), ('train_acc', 'acc'), ('valid_loss', 'val_loss'), ('valid_acc', 'val_acc'))

    def __init__(self, valid_data=None, verbose=False):
        self.valid_data, self.verbose = valid_data, verbose

    def on_train_begin(self, logs=None):
        for attr, _ in self.SERIES:
            setattr(self, attr, [])

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        for attr, key in self.SERIES:
            getattr(self, attr).append(logs.get(key))
        if self.verbose:
            LOGGER.info('epoch %d: %s', epoch, ', '.join('%s %.6f' % (k, logs[k]) for _, k in self.SERIES if k in logs))


class MLPModel(object):
    """What train_mlp uses of the Keras Model construct_mlp_model returns: compile / fit / predict / save_weights /
    load_weights / get_weights / set_weights.  The state lives on the GPU (an l3_mlp handle, created for the batch size of the
    first fit); the Adam step count and moments carry over between fit calls as Keras' optimizer state does, so a later fit
    must use the same batch size (a different one raises ValueError once the model has trained)."""

    name = 'urban_sound_classifier'

    def __init__(self, input_dim, weight_decay=1e-5, num_classes=10, seed=0, device=0):
        self.input_dim, self.weight_decay, self.num_classes = int(input_dim), float(weight_decay), int(num_classes)
        self.seed, self.device = int(seed), device
        self.lr = 1e-3
        self.stop_training = False
        self.iterations = 0
        self._h = None
        self._weights = None

    def _handle(self, batch=64):
        if self._h is not None and self._h.batch != batch and self.iterations > 0:
            # a new handle would carry the weights over but start Adam's moments from zero, which Keras never does
            raise ValueError('this model trained with batch size %d; fitting with batch size %d would reset its optimizer '
                             'state' % (self._h.batch, batch))
        if self._h is None or self._h.batch != batch:
            weights = self.get_weights() if (self._h is not None or self._weights is not None) else None
            if self._h is not None:
                self._h.close()
            self._h = _lib.MLP(self.input_dim, self.num_classes, batch, weight_decay=self.weight_decay, seed=self.seed,
                               device=self.device)
            if weights is not None:
                self._h.set_weights(weights)
            self._weights = None
        return self._h

    def compile(self, optimizer=None, loss='categorical_crossentropy', metrics=None, lr=None):
        if loss != 'categorical_crossentropy':
            raise ValueError('only categorical_crossentropy is built')
        if lr is None:
            lr = getattr(optimizer, 'lr', 1e-3) if optimizer is not None else 1e-3
        self.lr = float(lr)

    def get_weights(self):
        if self._h is None and self._weights is not None:
            return [w.copy() for w in self._weights]
        return self._handle().get_weights() if self._h is None else self._h.get_weights()

    def set_weights(self, weights):
        if self._h is None:
            shapes = _lib.mlp_shapes(self.input_dim, self.num_classes)
            if [tuple(np.shape(w)) for w in weights] != shapes:
                raise ValueError('weight shapes %s, expected %s' % ([np.shape(w) for w in weights], shapes))
            self._weights = [np.asarray(w, np.float32).copy() for w in weights]
        else:
            self._h.set_weights(weights)

    def save_weights(self, filepath, overwrite=True):
        kerasfile.save_dense_weights(filepath, self.get_weights())

    def load_weights(self, filepath):
        self.set_weights(kerasfile.load_dense_weights(filepath))

    def predict(self, x, batch_size=None, verbose=0):
        h = self._handle(self._h.batch if self._h is not None else 64)
        return h.predict_dev(x.handle) if isinstance(x, DeviceFeatures) else h.predict(x)

    def predict_files(self, x, file_idxs):
        """-> (file_proba (F, C) float32, file_predict (F,)): the mean of predict(x)[s:e] of each file_idxs entry and its arg-max,
        _file_predictions' bits.  x: a usc.DeviceFeatures; the (n, C) probabilities never leave the GPU (l3_mlp_predict_files_dev)."""
        if not isinstance(x, DeviceFeatures):
            raise TypeError('predict_files takes a usc.DeviceFeatures; on host rows use predict and _file_predictions')
        h = self._handle(self._h.batch if self._h is not None else 64)
        mean, pred = h.predict_files_dev(x.handle, np.asarray(file_idxs, np.int64).reshape(-1, 2))
        return mean, pred.astype(np.int64)

    def fit(self, x, y, batch_size=64, epochs=1, verbose=0, callbacks=None, validation_split=0.0, validation_data=None,
            shuffle=True, random_state=None):
        """keras Model.fit with shuffle=True: y one-hot (n, C); validation_split takes the LAST fraction of x before any
        shuffling (split_at = int(n * (1 - validation_split))).  -> {'loss': [...], 'acc': [...], 'val_loss': ..., 'val_acc': ...}

        x (and the validation features) may be usc.DeviceFeatures: their rows are then copied on the device into the model's
        own matrices, validation_split slicing by row range."""
        on_device = isinstance(x, DeviceFeatures)
        if not on_device:
            x = np.asarray(x, np.float32)
        labels = np.argmax(np.asarray(y), axis=1).astype(np.int32)
        n_train = len(x)
        # the split: the training rows are x[:n_train]; the validation rows are vx[vlo:vhi], of the held-out matrix or of x itself
        vx, vlo, vhi, vy = None, 0, 0, None
        if validation_data is not None:
            vx = validation_data[0]
            if not isinstance(vx, DeviceFeatures):
                vx = DeviceFeatures(np.asarray(vx, np.float32), x.device) if on_device else np.asarray(vx, np.float32)
            vhi = len(vx)
            vy = np.argmax(np.asarray(validation_data[1]), axis=1).astype(np.int32)
        elif validation_split and 0.0 < validation_split < 1.0:
            n_train = int(len(x) * (1.0 - validation_split))
            vx, vlo, vhi, vy = x, n_train, len(x), labels[n_train:]
            labels = labels[:n_train]
        h = self._handle(int(batch_size))
        if on_device:
            h.set_data_dev(x.handle, 0, n_train, labels, None if vx is None else vx.handle, vlo, vhi, vy)
        else:
            h.set_data(x[:n_train], labels, None if vx is None else vx[vlo:vhi], vy)

        rs = np.random.RandomState(random_state)
        cbs = list(callbacks or [])
        for cb in cbs:
            cb.set_model(self)
            cb.set_params({'epochs': epochs, 'batch_size': batch_size, 'samples': n_train})
        history = {}
        self.stop_training = False
        for cb in cbs:
            cb.on_train_begin()
        steps = -(-n_train // int(batch_size))
        for epoch in range(int(epochs)):
            for cb in cbs:
                cb.on_epoch_begin(epoch)
            perm = rs.permutation(n_train) if shuffle else np.arange(n_train)
            logs = h.epoch(perm, self.lr, self.iterations)
            self.iterations += steps
            if vy is None:
                logs = {k: logs[k] for k in ('loss', 'acc')}
            for k, v in logs.items():
                history.setdefault(k, []).append(v)
            if verbose:
                LOGGER.info('Epoch %d/%d - %s', epoch + 1, epochs, ' - '.join('%s: %.4f' % kv for kv in sorted(logs.items())))
            for cb in cbs:
                cb.on_epoch_end(epoch, dict(logs))
            if self.stop_training:
                break
        for cb in cbs:
            cb.on_train_end()
        return history


def construct_mlp_model(input_shape, weight_decay=1e-5, num_classes=10, seed=0):
    """train.py:230-257: Dense(512, relu) -> Dense(128, relu) -> Dense(num_classes, softmax), l2(weight_decay) on each kernel.
    -> (model, input_shape, output_shape)"""
    m = MLPModel(int(np.prod(input_shape)), weight_decay=weight_decay, num_classes=num_classes, seed=seed)
    return m, tuple(input_shape), (num_classes,)


def one_hot(labels, num_classes):
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    out = np.zeros((labels.size, num_classes))
    out[np.arange(labels.size), labels] = 1.0
    return out


def _class_indices(a):
    """class indices from labels, one-hot rows or probability rows"""
    a = np.asarray(a)
    return a.argmax(axis=1) if a.ndim == 2 else a


def compute_metrics(y, pred, num_classes=10):
    """classifier/metrics.py:8-46: overall accuracy, the accuracy within each true class (NaN for a class with no example)
    and their unweighted mean.  y and pred may be indices or (n, C) rows."""
    truth, guess = _class_indices(y), _class_indices(pred)
    hit = truth == guess
    per_class = []
    for c in range(num_classes):
        members = truth == c
        per_class.append(hit[members].mean() if members.any() else np.nan)
    return {'accuracy': hit.mean(), 'class_accuracy': per_class, 'average_class_accuracy': np.mean(per_class)}


def aggregate_metrics(fold_metrics):
    """classifier/metrics.py:49-78: the folds' values of every key of the FIRST fold's metrics -> {key: {'mean', 'var', 'min',
    '25_%ile', '75_%ile', 'median', 'max'}}, each as NumPy gives it over the list of the folds' values (a list-valued metric such
    as class_accuracy is reduced over all its entries)."""
    keys = list(fold_metrics[0].keys())
    out = {}
    for k in keys:
        values = [fold[k] for fold in fold_metrics]
        out[k] = {'mean': np.mean(values), 'var': np.var(values), 'min': np.min(values), '25_%ile': np.percentile(values, 25),
                  '75_%ile': np.percentile(values, 75), 'median': np.median(values), 'max': np.max(values)}
    return out


def _series_metrics(series, at):
    """loss / accuracy at the checkpoint epoch and their whole histories, from a MetricCallback's two series"""
    loss, acc = series
    return {'loss': loss[at], 'loss_history': list(loss), 'accuracy': acc[at], 'accuracy_history': list(acc)}


def _file_predictions(frame_probs, file_idxs):
    """one class per file: the argmax of the mean of its frames' probabilities"""
    return np.array([frame_probs[s:e].mean(axis=0).argmax() for s, e in file_idxs])


def train_mlp(train_data, valid_data, test_data, model_dir, batch_size=64, num_epochs=100, valid_split=0.15, patience=20,
              learning_rate=1e-4, weight_decay=1e-5, num_classes=10, random_state=12345678, verbose=False, **kwargs):
    """classifier/train.py:260-391 -> (model, train_metrics, valid_metrics, test_metrics).  With a validation split the
    last `valid_split` of the training rows validate (keras validation_split); with one, valid_split is ignored."""
    features = train_data['features']
    targets = one_hot(train_data['labels'], num_classes)
    held_out = None
    if valid_data:
        held_out = (valid_data['features'], one_hot(valid_data['labels'], num_classes))

    model, _, _ = construct_mlp_model(features.shape[1:], weight_decay=weight_decay, num_classes=num_classes,
                                      seed=random_state)
    best_path = os.path.join(model_dir, 'model.h5')
    series = MetricCallback(valid_data, verbose=verbose)
    hooks = [callbacks.ModelCheckpoint(best_path, monitor='val_loss', save_best_only=True, save_weights_only=True),
             EarlyStopping(monitor='val_loss', patience=patience),
             callbacks.LossHistory(os.path.join(model_dir, 'history_checkpoint.pkl')),
             callbacks.CSVLogger(os.path.join(model_dir, 'history_csvlog.csv'), separator=',', append=True),
             series]
    model.compile(lr=learning_rate)
    model.fit(features, targets, batch_size=batch_size, epochs=num_epochs, callbacks=hooks, validation_data=held_out,
              validation_split=0.0 if held_out is not None else valid_split, verbose=2 if verbose else 0,
              random_state=random_state)

    # back to the lowest-val_loss checkpoint; its epoch is the first minimum of the series
    model.load_weights(best_path)
    best = int(np.argmin(series.valid_loss))

    train_metrics = _series_metrics((series.train_loss, series.train_acc), best)
    on_train = compute_metrics(targets, model.predict(features), num_classes=num_classes)
    train_metrics['class_accuracy'] = on_train['class_accuracy']
    train_metrics['average_class_accuracy'] = on_train['average_class_accuracy']
    valid_metrics = _series_metrics((series.valid_loss, series.valid_acc), best)
    if held_out is not None:
        valid_metrics.update(compute_metrics(held_out[1], model.predict(held_out[0]), num_classes=num_classes))
    test_metrics = {}
    if test_data:
        per_file = _file_predictions(model.predict(test_data['features']), test_data['file_idxs'])
        test_metrics = compute_metrics(test_data['labels'], per_file, num_classes=num_classes)
    return model, train_metrics, valid_metrics, test_metrics


def train_svm(train_data, valid_data, test_data, model_dir, C=1.0, kernel='rbf', num_classes=10, tol=0.001, max_iterations=-1,
              verbose=False, random_state=12345678, evaluate_on_device=False, **kwargs):
    """classifier/train.py:79-166 -> (model, train_metrics, valid_metrics, test_metrics): SVC(C, kernel, tol, max_iter,
    probability=True, random_state) fitted on the GPU and pickled to model_dir/model.pkl; 'loss' is sklearn's hinge loss of the
    (ovr) decision values; the test set is classified per file as the argmax of the mean of its frames' predict_proba.
    evaluate_on_device: the splits stay as they are (usc.DeviceFeatures are not downloaded) and each is scored by one
    SVC.evaluate on the GPU (_svm_metrics_on_device); the same four values come back.  That path reads the classes off the fitted
    model (clf.classes_) where the default one passes labels=np.arange(num_classes) to hinge_loss: the two agree when every class of
    range(num_classes) occurs in the training split, and a validation label the training split lacks is a ValueError there."""
    if not evaluate_on_device:
        train_data, valid_data, test_data = (_on_host(d) for d in (train_data, valid_data, test_data))
    features, labels = train_data['features'], train_data['labels']
    clf = SVC(C=C, probability=True, kernel=kernel, max_iter=max_iterations, tol=tol, random_state=random_state, verbose=verbose)
    LOGGER.debug('Fitting model to data...')
    clf.fit(features, labels)
    LOGGER.info('Saving model...')
    _dump(os.path.join(model_dir, 'model.pkl'), clf)
    if evaluate_on_device:
        return (clf,) + _svm_metrics_on_device(clf, train_data, valid_data, test_data, num_classes)

    classes = np.arange(num_classes)
    train_metrics = compute_metrics(labels, clf.predict(features), num_classes=num_classes)
    train_metrics['loss'] = hinge_loss(labels, clf.decision_function(features), labels=classes)
    LOGGER.info('Train - hinge loss: %s, acc: %s', train_metrics['loss'], train_metrics['accuracy'])
    valid_metrics = {}
    if valid_data:
        vx, vy = valid_data['features'], valid_data['labels']
        valid_metrics = compute_metrics(vy, clf.predict(vx), num_classes=num_classes)
        valid_metrics['loss'] = hinge_loss(vy, clf.decision_function(vx), labels=classes)
        LOGGER.info('Valid - hinge loss: %s, acc: %s', valid_metrics['loss'], valid_metrics['accuracy'])
    test_metrics = {}
    if test_data:
        per_file = _file_predictions(clf.predict_proba(test_data['features']), test_data['file_idxs'])
        test_metrics = compute_metrics(test_data['labels'], per_file, num_classes=num_classes)
    return clf, train_metrics, valid_metrics, test_metrics


def train_rf(train_data, valid_data, test_data, model_dir, n_estimators=100, num_classes=10, random_state=12345678, **kwargs):
    """classifier/train.py:169-227 -> (model, train_metrics, valid_metrics, test_metrics): forest.RandomForestClassifier(
    n_estimators, random_state) fitted on the GPU and pickled to model_dir/model.pkl; 'loss' is 0 as in the reference; the test set
    is classified per file as the argmax of the mean of its frames' predict_proba, taken on the host over the downloaded (n, C)
    matrix.  The splits' features may be NumPy rows or usc.DeviceFeatures (fitted and scored where they are).  Of kwargs the
    forest's own arguments are passed on (RF_ARGS); the rest is ignored, as the reference ignores it."""
    features, labels = train_data['features'], train_data['labels']
    forest_args = {k: kwargs[k] for k in RF_ARGS if k in kwargs}
    if isinstance(features, DeviceFeatures):
        forest_args.setdefault('device', features.device)
    clf = RandomForestClassifier(n_estimators=n_estimators, random_state=random_state, **forest_args)
    LOGGER.debug('Fitting model to data...')
    clf.fit(features, labels)
    LOGGER.info('Saving model...')
    _dump(os.path.join(model_dir, 'model.pkl'), clf)

    train_metrics = compute_metrics(labels, clf.predict(features), num_classes=num_classes)
    train_metrics['loss'] = 0
    LOGGER.info('Train - acc: %s', train_metrics['accuracy'])
    valid_metrics = {}
    if valid_data:
        valid_metrics = compute_metrics(valid_data['labels'], clf.predict(valid_data['features']), num_classes=num_classes)
        valid_metrics['loss'] = 0
        LOGGER.info('Valid - acc: %s', valid_metrics['accuracy'])
    test_metrics = {}
    if test_data:
        per_file = _file_predictions(clf.predict_proba(test_data['features']), test_data['file_idxs'])
        test_metrics = compute_metrics(test_data['labels'], per_file, num_classes=num_classes)
    return clf, train_metrics, valid_metrics, test_metrics


# the arguments of forest.RandomForestClassifier that train_rf passes on from its keyword arguments
RF_ARGS = ('max_depth', 'min_samples_split', 'min_samples_leaf', 'max_features', 'bin_sample', 'device', 'wide_min_rows')


def _svm_metrics_on_device(clf, train_data, valid_data, test_data, num_classes):
    """-> (train_metrics, valid_metrics, test_metrics) of a fitted SVC, one SVC.evaluate per split: predictions and the hinge loss
    of the train and validation rows (no (n, C) array returns), the per-file classes of the test set"""
    metrics = []
    for name, data in (('Train', train_data), ('Valid', valid_data)):
        if not data:
            metrics.append({})
            continue
        got = clf.evaluate(data['features'], y=data['labels'], outputs=('predict', 'hinge_loss'))
        m = compute_metrics(data['labels'], got['predict'], num_classes=num_classes)
        m['loss'] = got['hinge_loss']
        LOGGER.info('%s - hinge loss: %s, acc: %s', name, m['loss'], m['accuracy'])
        metrics.append(m)
    test_metrics = {}
    if test_data:
        per_file = clf.evaluate(test_data['features'], file_idxs=test_data['file_idxs'], outputs=('file_predict',))['file_predict']
        test_metrics = compute_metrics(test_data['labels'], per_file, num_classes=num_classes)
    return metrics[0], metrics[1], test_metrics


# ---- who owns a feature matrix ----------------------------------------------------------------------------------------------------
# A split is {'features', 'labels', ...}; its features are a NumPy array or a usc.DeviceFeatures, which holds device memory until it
# is closed.  Whoever makes a DeviceFeatures closes it, once, through _closing: the fold driver the splits it obtained (whatever
# their features are by then: the preprocessing uploads arrays), a search the two parts of its cut and its merged matrix.  What a
# caller passes in is the caller's.
@contextlib.contextmanager
def _closing(splits):
    """the splits, for the length of a with block; on the way out the DeviceFeatures that they hold by then are closed"""
    try:
        yield splits
    finally:
        for d in splits:
            if d and isinstance(d.get('features'), DeviceFeatures):
                d['features'].close()


def _on_host(data):
    """the split with its features as a NumPy array (downloaded if preprocess_split_data left them on the device)"""
    if data and isinstance(data['features'], DeviceFeatures):
        data = dict(data, features=data['features'].to_host())
    return data


def _require_split_seed(search_on_cut, seed):
    """the one refusal of the search without a validation fold: it needs the seed of its cut"""
    if search_on_cut and seed is None:
        raise ValueError(NO_SSS)


def _cut_for_search(train_data, valid_ratio, split_random_state):
    """classifier/train.py:412-423 -> (search part, validation part), {'features', 'labels'} each: the training rows cut by
    usc.stratified_shuffle_split(labels, valid_ratio, split_random_state).  A DeviceFeatures is cut on its GPU by one
    DeviceFeatures.split into two new ones (the caller owns them), a NumPy array by indexing: the same bits."""
    labels = np.asarray(train_data['labels'])
    train_idx, valid_idx = stratified_shuffle_split(labels, valid_ratio, split_random_state)
    features = train_data['features']
    if isinstance(features, DeviceFeatures):
        kept, held = features.split(train_idx, valid_idx)
    else:
        kept, held = features[train_idx], features[valid_idx]
    return {'features': kept, 'labels': labels[train_idx]}, {'features': held, 'labels': labels[valid_idx]}


@contextlib.contextmanager
def _merged_and_shuffled(train_data, valid_data):
    """classifier/train.py:476-479: train + valid as one split, shuffled by one np.random.permutation (the global state), for the
    length of a with block.  Two DeviceFeatures on one GPU are stacked and shuffled there into a new one (one copy kernel, one
    gather; closed on the way out), anything else on the host: the same bits."""
    labels = np.concatenate((train_data['labels'], valid_data['labels']))
    mix = np.random.permutation(labels.size)
    tx, vx = train_data['features'], valid_data['features']
    resident = isinstance(tx, DeviceFeatures) and isinstance(vx, DeviceFeatures) and tx.device == vx.device
    if resident:
        stacked = DeviceFeatures.assemble([(tx, 0, len(tx)), (vx, 0, len(vx))], device=tx.device)
    else:
        stacked = np.vstack((_on_host(train_data)['features'], _on_host(valid_data)['features']))[mix]
    with _closing(({'features': stacked, 'labels': labels[mix]},)) as (merged,):
        if resident:
            stacked.handle.gather(mix)
        yield merged


def _search(train_data, valid_data, names, valid_ratio, split_random_state, train_with_valid, run_grid, refit):
    """The body of both parameter searches (classifier/train.py:394-492) -> (model, train_metrics, valid_metrics, test_metrics).
    With a validation fold the grid runs on (train_data, valid_data); without one (valid_data None) on the two parts of
    _cut_for_search, which needs split_random_state (None refuses, NO_SSS).  The point with the best validation accuracy is kept,
    the first one on ties.  train_with_valid then refits it without validation data: after a cut on the whole of train_data as it
    is (:471-474), else on train + valid shuffled together; without train_with_valid the chosen run stands.
    run_grid(search_train, search_valid) -> [(point, model, train metrics, valid metrics, test metrics)] in grid order;
    refit(point, data) -> (model, train metrics, test metrics); names: the searched parameters, in the order of a point's values."""
    _require_split_seed(not valid_data, split_random_state)
    with contextlib.ExitStack() as made:          # what the search makes: closed when it ends, however it ends
        searched = (train_data, valid_data) if valid_data else made.enter_context(
            _closing(_cut_for_search(train_data, valid_ratio, split_random_state)))
        runs = run_grid(*searched)
        chosen = runs[int(np.argmax([run[3]['accuracy'] for run in runs]))]
        point = chosen[0]
        LOGGER.info('Chosen %s (validation accuracy %s)', dict(zip(names, point)), chosen[3]['accuracy'])
        if not train_with_valid:
            model, train_metrics, test_metrics = chosen[1], dict(chosen[2]), chosen[4]
        elif valid_data:
            model, train_metrics, test_metrics = refit(point, made.enter_context(_merged_and_shuffled(train_data, valid_data)))
        else:
            model, train_metrics, test_metrics = refit(point, train_data)

    search_record = {'search_params': names, 'search_params_best_values': point}
    train_metrics.update(search_record, search={run[0]: run[2] for run in runs})
    valid_metrics = dict(chosen[3])
    valid_metrics.update(search_record, search={run[0]: run[3] for run in runs})
    return model, train_metrics, valid_metrics, test_metrics


def train_param_search(train_data, valid_data, test_data, model_dir, train_func, search_space, valid_ratio=0.15,
                       train_with_valid=True, split_random_state=None, **kwargs):
    """classifier/train.py:394-492: train_func once per point of the grid (the product of the search_space values, in key
    order), keep the point with the best validation accuracy (the first one on ties), then either retrain with no validation
    data (train_with_valid) or keep that run.  With a validation fold the search runs on (train, valid) and the retrain on the two
    shuffled together (on the GPU when both are usc.DeviceFeatures there).  Without one (valid_data None) the reference cuts
    valid_ratio of the training rows off with sklearn's StratifiedShuffleSplit: split_random_state, an int, is the seed of that cut
    (_cut_for_search), the search runs on its two parts, the retrain on the whole of train_data as it is, and the parts are closed
    at the end; None refuses (NO_SSS)."""
    names = list(search_space)

    def fit(point, train, valid):
        kwargs.update(zip(names, point))
        return tuple(train_func(train, valid, test_data, model_dir, **kwargs))

    def run_grid(search_train, search_valid):
        runs = []
        for point in product(*(search_space[n] for n in names)):
            LOGGER.info('Search point %s', dict(zip(names, point)))
            runs.append((point,) + fit(point, search_train, search_valid))
        return runs

    def refit(point, data):
        model, train_metrics, _, test_metrics = fit(point, data, None)
        return model, train_metrics, test_metrics

    return _search(train_data, valid_data, names, valid_ratio, split_random_state, train_with_valid, run_grid, refit)


SVM_SEARCH_CS = (0.1, 1, 10, 100, 1000)        # classifier/train.py:609


def train_svm_search(train_data, valid_data, test_data, model_dir, Cs=SVM_SEARCH_CS, train_with_valid=False, platt='device', C=None,
                     kernel='rbf', num_classes=10, tol=0.001, max_iterations=-1, verbose=False, random_state=12345678,
                     max_entries=None, valid_ratio=0.15, split_random_state=None, **kwargs):
    """train_param_search(..., train_func=train_svm, search_space={'C': Cs}, evaluate_on_device=True) with the grid fitted in one
    pass: one svm.fit_grid over the training split (NumPy rows or usc.DeviceFeatures, resident once), one SVC.evaluate per split
    and model, the cost with the best validation accuracy (the first one on ties), and with train_with_valid the retrain on
    train + valid shuffled together (np.random.permutation as there; two usc.DeviceFeatures on one GPU are merged and shuffled
    there, anything else on the host: the same bits).  -> the same tuple (model, train_metrics,
    valid_metrics, test_metrics) with the same search records.  platt: svm.fit_grid's ('host': Platt's sigmoids as SVC.fit
    fits them, so every number equals that of the separate fits).  model_dir/model.pkl holds the returned model (the loop over
    train_svm leaves the one it fitted last there).  C is ignored (the search sets it); the other arguments are train_svm's.
    Without a validation fold (valid_data None): train_param_search's cut of valid_ratio of the training rows, seeded by
    split_random_state (None refuses, NO_SSS); the grid is fitted and scored on its two parts, and train_with_valid refits the
    chosen cost on the whole of train_data as it is."""
    Cs = list(Cs)

    def fit(data, costs):
        return _svm.fit_grid(data['features'], data['labels'], costs, platt=platt, max_entries=max_entries, probability=True,
                             kernel=kernel, max_iter=max_iterations, tol=tol, random_state=random_state, verbose=verbose)

    def run_grid(search_train, search_valid):
        LOGGER.info('Fitting the grid C = %s', Cs)
        runs = []
        for c, clf in zip(Cs, fit(search_train, Cs)):
            LOGGER.info('Search point %s', {'C': c})
            runs.append(((c,), clf) + _svm_metrics_on_device(clf, search_train, search_valid, test_data, num_classes))
        return runs

    def refit(point, data):
        model = fit(data, [point[0]])[0]
        train_metrics, _, test_metrics = _svm_metrics_on_device(model, data, None, test_data, num_classes)
        return model, train_metrics, test_metrics

    outcome = _search(train_data, valid_data, ['C'], valid_ratio, split_random_state, train_with_valid, run_grid, refit)
    LOGGER.info('Saving model...')
    _dump(os.path.join(model_dir, 'model.pkl'), outcome[0])
    return outcome


RF_SEARCH_GRID = (100, 500, 1000)        # classifier/train.py:626


def _rf_grid(n_estimators_grid):
    """the grid as a list of distinct positive ints, in the caller's order"""
    grid = list(n_estimators_grid)
    if not grid or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1 for n in grid) or len(set(grid)) != len(grid):
        raise ValueError('n_estimators_grid must hold distinct positive ints, one at least, not %r' % (n_estimators_grid,))
    return [int(n) for n in grid]


def train_rf_search(train_data, valid_data, test_data, model_dir, n_estimators_grid=RF_SEARCH_GRID, train_with_valid=False,
                    num_classes=10, random_state=12345678, valid_ratio=0.15, split_random_state=None, n_estimators=None, **kwargs):
    """train_param_search(..., train_func=train_rf, search_space={'n_estimators': n_estimators_grid}) with the grid fitted in one
    pass: one forest of max(grid) trees on the search's training part, whose first n trees are the forest train_rf fits with
    n_estimators=n (RandomForestClassifier.prefix), and one RandomForestClassifier.evaluate per split at all sizes at once: the
    training rows where the fit left them on the GPU, the validation rows, the test rows with their files.  The size with the best
    validation accuracy is kept (the earlier grid entry on ties), and with train_with_valid it is refitted as train_param_search
    refits it.  -> the same tuple (model, train_metrics, valid_metrics, test_metrics) with the same search records and the same
    numbers; 'loss' is 0.  model_dir/model.pkl holds the returned model (the loop over train_rf leaves the one it fitted last
    there).  n_estimators is ignored (the search sets it); of kwargs RF_ARGS are passed on, as in train_rf.  Without a validation
    fold (valid_data None): train_param_search's cut of valid_ratio of the training rows, seeded by split_random_state (None
    refuses, NO_SSS)."""
    grid = _rf_grid(n_estimators_grid)
    sizes = sorted(grid)
    forest_args = {k: kwargs[k] for k in RF_ARGS if k in kwargs}

    def fit(data, n):
        args = dict(forest_args)
        if isinstance(data['features'], DeviceFeatures):
            args.setdefault('device', data['features'].device)
        return RandomForestClassifier(n_estimators=n, random_state=random_state, **args).fit(data['features'], data['labels'])

    def score(clf, prefixes, train, valid):
        """-> [(train metrics, valid metrics, test metrics)] per prefix of the forest just fitted on `train`"""
        on_train = clf.evaluate(FITTED_ROWS, prefixes=prefixes)['predict']
        on_valid = clf.evaluate(valid['features'], prefixes=prefixes)['predict'] if valid else None
        per_file = None
        if test_data:          # train_rf scores the files by class index
            per_file = np.searchsorted(clf.classes_, clf.evaluate(test_data['features'], file_idxs=test_data['file_idxs'],
                                                                  prefixes=prefixes, outputs=('file_predict',))['file_predict'])
        scored = []
        for g in range(len(on_train)):
            train_metrics = compute_metrics(train['labels'], on_train[g], num_classes=num_classes)
            train_metrics['loss'] = 0
            valid_metrics = {}
            if valid:
                valid_metrics = compute_metrics(valid['labels'], on_valid[g], num_classes=num_classes)
                valid_metrics['loss'] = 0
            test_metrics = compute_metrics(test_data['labels'], per_file[g], num_classes=num_classes) if test_data else {}
            scored.append((train_metrics, valid_metrics, test_metrics))
        return scored

    def run_grid(search_train, search_valid):
        LOGGER.info('Fitting the grid n_estimators = %s as one forest of %d trees', grid, sizes[-1])
        whole = fit(search_train, sizes[-1])
        scored = score(whole, sizes, search_train, search_valid)
        return [((n,), whole.prefix(n)) + scored[sizes.index(n)] for n in grid]

    def refit(point, data):
        model = fit(data, point[0])
        train_metrics, _, test_metrics = score(model, None, data, None)[0]
        return model, train_metrics, test_metrics

    outcome = _search(train_data, valid_data, ['n_estimators'], valid_ratio, split_random_state, train_with_valid, run_grid, refit)
    LOGGER.info('Saving model...')
    _dump(os.path.join(model_dir, 'model.pkl'), outcome[0])
    return outcome


def train_rf_oob_search(train_data, valid_data, test_data, model_dir, n_estimators_grid=RF_SEARCH_GRID, train_with_valid=False,
                        num_classes=10, random_state=12345678, n_estimators=None, **kwargs):
    """The search over n_estimators (classifier/train.py:623-630) decided by out-of-bag accuracy instead of validation rows
    (DESIGN.md 8l): one forest of max(grid) trees fitted on the search rows -- train_data, or with train_with_valid and a
    valid_data train + valid shuffled together as train_param_search's refit merges them -- and one
    RandomForestClassifier.oob_evaluate of those rows at all sizes at once.  No row is cut off and nothing is fitted twice: the
    size with the best out-of-bag accuracy is kept (the earlier grid entry on ties) and the returned model is that prefix of the one
    forest, bit for bit the forest a separate fit of that size gives.  -> train_rf_search's tuple (model, train_metrics,
    valid_metrics, test_metrics): the metrics of the chosen size on the search rows, the validation rows (when given; with
    train_with_valid they were trained on) and the test files, scored as train_rf_search scores them, 'loss' 0, with its search
    records ('search' holds every size's metrics of that split); train_metrics also carries 'oob', compute_metrics of the chosen
    size's out-of-bag predictions, and 'oob_search', {(n,): those metrics} in grid order.  model_dir/model.pkl holds the returned
    model.  n_estimators is ignored (the search sets it); of kwargs RF_ARGS are passed on, as in train_rf."""
    grid = _rf_grid(n_estimators_grid)
    sizes = sorted(grid)
    forest_args = {k: kwargs[k] for k in RF_ARGS if k in kwargs}
    with contextlib.ExitStack() as made:
        rows = made.enter_context(_merged_and_shuffled(train_data, valid_data)) if train_with_valid and valid_data else train_data
        if isinstance(rows['features'], DeviceFeatures):
            forest_args.setdefault('device', rows['features'].device)
        LOGGER.info('Fitting the grid n_estimators = %s as one forest of %d trees', grid, sizes[-1])
        whole = RandomForestClassifier(n_estimators=sizes[-1], random_state=random_state, **forest_args)
        whole.fit(rows['features'], rows['labels'])
        out_of_bag = whole.oob_evaluate(prefixes=sizes, outputs=('predict',))['predict']
        on_train = whole.evaluate(FITTED_ROWS, prefixes=sizes)['predict']
        labels = np.asarray(rows['labels'])
    on_valid = whole.evaluate(valid_data['features'], prefixes=sizes)['predict'] if valid_data else None
    per_file = None
    if test_data:          # train_rf scores the files by class index
        per_file = np.searchsorted(whole.classes_, whole.evaluate(test_data['features'], file_idxs=test_data['file_idxs'], prefixes=sizes,
                                                                  outputs=('file_predict',))['file_predict'])

    def metrics(y, pred, loss=True):
        m = compute_metrics(y, pred, num_classes=num_classes)
        if loss:
            m['loss'] = 0
        return m

    at = [sizes.index(n) for n in grid]
    oob = [metrics(labels, out_of_bag[g], loss=False) for g in at]
    best = int(np.argmax([m['accuracy'] for m in oob]))          # the first of the largest: the earlier grid entry
    point = (grid[best],)
    LOGGER.info('Chosen %s (out-of-bag accuracy %s)', {'n_estimators': point[0]}, oob[best]['accuracy'])
    points = [(n,) for n in grid]
    record = {'search_params': ['n_estimators'], 'search_params_best_values': point}
    train_runs = [metrics(labels, on_train[g]) for g in at]
    train_metrics = dict(train_runs[best], search=dict(zip(points, train_runs)), oob=oob[best], oob_search=dict(zip(points, oob)), **record)
    valid_runs = [metrics(valid_data['labels'], on_valid[g]) if valid_data else {} for g in at]
    valid_metrics = dict(valid_runs[best], search=dict(zip(points, valid_runs)), **record)
    test_metrics = compute_metrics(test_data['labels'], per_file[at[best]], num_classes=num_classes) if test_data else {}
    model = whole.prefix(point[0])
    LOGGER.info('Saving model...')
    _dump(os.path.join(model_dir, 'model.pkl'), model)
    return model, train_metrics, valid_metrics, test_metrics


KNN_SEARCH_KS = (1, 3, 5, 10, 20, 50)
# the arguments of knn.KNeighborsClassifier that train_knn passes on from its keyword arguments
KNN_ARGS = ('device',)


def _knn_fit(data, n_neighbors, metric, num_classes, kwargs):
    args = {k: kwargs[k] for k in KNN_ARGS if k in kwargs}
    if isinstance(data['features'], DeviceFeatures):
        args.setdefault('device', data['features'].device)
    return KNeighborsClassifier(n_neighbors=n_neighbors, metric=metric, num_classes=num_classes, **args).fit(data['features'], data['labels'])


def _knn_scores(clf, ks, train, valid, test_data, num_classes):
    """-> [(train metrics, valid metrics, test metrics)] per size of ks (None: the classifier's own) of a classifier just fitted on
    `train`: one query per split at the largest size.  The training rows leave themselves out; the test set is scored per file."""
    on_train = np.atleast_2d(clf.evaluate(None, ks=ks)['predict'])
    on_valid = np.atleast_2d(clf.evaluate(valid['features'], ks=ks)['predict']) if valid else None
    per_file = None
    if test_data:
        per_file = np.atleast_2d(clf.evaluate(test_data['features'], file_idxs=test_data['file_idxs'], ks=ks,
                                              outputs=('file_predict',))['file_predict'])
    scored = []
    for g in range(len(on_train)):
        train_metrics = compute_metrics(train['labels'], on_train[g], num_classes=num_classes)
        train_metrics['loss'] = 0
        valid_metrics = {}
        if valid:
            valid_metrics = compute_metrics(valid['labels'], on_valid[g], num_classes=num_classes)
            valid_metrics['loss'] = 0
        test_metrics = compute_metrics(test_data['labels'], per_file[g], num_classes=num_classes) if test_data else {}
        scored.append((train_metrics, valid_metrics, test_metrics))
    return scored


def train_knn(train_data, valid_data, test_data, model_dir, n_neighbors=5, metric='sqeuclidean', num_classes=10, **kwargs):
    """-> (model, train_metrics, valid_metrics, test_metrics) with train_rf's conventions: knn.KNeighborsClassifier(n_neighbors,
    metric) holding the training rows, pickled to model_dir/model.pkl; 'loss' is 0; the test set is classified per file by the sum of
    its frames' votes.  Nothing is fitted, so a training row's nearest neighbour would be itself: the training metrics are
    leave-one-row-out.  The splits' features may be NumPy rows or usc.DeviceFeatures (queried where they are).  Of kwargs KNN_ARGS
    are passed on; the rest is ignored."""
    clf = _knn_fit(train_data, n_neighbors, metric, num_classes, kwargs)
    LOGGER.info('Saving model...')
    _dump(os.path.join(model_dir, 'model.pkl'), clf)
    train_metrics, valid_metrics, test_metrics = _knn_scores(clf, None, train_data, valid_data, test_data, num_classes)[0]
    LOGGER.info('Train (leave-one-out) - acc: %s', train_metrics['accuracy'])
    if valid_data:
        LOGGER.info('Valid - acc: %s', valid_metrics['accuracy'])
    return clf, train_metrics, valid_metrics, test_metrics


def _knn_sizes(ks):
    """the searched sizes as a list of distinct ints in [1, 64], at most 8, in the caller's order"""
    sizes = list(ks)
    if not 1 <= len(sizes) <= _lib.KNN_MAX_SIZES or len(set(sizes)) != len(sizes) or \
            any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _lib.KNN_TOPK_MAX for k in sizes):
        raise ValueError('ks must hold 1 to %d distinct ints in [1, %d], not %r' % (_lib.KNN_MAX_SIZES, _lib.KNN_TOPK_MAX, ks))
    return [int(k) for k in sizes]


def train_knn_search(train_data, valid_data, test_data, model_dir, ks=KNN_SEARCH_KS, train_with_valid=False, metric='sqeuclidean',
                     num_classes=10, valid_ratio=0.15, split_random_state=None, n_neighbors=None, **kwargs):
    """train_param_search(..., train_func=train_knn, search_space={'n_neighbors': ks}) from one query per split: the first k'
    entries of a sorted k-list are the k'-list, so the lists at max(ks) score every size (KNeighborsClassifier.evaluate(ks=...)).
    The size with the best validation accuracy is kept, the first one of ks on ties (_search's rule), and with train_with_valid
    it is refitted as train_param_search refits it.  -> (model, train_metrics, valid_metrics, test_metrics) with the search records
    train_rf_search writes; 'loss' is 0; model_dir/model.pkl holds the returned model.  n_neighbors is ignored (the search sets
    it).  Without a validation fold (valid_data None): train_param_search's cut of valid_ratio of the training rows, seeded by
    split_random_state (None refuses, NO_SSS)."""
    grid = _knn_sizes(ks)
    sizes = sorted(grid)

    def run_grid(search_train, search_valid):
        LOGGER.info('Scoring n_neighbors = %s from one query at %d', grid, sizes[-1])
        whole = _knn_fit(search_train, sizes[-1], metric, num_classes, kwargs)
        scored = _knn_scores(whole, sizes, search_train, search_valid, test_data, num_classes)
        return [((k,), whole.with_neighbors(k)) + scored[sizes.index(k)] for k in grid]

    def refit(point, data):
        model = _knn_fit(data, point[0], metric, num_classes, kwargs)
        train_metrics, _, test_metrics = _knn_scores(model, None, data, None, test_data, num_classes)[0]
        return model, train_metrics, test_metrics

    outcome = _search(train_data, valid_data, ['n_neighbors'], valid_ratio, split_random_state, train_with_valid, run_grid, refit)
    LOGGER.info('Saving model...')
    _dump(os.path.join(model_dir, 'model.pkl'), outcome[0])
    return outcome


MLP_SEARCH_SPACE = {'learning_rate': [1e-5, 1e-4, 1e-3], 'weight_decay': [1e-5, 1e-4, 1e-3]}        # classifier/train.py:638-651


class _GroupMember(object):
    """What train_mlp's callbacks see of a model, for one member of an _lib.MLPGroup: stop_training, and save_weights, which
    snapshots the member's weights on the device (ModelCheckpoint's file is written once, at the end, for the returned model)."""

    def __init__(self, group, index, patience, verbose):
        self.group, self.index = group, index
        self.stop_training = False
        self.logs = []          # one dict per epoch the member ran
        self.series = MetricCallback(verbose=verbose)
        # train_mlp's callbacks that decide something, in its order; the two that only write files are replayed afterwards
        self.hooks = [callbacks.ModelCheckpoint('', monitor='val_loss', save_best_only=True, save_weights_only=True),
                      EarlyStopping(monitor='val_loss', patience=patience), self.series]
        for cb in self.hooks:
            cb.set_model(self)
            cb.on_train_begin()

    def save_weights(self, filepath, overwrite=True):
        self.group.keep_best([self.index])

    def epoch_end(self, epoch, logs):
        self.logs.append(logs)
        for cb in self.hooks:
            cb.on_epoch_end(epoch, dict(logs))


def fit_mlp_grid(train_data, valid_data, test_data, model_dir, points, batch_size=64, num_epochs=100, valid_split=0.15, patience=20,
                 num_classes=10, random_state=12345678, verbose=False):
    """train_mlp at every (learning_rate, weight_decay) of `points`, fitted together as one _lib.MLPGroup (at most
    _lib.MLP_MAX_MEMBERS points at a time) -> [(model, train_metrics, valid_metrics, test_metrics)], one per point, each what
    train_mlp returns for that point, bit for bit.

    train_mlp seeds the Glorot draw and the epoch shuffle from random_state at every point, so the members start from the same
    weights and take the same rows at every step; they differ in the rate, the weight decay and the epoch at which early stopping
    ends them.  The rows are resident once (NumPy rows are uploaded once, a usc.DeviceFeatures is copied on its device); an epoch's
    step is seven launches for all live members.  Per member and in train_mlp's order: ModelCheckpoint's rule (a device snapshot
    when val_loss improves: strict <, so the first minimum), EarlyStopping, the metric series; a member that stops leaves the live
    set from the next epoch.  The validation rows are valid_data, or without it the last valid_split of the training rows, as
    MLPModel.fit slices them.  Every member is scored on the resident rows and, in one pass, on the test rows.
    In model_dir: history_csvlog.csv gets the rows train_mlp's CSVLogger appends, point by point in the order of `points`, and
    history_checkpoint.pkl is the last point's; model.h5 is left to the caller.  Each model is an MLPModel holding the point's
    best weights (no optimizer state)."""
    points = [(float(lr), float(wd)) for lr, wd in points]
    features, labels = train_data['features'], np.asarray(train_data['labels']).reshape(-1).astype(np.int32)
    on_device = isinstance(features, DeviceFeatures)
    if not on_device:
        features = np.asarray(features, np.float32)
    n_train, held_out = len(features), None
    if valid_data:
        held_out = valid_data['features']
        if not isinstance(held_out, DeviceFeatures):
            held_out = np.asarray(held_out, np.float32)
            if on_device:
                raise ValueError('the validation rows must be where the training rows are: a usc.DeviceFeatures')
        elif not on_device:
            raise ValueError('the validation rows must be where the training rows are: NumPy rows')
        valid_labels = np.asarray(valid_data['labels']).reshape(-1).astype(np.int32)
    elif valid_split and 0.0 < valid_split < 1.0:
        n_train = int(len(features) * (1.0 - valid_split))
        valid_labels = labels[n_train:]
    else:
        raise ValueError('the grid needs validation rows (early stopping and the checkpoint follow val_loss): valid_data, or a '
                         'valid_split in (0, 1)')
    targets = one_hot(labels, num_classes)
    steps = -(-n_train // int(batch_size))
    results = []
    for first in range(0, len(points), _lib.MLP_MAX_MEMBERS):
        chunk = points[first:first + _lib.MLP_MAX_MEMBERS]
        lrs = [lr for lr, _ in chunk]
        group = _lib.MLPGroup(features.shape[1], num_classes, int(batch_size), [wd for _, wd in chunk], [random_state] * len(chunk),
                              device=features.device if on_device else 0)
        try:
            if on_device:
                vx, vlo, vhi = (held_out, 0, len(held_out)) if held_out is not None else (features, n_train, len(features))
                group.set_data_dev(features.handle, 0, n_train, labels[:n_train], vx.handle, vlo, vhi, valid_labels)
            else:
                group.set_data(features[:n_train], labels[:n_train], held_out if held_out is not None else features[n_train:],
                               valid_labels)
            members = [_GroupMember(group, i, patience, verbose) for i in range(len(chunk))]
            rs = np.random.RandomState(random_state)
            for epoch in range(int(num_epochs)):
                live = [not m.stop_training for m in members]
                if not any(live):
                    break
                stats = group.epoch(rs.permutation(n_train), lrs, epoch * steps, live)
                for m, alive, logs in zip(members, live, stats):
                    if alive:
                        m.epoch_end(epoch, logs)
            # back to every member's lowest-val_loss snapshot, then all of them through each split in one pass
            group.restore_best(range(len(chunk)))
            if held_out is not None:
                on_train, on_valid = group.predict_resident(), group.predict_resident(valid=True)
            else:          # train_mlp predicts the whole of `features`, the validation tail included, in predict's row blocks
                on_train, on_valid = group.predict_dev(features.handle) if on_device else group.predict(features), None
            on_test = None
            if test_data:
                tx = test_data['features']
                on_test = group.predict_dev(tx.handle) if isinstance(tx, DeviceFeatures) else group.predict(tx)
            for i, ((lr, wd), m) in enumerate(zip(chunk, members)):
                for cb in (callbacks.LossHistory(os.path.join(model_dir, 'history_checkpoint.pkl')),
                           callbacks.CSVLogger(os.path.join(model_dir, 'history_csvlog.csv'), separator=',', append=True)):
                    cb.on_train_begin()
                    for epoch, logs in enumerate(m.logs):
                        cb.on_epoch_end(epoch, dict(logs))
                    cb.on_train_end()
                best = int(np.argmin(m.series.valid_loss))
                train_metrics = _series_metrics((m.series.train_loss, m.series.train_acc), best)
                scored = compute_metrics(targets, on_train[i], num_classes=num_classes)
                train_metrics['class_accuracy'] = scored['class_accuracy']
                train_metrics['average_class_accuracy'] = scored['average_class_accuracy']
                valid_metrics = _series_metrics((m.series.valid_loss, m.series.valid_acc), best)
                if on_valid is not None:
                    valid_metrics.update(compute_metrics(one_hot(valid_labels, num_classes), on_valid[i], num_classes=num_classes))
                test_metrics = {}
                if test_data:
                    per_file = _file_predictions(on_test[i], test_data['file_idxs'])
                    test_metrics = compute_metrics(test_data['labels'], per_file, num_classes=num_classes)
                model, _, _ = construct_mlp_model(features.shape[1:], weight_decay=wd, num_classes=num_classes, seed=random_state)
                model.compile(lr=lr)
                model.set_weights(group.get_weights(i))
                results.append((model, train_metrics, valid_metrics, test_metrics))
        finally:
            group.close()
    return results


def train_mlp_search(train_data, valid_data, test_data, model_dir, search_space=MLP_SEARCH_SPACE, train_with_valid=True,
                     valid_ratio=0.15, split_random_state=None, batch_size=64, num_epochs=100, valid_split=0.15, patience=20,
                     num_classes=10, random_state=12345678, verbose=False, **kwargs):
    """train_param_search(..., train_func=train_mlp, search_space=search_space) with the grid fitted as one group of models on the
    GPU (fit_mlp_grid: one resident copy of the rows, seven launches per step for all live points, every point scored on the
    resident rows): every metric, history and search record, the chosen point and the returned weights equal the loop's bit for
    bit.  search_space: values for 'learning_rate' and 'weight_decay', the grid being their product in key order.  The splits'
    features are NumPy rows or usc.DeviceFeatures (kept on their device).  With train_with_valid the chosen point is refitted by a
    plain train_mlp, as train_param_search refits it; without a validation fold (valid_data None) the search runs on
    train_param_search's cut (valid_ratio, split_random_state; None refuses, NO_SSS).  -> (model, train_metrics, valid_metrics,
    test_metrics); model is an MLPModel with the chosen point's best weights.  In model_dir history_csvlog.csv and
    history_checkpoint.pkl are what the loop leaves; model.h5 holds the returned model (the loop over train_mlp leaves the
    checkpoint of the run it made last).  learning_rate and weight_decay among kwargs are ignored (the search sets them), and so
    is the rest, as train_mlp ignores it."""
    names = list(search_space)
    if sorted(names) != ['learning_rate', 'weight_decay']:
        raise ValueError('the MLP\'s grid is over learning_rate and weight_decay, not %r' % (names,))
    grid = list(product(*(search_space[n] for n in names)))
    at = {n: names.index(n) for n in names}
    args = dict(batch_size=batch_size, num_epochs=num_epochs, valid_split=valid_split, patience=patience, num_classes=num_classes,
                random_state=random_state, verbose=verbose)

    def run_grid(search_train, search_valid):
        LOGGER.info('Fitting the grid %s as one group of %d models', dict(search_space), len(grid))
        fitted = fit_mlp_grid(search_train, search_valid, test_data, model_dir,
                              [(p[at['learning_rate']], p[at['weight_decay']]) for p in grid], **args)
        return [(point,) + run for point, run in zip(grid, fitted)]

    def refit(point, data):
        model, train_metrics, _, test_metrics = train_mlp(data, None, test_data, model_dir, learning_rate=point[at['learning_rate']],
                                                          weight_decay=point[at['weight_decay']], **args)
        return model, train_metrics, test_metrics

    outcome = _search(train_data, valid_data, names, valid_ratio, split_random_state, train_with_valid, run_grid, refit)
    LOGGER.info('Saving model...')
    outcome[0].save_weights(os.path.join(model_dir, 'model.h5'))
    return outcome


# ---- one cross-validation fold ------------------------------------------------------------------------------------------------------
def _dataset_of(features_dir):
    """'.../features/us8k/l3/...' -> ('us8k', 'us8k/l3/...'): the path after the last 'features/' and its first part, a dataset"""
    at = features_dir.rindex('features')
    desc = features_dir[at + len('features/'):]
    dataset = desc.split('/')[0]
    if dataset not in DATASET_NUM_CLASSES:
        raise ValueError('the features directory must name a dataset right after "features/" (one of {})'.format(
            ', '.join(sorted(DATASET_NUM_CLASSES))))
    return dataset, desc


def _model_id(desc, feature_mode, non_overlap, use_min_max, model_type):
    return os.path.join(desc, feature_mode, 'non-overlap' if non_overlap else 'overlap', 'min-max' if use_min_max else 'no-min-max',
                        model_type)


def _dump(path, obj):
    with open(path, 'wb') as fh:
        pk.dump(obj, fh, protocol=pk.HIGHEST_PROTOCOL)


def _searches_without_valid_fold(fold):
    """whether the fold's parameter search has no validation fold: every fold but the test fold then trains"""
    return bool(fold['parameter_search'] and not fold['parameter_search_valid_fold'])


def _searches_on_a_cut(fold):
    """whether the fold's parameter search has no validation fold and cuts the training rows instead; refuses without the seed.  A
    search that says it needs no validation rows (search_without_cut: the forest's out-of-bag search) makes no cut."""
    on_cut = _searches_without_valid_fold(fold) and not fold.get('search_without_cut')
    _require_split_seed(on_cut, fold['parameter_search_split_seed'])
    return on_cut


# config.json: the reference's keys in its order (no git metadata: git_commit is None), then the two that are named only when set
_CONFIG_KEYS = ('fold_num', 'parameter_search', 'parameter_search_valid_fold', 'parameter_search_valid_ratio',
                'parameter_search_train_with_valid', 'model_type', 'feature_mode', 'train_batch_size', 'patience', 'non_overlap',
                'non_overlap_chunk_size', 'random_state', 'verbose')
_CONFIG_KEYS_WHEN_SET = ('preprocess_device', 'parameter_search_split_seed')


def _run_fold(fold, get_splits=None):
    """One cross-validation fold of any model type (classifier/train.py:495-709) -> its directory.  fold: the settings, the
    arguments of train / train_svm_fold by name (model_type, fold_num and model_args among them; model_part, where given, is the
    function that runs the fold's model in place of the model type's own).  get_splits: a function of
    (with_valid_fold) that gives the fold's (train, valid or None, test) in place of usc.get_split (cross_validate's come from its
    FoldBank).  The splits are the driver's from the moment it has them: closed once, whatever fails after that."""
    on_cut = _searches_on_a_cut(fold)
    if fold['gsheet_id']:
        LOGGER.warning('Google Sheets logging is not built; gsheet_id ignored')
    features_dir, fold_num = fold['features_dir'], fold['fold_num']
    dataset, desc = _dataset_of(features_dir)
    model_id = _model_id(desc, fold['feature_mode'], fold['non_overlap'], fold['use_min_max'], fold['model_type'])
    model_dir = os.path.join(fold['output_dir'], 'classifier', model_id, 'fold%d' % fold_num,
                             datetime.datetime.now().strftime('%Y%m%d%H%M%S'))
    os.makedirs(model_dir, exist_ok=True)

    config = dict(username=getpass.getuser(), features_dir=features_dir, output_dir=fold['output_dir'], model_dir=model_dir,
                  model_id=model_id)
    config.update((k, fold[k]) for k in _CONFIG_KEYS)
    config.update(git_commit=None, gsheet_id=fold['gsheet_id'], google_dev_app_name=fold['google_dev_app_name'])
    config.update((k, fold[k]) for k in _CONFIG_KEYS_WHEN_SET if fold[k] is not None)
    config.update(fold['model_args'])
    with open(os.path.join(model_dir, 'config.json'), 'w') as fh:
        json.dump(config, fh)

    LOGGER.info('Fold %d of %s: loading and preprocessing', fold_num, dataset)
    get_splits = get_splits or functools.partial(get_split, features_dir, fold_num - 1, dataset)
    with _closing(get_splits(not _searches_without_valid_fold(fold))) as splits:
        scalers = preprocess_split_data(*splits, feature_mode=fold['feature_mode'], non_overlap=fold['non_overlap'],
                                        non_overlap_chunk_size=int(fold['non_overlap_chunk_size']), use_min_max=fold['use_min_max'],
                                        device=fold['preprocess_device'])
        for name, scaler in zip(('min_max_scaler.pkl', 'stdizer.pkl'), scalers):
            _dump(os.path.join(model_dir, name), scaler)
        model_part = fold.get('model_part') or {'mlp': _mlp_part, 'svm': _svm_part, 'rf': _rf_part}[fold['model_type']]
        _, train_metrics, valid_metrics, test_metrics = model_part(
            splits, model_dir, dict(fold, num_classes=DATASET_NUM_CLASSES[dataset], search_on_cut=on_cut))
    _dump(os.path.join(model_dir, 'results.pkl'), {'train': train_metrics, 'valid': valid_metrics, 'test': test_metrics})
    LOGGER.info('Fold %d done: results in %s', fold_num, model_dir)
    return model_dir


def _mlp_part(splits, model_dir, fold):
    """the MLP's part of a fold -> (model, train_metrics, valid_metrics, test_metrics): one train_mlp, or the search over learning
    rate and weight decay"""
    args = dict(dict(batch_size=fold['train_batch_size'], patience=fold['patience'], random_state=fold['random_state'],
                     num_classes=fold['num_classes'], verbose=fold['verbose']), **fold['model_args'])
    if not fold['parameter_search']:
        return train_mlp(*splits, model_dir, **args)
    if not fold['search_on_cut']:          # with a validation fold: one download; the search then runs as on the host
        splits = tuple(_on_host(d) for d in splits)
    # on a cut the splits stay where they are: train_mlp takes DeviceFeatures as it does without a search
    return train_param_search(*splits, model_dir, train_func=train_mlp, search_space=MLP_SEARCH_SPACE, valid_ratio=fold['parameter_search_valid_ratio'],
                              train_with_valid=fold['parameter_search_train_with_valid'],
                              split_random_state=fold['parameter_search_split_seed'], **args)


def _mlp_search_part(splits, model_dir, fold):
    """the part of a fold that searches the MLP's learning rate and weight decay as one group of models -> (model, train_metrics,
    valid_metrics, test_metrics): train_mlp_search on the validation fold or on a cut, the splits staying where they are"""
    args = dict(dict(batch_size=fold['train_batch_size'], patience=fold['patience'], random_state=fold['random_state'],
                     num_classes=fold['num_classes'], verbose=fold['verbose']), **fold['model_args'])
    return train_mlp_search(*splits, model_dir, valid_ratio=fold['parameter_search_valid_ratio'],
                            train_with_valid=fold['parameter_search_train_with_valid'],
                            split_random_state=fold['parameter_search_split_seed'], **args)


def _svm_part(splits, model_dir, fold):
    """the SVM's part of a fold -> (model, train_metrics, valid_metrics, test_metrics): one train_svm scored on the device, or the
    search over C"""
    args = dict(dict(random_state=fold['random_state'], num_classes=fold['num_classes'], verbose=fold['verbose']), **fold['model_args'])
    if not fold['parameter_search']:
        return train_svm(*splits, model_dir, evaluate_on_device=True, **args)
    if fold['search_on_cut']:
        args.update(valid_ratio=fold['parameter_search_valid_ratio'], split_random_state=fold['parameter_search_split_seed'])
    return train_svm_search(*splits, model_dir, train_with_valid=fold['parameter_search_train_with_valid'], platt=fold['platt'], **args)


def _rf_part(splits, model_dir, fold):
    """the random forest's part of a fold -> (model, train_metrics, valid_metrics, test_metrics): one train_rf; no search"""
    if fold['parameter_search']:
        raise ValueError(NO_RF_SEARCH)
    args = dict(dict(random_state=fold['random_state'], num_classes=fold['num_classes'], verbose=fold['verbose']), **fold['model_args'])
    return train_rf(*splits, model_dir, **args)


def _rf_search_part(splits, model_dir, fold):
    """the part of a fold that searches the random forest's n_estimators -> (model, train_metrics, valid_metrics, test_metrics):
    train_rf_search with the fold's grid (in model_args), on the validation fold or on a cut"""
    args = dict(dict(random_state=fold['random_state'], num_classes=fold['num_classes'], verbose=fold['verbose']), **fold['model_args'])
    if fold['search_on_cut']:
        args.update(valid_ratio=fold['parameter_search_valid_ratio'], split_random_state=fold['parameter_search_split_seed'])
    return train_rf_search(*splits, model_dir, train_with_valid=fold['parameter_search_train_with_valid'], **args)


def _rf_oob_part(splits, model_dir, fold):
    """the part of a fold that searches the random forest's n_estimators by out-of-bag accuracy -> (model, train_metrics,
    valid_metrics, test_metrics): train_rf_oob_search with the fold's grid (in model_args); without a validation fold every
    training row is fitted and none is cut off"""
    args = dict(dict(random_state=fold['random_state'], num_classes=fold['num_classes'], verbose=fold['verbose']), **fold['model_args'])
    return train_rf_oob_search(*splits, model_dir, train_with_valid=fold['parameter_search_train_with_valid'], **args)


def train(features_dir, output_dir, fold_num, model_type='svm', feature_mode='framewise', train_batch_size=64, patience=20,
          random_state=20171021, parameter_search=False, parameter_search_valid_fold=True, parameter_search_valid_ratio=0.15,
          parameter_search_train_with_valid=False, gsheet_id=None, google_dev_app_name=None, verbose=False, non_overlap=False,
          non_overlap_chunk_size=10, use_min_max=False, preprocess_device=None, parameter_search_split_seed=None, **model_args):
    """classifier/train.py:495-709 for model_type='mlp': one cross-validation fold (fold_num is 1-based) of the features under
    `features_dir` (its path names the dataset after 'features/'), written to
    <output_dir>/classifier/<features desc>/<mode>/<overlap>/<min-max>/mlp/fold<N>/<timestamp>/: config.json,
    min_max_scaler.pkl, stdizer.pkl, model.h5, history_checkpoint.pkl, history_csvlog.csv, results.pkl.
    preprocess_device: a GPU index preprocesses the folds on that GPU (usc.preprocess_split_data(device=...)) and, without a
    parameter search, hands them to the MLP there; config.json names it only when it is set.
    parameter_search_split_seed: an int lets parameter_search=True, parameter_search_valid_fold=False run: the search is made on a
    stratified cut of parameter_search_valid_ratio of the training rows, drawn from this seed (train_param_search's
    split_random_state), and with preprocess_device the rows stay on the GPU through the cut and every run of the grid; None
    refuses that mode (NO_SSS).  config.json names it only when it is set.
    -> that directory."""
    fold = dict(locals())          # the fold's settings by name, before any other local exists
    if model_type != 'mlp':
        raise ValueError(ONLY_MLP.format(model_type))
    return _run_fold(fold)


def train_svm_fold(features_dir, output_dir, fold_num, feature_mode='framewise', train_batch_size=64, patience=20,
                   random_state=20171021, parameter_search=False, parameter_search_valid_fold=True,
                   parameter_search_valid_ratio=0.15, parameter_search_train_with_valid=False, gsheet_id=None,
                   google_dev_app_name=None, verbose=False, non_overlap=False, non_overlap_chunk_size=10, use_min_max=False,
                   preprocess_device=None, platt='device', parameter_search_split_seed=None, **model_args):
    """classifier/train.py:495-709 for model_type='svm': one cross-validation fold as train() runs it for the MLP, written to
    <output_dir>/classifier/<features desc>/<mode>/<overlap>/<min-max>/svm/fold<N>/<timestamp>/: config.json, min_max_scaler.pkl,
    stdizer.pkl, model.pkl, results.pkl.  preprocess_device: a GPU index preprocesses the folds on that GPU and the SVM is
    fitted and scored from the splits there (nothing is downloaded but the results); config.json names it only when it is set.
    parameter_search: train_svm_search over C = 0.1 ... 1000 (platt: its sigmoid fit, 'device' or 'host'); else one train_svm with
    model_args (C, kernel, tol, max_iterations).  train_batch_size and patience are recorded as the reference records them; the
    SVM does not use them.  parameter_search_split_seed: as in train(); the cut and the search on it are train_svm_search's.
    -> that directory."""
    return _run_fold(dict(locals(), model_type='svm'))          # the fold's settings by name


def train_rf_fold(features_dir, output_dir, fold_num, feature_mode='framewise', train_batch_size=64, patience=20,
                  random_state=20171021, parameter_search=False, parameter_search_valid_fold=True,
                  parameter_search_valid_ratio=0.15, parameter_search_train_with_valid=False, gsheet_id=None,
                  google_dev_app_name=None, verbose=False, non_overlap=False, non_overlap_chunk_size=10, use_min_max=False,
                  preprocess_device=None, parameter_search_split_seed=None, **model_args):
    """classifier/train.py:495-709 for model_type='rf': one cross-validation fold as train() runs it for the MLP, written to
    <output_dir>/classifier/<features desc>/<mode>/<overlap>/<min-max>/rf/fold<N>/<timestamp>/: config.json, min_max_scaler.pkl,
    stdizer.pkl, model.pkl, results.pkl.  preprocess_device: a GPU index preprocesses the folds on that GPU and the forest is fitted
    and scored from the splits there; config.json names it only when it is set.  One train_rf with model_args (n_estimators and
    RF_ARGS); parameter_search=True raises (NO_RF_SEARCH) before anything is read.  train_batch_size and patience are recorded as
    the reference records them; the forest does not use them.  -> that directory."""
    if parameter_search:
        raise ValueError(NO_RF_SEARCH)
    return _run_fold(dict(locals(), model_type='rf'))          # the fold's settings by name


def train_rf_search_fold(features_dir, output_dir, fold_num, feature_mode='framewise', train_batch_size=64, patience=20,
                         random_state=20171021, n_estimators_grid=RF_SEARCH_GRID, parameter_search_valid_fold=True,
                         parameter_search_valid_ratio=0.15, parameter_search_train_with_valid=False, gsheet_id=None,
                         google_dev_app_name=None, verbose=False, non_overlap=False, non_overlap_chunk_size=10, use_min_max=False,
                         preprocess_device=None, parameter_search_split_seed=None, **model_args):
    """classifier/train.py:495-709 for model_type='rf' with parameter_search (:623-630): train_rf_fold's fold, directory
    (.../rf/fold<N>/<timestamp>/) and five files, the model chosen by train_rf_search over n_estimators_grid: on the validation
    fold, or with parameter_search_valid_fold=False on a stratified cut seeded by parameter_search_split_seed (None refuses,
    NO_SSS).  config.json records parameter_search true and n_estimators_grid; model_args are RF_ARGS.  -> that directory."""
    fold = dict(locals(), model_type='rf', parameter_search=True, model_part=_rf_search_part)          # the fold's settings by name
    fold['model_args'] = dict(model_args, n_estimators_grid=_rf_grid(fold.pop('n_estimators_grid')))
    return _run_fold(fold)


def _refuse_cut_settings(model_args):
    """the out-of-bag search's one refusal of its own: the settings of a cut that it does not make"""
    named = sorted({'parameter_search_valid_ratio', 'parameter_search_split_seed'} & set(model_args))
    if named:
        raise ValueError('the out-of-bag search cuts no validation rows off: %s do not apply' % ', '.join(named))


def train_rf_oob_fold(features_dir, output_dir, fold_num, feature_mode='framewise', train_batch_size=64, patience=20,
                      random_state=20171021, n_estimators_grid=RF_SEARCH_GRID, parameter_search_valid_fold=True,
                      parameter_search_train_with_valid=False, gsheet_id=None, google_dev_app_name=None, verbose=False,
                      non_overlap=False, non_overlap_chunk_size=10, use_min_max=False, preprocess_device=None, **model_args):
    """classifier/train.py:495-709 for model_type='rf' with parameter_search (:623-630), the size chosen by out-of-bag accuracy
    (DESIGN.md 8l): train_rf_search_fold's fold, directory (.../rf/fold<N>/<timestamp>/) and five files, the model chosen by
    train_rf_oob_search over n_estimators_grid.  With parameter_search_valid_fold=False no seed is needed: no rows are cut off, every
    fold but the test fold trains, and the search decides on the rows it trains on.  With a validation fold that fold is scored
    (and with parameter_search_train_with_valid trained on) but does not decide.  config.json records parameter_search true,
    n_estimators_grid and selection 'oob'; it has no ratio and no seed of a cut to record (parameter_search_valid_ratio is null).
    model_args are RF_ARGS.  -> that directory."""
    _refuse_cut_settings(model_args)
    fold = dict(locals(), model_type='rf', parameter_search=True, model_part=_rf_oob_part, search_without_cut=True,
                parameter_search_valid_ratio=None, parameter_search_split_seed=None)          # the fold's settings by name
    fold['model_args'] = dict(model_args, n_estimators_grid=_rf_grid(fold.pop('n_estimators_grid')), selection='oob')
    return _run_fold(fold)


def train_mlp_search_fold(features_dir, output_dir, fold_num, feature_mode='framewise', train_batch_size=64, patience=20,
                          random_state=20171021, parameter_search_valid_fold=True, parameter_search_valid_ratio=0.15,
                          parameter_search_train_with_valid=False, gsheet_id=None, google_dev_app_name=None, verbose=False,
                          non_overlap=False, non_overlap_chunk_size=10, use_min_max=False, preprocess_device=None,
                          parameter_search_split_seed=None, **model_args):
    """classifier/train.py:495-709 for model_type='mlp' with parameter_search (:638-651): train(parameter_search=True)'s fold,
    directory (.../mlp/fold<N>/<timestamp>/), seven files and config.json keys, the model chosen by train_mlp_search: the grid over
    learning rate and weight decay (MLP_SEARCH_SPACE) fitted as one group of models on the GPU, on the validation fold, or with
    parameter_search_valid_fold=False on a stratified cut seeded by parameter_search_split_seed (None refuses, NO_SSS).  With
    preprocess_device the splits stay on that GPU through the search.  model_args: train_mlp's (num_epochs, ...; learning_rate and
    weight_decay are recorded and then set by the search).  model.h5 holds the returned model.  -> that directory."""
    return _run_fold(dict(locals(), model_type='mlp', parameter_search=True, model_part=_mlp_search_part))      # the settings by name


def _knn_part(splits, model_dir, fold):
    """the nearest-neighbour classifier's part of a fold -> (model, train_metrics, valid_metrics, test_metrics): one train_knn"""
    return train_knn(*splits, model_dir, **dict(dict(num_classes=fold['num_classes']), **fold['model_args']))


def _knn_search_part(splits, model_dir, fold):
    """the part of a fold that searches n_neighbors -> (model, train_metrics, valid_metrics, test_metrics): train_knn_search with
    the fold's sizes (in model_args), on the validation fold or on a cut"""
    args = dict(dict(num_classes=fold['num_classes']), **fold['model_args'])
    if fold['search_on_cut']:
        args.update(valid_ratio=fold['parameter_search_valid_ratio'], split_random_state=fold['parameter_search_split_seed'])
    return train_knn_search(*splits, model_dir, train_with_valid=fold['parameter_search_train_with_valid'], **args)


def train_knn_fold(features_dir, output_dir, fold_num, feature_mode='framewise', train_batch_size=64, patience=20,
                   random_state=20171021, parameter_search_valid_fold=True, parameter_search_valid_ratio=0.15,
                   parameter_search_train_with_valid=False, gsheet_id=None, google_dev_app_name=None, verbose=False,
                   non_overlap=False, non_overlap_chunk_size=10, use_min_max=False, preprocess_device=None,
                   parameter_search_split_seed=None, **model_args):
    """One cross-validation fold as train_rf_fold runs it, for the nearest-neighbour classifier: written to
    <output_dir>/classifier/<features desc>/<mode>/<overlap>/<min-max>/knn/fold<N>/<timestamp>/: config.json, min_max_scaler.pkl,
    stdizer.pkl, model.pkl, results.pkl.  One train_knn with model_args (n_neighbors, metric and KNN_ARGS); no search
    (train_knn_search_fold).  train_batch_size, patience and random_state are recorded as the reference records them; nothing here
    uses them.  -> that directory."""
    return _run_fold(dict(locals(), model_type='knn', parameter_search=False, model_part=_knn_part))      # the settings by name


def train_knn_search_fold(features_dir, output_dir, fold_num, feature_mode='framewise', train_batch_size=64, patience=20,
                          random_state=20171021, ks=KNN_SEARCH_KS, parameter_search_valid_fold=True,
                          parameter_search_valid_ratio=0.15, parameter_search_train_with_valid=False, gsheet_id=None,
                          google_dev_app_name=None, verbose=False, non_overlap=False, non_overlap_chunk_size=10, use_min_max=False,
                          preprocess_device=None, parameter_search_split_seed=None, **model_args):
    """train_knn_fold's fold, directory (.../knn/fold<N>/<timestamp>/) and five files, the model chosen by train_knn_search over
    ks: on the validation fold, or with parameter_search_valid_fold=False on a stratified cut seeded by
    parameter_search_split_seed (None refuses, NO_SSS).  config.json records parameter_search true and ks; model_args are metric
    and KNN_ARGS.  -> that directory."""
    fold = dict(locals(), model_type='knn', parameter_search=True, model_part=_knn_search_part)          # the fold's settings by name
    fold['model_args'] = dict(model_args, ks=_knn_sizes(fold.pop('ks')))
    return _run_fold(fold)


# what a fold's metrics hold besides numbers and lists of numbers with one entry per class: the per-epoch histories (their length
# differs from fold to fold under early stopping) and the parameter search's records
NOT_AGGREGATED = ('loss_history', 'accuracy_history', 'search', 'search_params', 'search_params_best_values')


def _aggregated_part(fold_metrics):
    """aggregate_metrics over the keys of the first fold that hold a number or a list of numbers and are not in NOT_AGGREGATED"""
    def numeric(v):
        a = np.asarray(v)
        return a.ndim <= 1 and a.size > 0 and a.dtype.kind in 'biuf'
    keys = [k for k, v in fold_metrics[0].items() if k not in NOT_AGGREGATED and numeric(v)]
    return aggregate_metrics([{k: fold[k] for k in keys} for fold in fold_metrics]) if keys else {}


def _jsonable(v):
    """NumPy scalars and arrays as Python numbers and lists, tuples as lists, every dictionary key as a string"""
    if isinstance(v, dict):
        return {k if isinstance(k, str) else str(k): _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, np.ndarray):
        return _jsonable(v.tolist())
    if isinstance(v, np.generic):
        return v.item()
    return v


def cross_validate(features_dir, output_dir, model_type='svm', folds=None, fold_seed=None, preprocess_device=0,
                   feature_mode='framewise', train_batch_size=64, patience=20, random_state=20171021, parameter_search=False,
                   parameter_search_valid_fold=True, parameter_search_valid_ratio=0.15, parameter_search_train_with_valid=False,
                   gsheet_id=None, google_dev_app_name=None, verbose=False, non_overlap=False, non_overlap_chunk_size=10,
                   use_min_max=False, platt='device', parameter_search_split_seed=None, **model_args):
    """Every fold of a dataset in one run: what one train(model_type='mlp') or train_svm_fold (model_type='svm'; 'rf' raises as in
    train) call per fold does -- the same per-fold directories and files, from the same arguments -- with the feature files read
    and uploaded once (usc.FoldBank on preprocess_device; None keeps the folds and their preprocessing on the host) and every
    fold's splits put together from them on the GPU, bit for bit the matrices usc.get_split stacks.

    folds: the test folds to run, 1-based; None runs all of the dataset's.  fold_seed: an int seeds NumPy's global state
    (np.random.seed) before each fold, so that fold k equals a separate per-fold call made after np.random.seed(fold_seed); None
    leaves the global state alone, and the folds draw their shuffles one after the other from it.  platt: train_svm_fold's.
    parameter_search_split_seed: train()'s and train_svm_fold's, the same seed for every fold.
    A fold's splits are closed before the next fold's are assembled.

    Afterwards <output_dir>/classifier/<model_id>/cross_validation/<timestamp>/results.pkl and results.json hold
    {'folds': the fold numbers, 'fold_dirs': their directories, 'train' / 'valid' / 'test': the list of the folds' metrics as
    their results.pkl holds them, 'aggregate': {'train', 'valid', 'test'}: aggregate_metrics over the folds of every key whose
    value is a number or a list of numbers}.  Not aggregated (NOT_AGGREGATED): loss_history and accuracy_history, whose lengths
    differ between folds, and the search records search, search_params and search_params_best_values.  In results.json NumPy
    values are plain numbers and the search's tuple keys are strings.  -> that directory."""
    settings = dict(locals())          # every fold's settings by name, before any other local exists
    if model_type not in ('mlp', 'svm'):
        raise ValueError(ONLY_MLP.format(model_type))
    dataset, desc = _dataset_of(features_dir)
    _searches_on_a_cut(settings)          # refused before anything is read
    fold_dirs = []
    with FoldBank(features_dir, dataset, device=preprocess_device) as bank:
        folds = list(range(1, bank.num_folds + 1)) if folds is None else [int(f) for f in folds]
        for fold_num in folds:
            if not 1 <= fold_num <= bank.num_folds:
                raise ValueError('fold {} of {} ({} folds, counted from 1)'.format(fold_num, dataset, bank.num_folds))
        for fold_num in folds:
            if fold_seed is not None:
                np.random.seed(fold_seed)
            fold_dirs.append(_run_fold(dict(settings, fold_num=fold_num), get_splits=functools.partial(bank.split, fold_num - 1)))

    results = {'folds': folds, 'fold_dirs': fold_dirs}
    per_fold = []
    for d in fold_dirs:
        with open(os.path.join(d, 'results.pkl'), 'rb') as fh:
            per_fold.append(pk.load(fh))
    for part in ('train', 'valid', 'test'):
        results[part] = [r[part] for r in per_fold]
    results['aggregate'] = {part: _aggregated_part(results[part]) for part in ('train', 'valid', 'test')}

    out_dir = os.path.join(output_dir, 'classifier', _model_id(desc, feature_mode, non_overlap, use_min_max, model_type), 'cross_validation',
                           datetime.datetime.now().strftime('%Y%m%d%H%M%S'))
    os.makedirs(out_dir, exist_ok=True)
    _dump(os.path.join(out_dir, 'results.pkl'), results)
    with open(os.path.join(out_dir, 'results.json'), 'w') as fh:
        json.dump(_jsonable(results), fh)
    LOGGER.info('Cross-validation of %d folds done: results in %s', len(folds), out_dir)
    return out_dir
