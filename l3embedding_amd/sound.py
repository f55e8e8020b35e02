"""Classify audio with a trained L3 embedding and a trained downstream classifier, end to end on one GPU: the inference step of
the reference's notebooks/pimodel.ipynb (audio -> 1 s frames -> embedding -> standardiser -> classifier -> mean of the frame
probabilities per file -> arg-max) on top of data/usc/features.py:256-306 (get_l3_frames_uniform) and the transforms of :97-150.

The pooled embedding rows never leave the device: EmbeddingModel.predict_clips(..., to_device=True) writes them into a
usc.DeviceFeatures, the stages of usc._preprocess_on_device run on it with the run's fitted scalers, and each classifier scores it
where it is -- the MLP through MLPModel.predict_files (csrc/mlp.hip, per-file mean and arg-max on the device), the SVM and the
forest through their evaluate().  What comes back is (F, C) probabilities and F classes.

SoundClassifier.from_run reads what a fold's run directory holds (classifier._run_fold): config.json, min_max_scaler.pkl,
stdizer.pkl and model.h5 or model.pkl.
"""
import json
import os
import pickle as pk

import numpy as np

from . import usc
from .features import read_wav

MODEL_TYPES = ('mlp', 'svm', 'rf')


def _fitted(scaler, attr):
    return scaler is not None and hasattr(scaler, attr)


def _model_kind(classifier):
    from .classifier import MLPModel
    from .forest import RandomForestClassifier
    from .svm import SVC
    for kind, cls in (('mlp', MLPModel), ('svm', SVC), ('rf', RandomForestClassifier)):
        if isinstance(classifier, cls):
            return kind
    raise TypeError('classifier must be a classifier.MLPModel, svm.SVC or forest.RandomForestClassifier, not %s'
                    % type(classifier).__name__)


def _input_width(kind, classifier):
    if kind == 'mlp':
        return int(classifier.input_dim)
    if kind == 'svm':
        classifier._check_fitted()
        return int(classifier.shape_fit_[1])
    classifier._check_fitted()
    return int(classifier.n_features_)


class SoundClassifier(object):
    """embedding: the audio EmbeddingModel of load_embedding; classifier: a trained MLPModel, SVC(probability=True) or
    RandomForestClassifier on the embedding's GPU; stdizer: the run's fitted usc.StandardScaler; min_max_scaler: its
    usc.MinMaxScaler, applied only when it is fitted; feature_mode, non_overlap, non_overlap_chunk_size: the run's
    preprocessing; hop_size: seconds between frames.

    predict_clips / predict_files -> {'file_proba': (F, C), 'file_predict': (F,)}: per file the mean of its frames' class
    probabilities (float32 for the MLP, float64 for the SVM and the forest) and its arg-max -- a class index for the MLP, a
    classes_ value for the other two, as their own predict gives."""

    def __init__(self, embedding, classifier, stdizer, min_max_scaler=None, feature_mode='framewise', non_overlap=False,
                 non_overlap_chunk_size=10, hop_size=0.1):
        from .model import EmbeddingModel
        if not isinstance(embedding, EmbeddingModel) or embedding.embedding_type != 'audio':
            raise TypeError('embedding must be the audio embedding model load_embedding(..., "audio", ...) returns')
        if feature_mode not in ('framewise', 'stats'):
            raise ValueError("feature_mode must be 'framewise' or 'stats', not {!r}".format(feature_mode))
        if not _fitted(stdizer, 'scale_'):
            raise ValueError('stdizer must be a fitted usc.StandardScaler')
        self.kind = _model_kind(classifier)
        if self.kind == 'svm' and not classifier.probability:
            raise ValueError('the SVC was fitted with probability=False: it has no class probabilities to average')
        self.embedding, self.classifier, self.stdizer = embedding, classifier, stdizer
        self.min_max_scaler = min_max_scaler if _fitted(min_max_scaler, 'scale_') else None
        self.feature_mode, self.non_overlap = feature_mode, bool(non_overlap)
        self.non_overlap_chunk_size, self.hop_size = int(non_overlap_chunk_size), float(hop_size)
        if self.non_overlap and self.non_overlap_chunk_size < 1:
            raise ValueError('non_overlap_chunk_size must be >= 1')
        self.hop_length = int(self.hop_size * 48000)
        if self.hop_length < 1:
            raise ValueError('hop_size must be at least one sample at 48 kHz')
        # every width, before anything runs
        D = embedding.embedding_dim()
        width = 7 * D if feature_mode == 'stats' else D
        got = _input_width(self.kind, classifier)
        if got != width:
            raise ValueError('the classifier takes %d features per row; the embedding gives %d%s' % (
                got, width, ' (7 statistics of %d)' % D if feature_mode == 'stats' else ''))
        for name, scaler, attr, want in (('min_max_scaler', self.min_max_scaler, 'scale_', D), ('stdizer', stdizer, 'scale_', width)):
            if scaler is not None and np.shape(getattr(scaler, attr)) != (want,):
                raise ValueError('%s was fitted on %s features per row, not %d' % (name, np.shape(getattr(scaler, attr)), want))
        device = int(embedding.base.device)
        if int(getattr(classifier, 'device', device)) != device:
            raise ValueError('the classifier is on device %s, the embedding on device %d' % (classifier.device, device))
        self.device = device

    @classmethod
    def from_run(cls, embedding, model_dir, hop_size=0.1):
        """The classifier a fold's run directory holds (classifier._run_fold): config.json names model_type, feature_mode,
        non_overlap and non_overlap_chunk_size; min_max_scaler.pkl and stdizer.pkl are the fitted scalers (an unfitted min-max
        scaler: that run did not scale); model.h5 (mlp) or model.pkl (svm, rf) the model, put on the embedding's GPU."""
        with open(os.path.join(model_dir, 'config.json')) as fh:
            config = json.load(fh)
        model_type = config.get('model_type')
        if model_type not in MODEL_TYPES:
            raise ValueError('%s: model_type %r; one of %s' % (os.path.join(model_dir, 'config.json'), model_type, list(MODEL_TYPES)))
        scalers = []
        for name in ('min_max_scaler.pkl', 'stdizer.pkl'):
            with open(os.path.join(model_dir, name), 'rb') as fh:
                scalers.append(pk.load(fh))
        device = int(embedding.base.device)
        if model_type == 'mlp':
            from . import kerasfile
            from .classifier import MLPModel
            weights = kerasfile.load_dense_weights(os.path.join(model_dir, 'model.h5'))
            if len(weights) != 6:
                raise ValueError('%s: %d weight arrays, not the 6 of construct_mlp_model' % (os.path.join(model_dir, 'model.h5'),
                                                                                           len(weights)))
            classifier = MLPModel(weights[0].shape[0], num_classes=weights[-1].shape[0], device=device)
            classifier.set_weights(weights)
        else:
            with open(os.path.join(model_dir, 'model.pkl'), 'rb') as fh:
                classifier = pk.load(fh)
            classifier.device = device          # pickled without its device handle: it uploads itself on first use
        return cls(embedding, classifier, scalers[1], min_max_scaler=scalers[0], feature_mode=config.get('feature_mode', 'framewise'),
                   non_overlap=bool(config.get('non_overlap', False)),
                   non_overlap_chunk_size=int(config.get('non_overlap_chunk_size', 10)), hop_size=hop_size)

    def _score(self, X, file_idxs):
        """the stages of usc._preprocess_on_device on the resident rows, in its order, then the classifier's device scoring"""
        f = X.handle
        if self.non_overlap:
            rows, file_idxs = usc.non_overlap_rows(file_idxs, self.non_overlap_chunk_size)
            f.gather(rows)
        if self.min_max_scaler is not None:
            f.affine32(self.min_max_scaler.scale_, self.min_max_scaler.min_)
        if self.feature_mode == 'stats':
            f.file_stats(file_idxs)
            file_idxs = usc._row_ranges(np.ones(len(file_idxs), dtype=np.int64))
        f.standardize(self.stdizer.mean_, self.stdizer.scale_)
        if self.kind == 'mlp':
            proba, pred = self.classifier.predict_files(X, file_idxs)
        elif self.kind == 'svm':
            got = self.classifier.evaluate(X, file_idxs=file_idxs, outputs=('file_proba', 'file_predict'))
            proba, pred = got['file_proba'], got['file_predict']
        else:
            got = self.classifier.evaluate(X, file_idxs=file_idxs, outputs=('file_mean', 'file_predict'))
            proba, pred = got['file_mean'][0], got['file_predict'][0]
        return {'file_proba': proba, 'file_predict': pred}

    def predict_clips(self, clips, rates=None):
        """clips: 1-D float32 arrays, at 48 kHz or at `rates` (whole Hz, one per clip; resampled on the GPU as load_audio does)"""
        clips = list(clips)
        if not clips:
            raise ValueError('no clips to classify')
        X, file_idxs = self.embedding.predict_clips(clips, self.hop_length, rates=rates, to_device=True)
        try:
            return self._score(X, file_idxs)
        finally:
            X.close()

    def predict_files(self, paths):
        """paths: WAV files (features.read_wav), read and embedded in usc_generate.embed_files' batches of files"""
        from .usc_generate import BATCH_FILES, BATCH_SAMPLES
        paths = list(paths)
        if not paths:
            raise ValueError('no files to classify')
        parts, i = [], 0
        while i < len(paths):
            clips, rates, total = [], [], 0
            while i < len(paths) and len(clips) < BATCH_FILES and (not clips or total < BATCH_SAMPLES):
                x, sr = read_wav(paths[i])
                clips.append(x)
                rates.append(sr)
                total += x.size
                i += 1
            parts.append(self.predict_clips(clips, rates=rates))
        return {k: np.concatenate([p[k] for p in parts]) for k in ('file_proba', 'file_predict')}
