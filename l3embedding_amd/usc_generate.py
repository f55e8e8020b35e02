"""Embedding feature folds of the downstream sound-classification sets -- the reference's data/usc/us8k.py, esc50.py and
dcase2013.py generation (driven by 05_generate_embedding_samples.py), restated for the GPU pipeline.  features='vggish' with a
vggish_model (vggish.VGGishModel) writes the VGGish baseline's features into the same layout.

Per fold k (counted from 1): <output_dir>/fold<k>/<basename>.npz with X the (n_frames, D) embeddings of the file and y its class
index, written with np.savez_compressed -- the layout usc.get_fold reads.  A file whose .npz exists already is skipped.  What
differs from the reference is how the files reach the model: many files go into one EmbeddingModel.predict_clips call, each at
its own sample rate (rates=...), and are resampled to 48 kHz and framed on the device.  The embeddings equal those of
get_l3_frames_uniform on features.read_audio(path, 48000) file by file up to the last bits: packing puts a frame on another row
of an engine batch, where the solo Winograd tail split can sum it in another order.

Labels: US8K from the metadata CSV's classID, each clip's variants found by the reference's glob (<stem>[!0-9]*[wm][ap][v3],
recursive, .jams excluded); ESC-50 the last '-' field of the basename; DCASE 2013 CLASS_TO_INT[basename[:-2]].  mp3 variants are
skipped with an error log (soundfile, which the reference reads with, does not read mp3 either).
"""
import csv
import glob
import logging
import os
import random

import numpy as np

from .features import read_wav

LOGGER = logging.getLogger('cls-data-generation')

NUM_FOLDS = {'us8k': 10, 'esc50': 5, 'dcase2013': 2}
DCASE2013_CLASS_TO_INT = {'bus': 0, 'busystreet': 1, 'office': 2, 'openairmarket': 3, 'park': 4, 'quietstreet': 5,
                          'restaurant': 6, 'supermarket': 7, 'tube': 8, 'tubestation': 9}
SR = 48000
# files per predict_clips call: at most this many, and at most this many native samples (128 MiB of float32) unless one file is
# larger on its own
BATCH_FILES = 256
BATCH_SAMPLES = 1 << 25


def load_us8k_metadata(path):
    """data/usc/us8k.py:17-38: one {slice_file_name: row} dict per fold, rows with numeric start, end, salience, fold, classID"""
    metadata = [{} for _ in range(NUM_FOLDS['us8k'])]
    with open(path) as csvfile:
        for row in csv.DictReader(csvfile):
            row['start'] = float(row['start'])
            row['end'] = float(row['end'])
            row['salience'] = float(row['salience'])
            fold_num = row['fold'] = int(row['fold'])
            row['classID'] = int(row['classID'])
            metadata[fold_num - 1][row['slice_file_name']] = row
    return metadata


def us8k_variants(audio_fold_dir, fname):
    """the variant files of one US8K clip: us8k.py:128-131's glob, recursive, files only, no .jams"""
    pattern = os.path.join(audio_fold_dir, '**', os.path.splitext(fname)[0] + '[!0-9]*[wm][ap][v3]')
    return [x for x in glob.glob(pattern, recursive=True) if os.path.isfile(x) and not x.endswith('.jams')]


def _seed_fold(random_state, fold_idx):
    # us8k.py:110-113 / esc50.py:30-33 / dcase2013.py:43-46: the RNGs seeded per fold
    random.seed(random_state + fold_idx)
    np.random.seed(random_state + fold_idx)


def _fold_dirs(data_dir, output_dir, fold_idx):
    out = os.path.join(output_dir, 'fold{}'.format(fold_idx + 1))
    if not os.path.isdir(out):
        os.makedirs(out)
    LOGGER.info('Generating fold {} in {}'.format(fold_idx + 1, out))
    return os.path.join(data_dir, 'fold{}'.format(fold_idx + 1)), out


def _check_features(features, l3embedding_model, vggish_model=None):
    if features == 'vggish' and vggish_model:
        return
    if features != 'l3':
        raise ValueError('Invalid feature type: {} (l3, or vggish with a vggish_model)'.format(features))
    if not l3embedding_model:
        raise ValueError('Must provide L3 embedding model to use {} features'.format(features))


def embed_files(jobs, l3embedding_model, hop_size=0.1, features='l3', vggish_model=None, **_):
    """jobs: (audio_path, output_path, label) in order.  Files whose output exists, or is the output of an earlier job, are
    skipped, mp3 files are skipped with an error log; the rest are read (features.read_wav), embedded in batches of many files
    by one predict_clips(..., rates=...) call each, and written as <output_path> {X, y}.  features='vggish': the batches go to
    vggish_model.predict_clips(clips, rates, hop_size=...) (vggish.VGGishModel) instead.  Returns the output paths written."""
    hop_length = int(hop_size * SR)
    todo, claimed = [], set()
    for audio_path, output_path, label in jobs:
        # a second job with the same output (US8K variants of one name in two sub-directories) finds the first one's file in
        # the reference, which writes each file before it looks at the next
        if os.path.exists(output_path) or output_path in claimed:
            LOGGER.info('File {} already exists'.format(output_path))
        elif audio_path.lower().endswith('.mp3'):
            LOGGER.error('Could not generate data for {}: mp3 files are not read'.format(audio_path))
        else:
            todo.append((audio_path, output_path, label))
            claimed.add(output_path)
    written = []
    i = 0
    while i < len(todo):
        clips, rates, batch, total = [], [], [], 0
        while i < len(todo) and len(batch) < BATCH_FILES and (not batch or total < BATCH_SAMPLES):
            x, sr = read_wav(todo[i][0])
            clips.append(x)
            rates.append(sr)
            batch.append(todo[i])
            total += x.size
            i += 1
        if features == 'vggish':
            embeddings = vggish_model.predict_clips(clips, rates, hop_size=hop_size)
        else:
            embeddings = l3embedding_model.predict_clips(clips, hop_length, rates=rates)
        for (audio_path, output_path, label), X in zip(batch, embeddings):
            np.savez_compressed(output_path, X=X, y=label)
            LOGGER.debug('Processed {}'.format(audio_path))
            written.append(output_path)
    return written


def generate_us8k_fold_data(metadata, data_dir, fold_idx, output_dir, l3embedding_model=None, features='l3',
                            random_state=12345678, vggish_model=None, **feature_args):
    """us8k.py:70-134 for one fold (fold_idx counted from 0); metadata as load_us8k_metadata returns it, or the CSV's path"""
    _check_features(features, l3embedding_model, vggish_model)
    if isinstance(metadata, str):
        metadata = load_us8k_metadata(metadata)
    _seed_fold(random_state, fold_idx)
    audio_fold_dir, out = _fold_dirs(data_dir, output_dir, fold_idx)
    jobs = []
    for fname, example_metadata in metadata[fold_idx].items():
        for var_path in us8k_variants(audio_fold_dir, fname):
            basename = os.path.splitext(os.path.basename(var_path))[0]
            jobs.append((var_path, os.path.join(out, basename + '.npz'), example_metadata['classID']))
    return embed_files(jobs, l3embedding_model, features=features, vggish_model=vggish_model, **feature_args)


def generate_us8k_folds(metadata_path, data_dir, output_dir, l3embedding_model=None, features='l3', random_state=12345678,
                        vggish_model=None, **feature_args):
    LOGGER.info('Generating all folds.')
    metadata = load_us8k_metadata(metadata_path)
    for fold_idx in range(NUM_FOLDS['us8k']):
        generate_us8k_fold_data(metadata, data_dir, fold_idx, output_dir, l3embedding_model=l3embedding_model,
                                features=features, random_state=random_state, vggish_model=vggish_model, **feature_args)


def _generate_listed_fold(data_dir, fold_idx, output_dir, label_of, l3embedding_model, features, random_state, vggish_model,
                          feature_args):
    # esc50.py:25-51 / dcase2013.py:38-64: every entry of the fold directory, in glob order
    _check_features(features, l3embedding_model, vggish_model)
    _seed_fold(random_state, fold_idx)
    audio_fold_dir, out = _fold_dirs(data_dir, output_dir, fold_idx)
    jobs = []
    for f in glob.glob(audio_fold_dir + '/*'):
        basename = os.path.splitext(os.path.basename(f))[0]
        jobs.append((f, os.path.join(out, basename + '.npz'), label_of(basename)))
    return embed_files(jobs, l3embedding_model, features=features, vggish_model=vggish_model, **feature_args)


def esc50_label(basename):
    return int(basename.split('-')[-1])         # esc50.py:70


def dcase2013_label(basename):
    return DCASE2013_CLASS_TO_INT[basename[:-2]]     # dcase2013.py:84


def generate_esc50_fold_data(data_dir, fold_idx, output_dir, l3embedding_model=None, features='l3', random_state=12345678,
                             vggish_model=None, **feature_args):
    return _generate_listed_fold(data_dir, fold_idx, output_dir, esc50_label, l3embedding_model, features, random_state,
                                 vggish_model, feature_args)


def generate_esc50_folds(data_dir, output_dir, l3embedding_model=None, features='l3', random_state=12345678, vggish_model=None,
                         **feature_args):
    for fold_idx in range(NUM_FOLDS['esc50']):
        generate_esc50_fold_data(data_dir, fold_idx, output_dir, l3embedding_model=l3embedding_model, features=features,
                                 random_state=random_state, vggish_model=vggish_model, **feature_args)


def generate_dcase2013_fold_data(data_dir, fold_idx, output_dir, l3embedding_model=None, features='l3', random_state=12345678,
                                 vggish_model=None, **feature_args):
    return _generate_listed_fold(data_dir, fold_idx, output_dir, dcase2013_label, l3embedding_model, features, random_state,
                                 vggish_model, feature_args)


def generate_dcase2013_folds(data_dir, output_dir, l3embedding_model=None, features='l3', random_state=12345678,
                             vggish_model=None, **feature_args):
    for fold_idx in range(NUM_FOLDS['dcase2013']):
        generate_dcase2013_fold_data(data_dir, fold_idx, output_dir, l3embedding_model=l3embedding_model, features=features,
                                     random_state=random_state, vggish_model=vggish_model, **feature_args)
