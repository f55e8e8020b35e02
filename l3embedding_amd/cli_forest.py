"""Command line of the reference's 06_train_classifier.py for `-mt rf` (06_train_classifier.py:5-203: the flags that apply to the
random forest, with their defaults) driving l3embedding_amd.classifier.train_rf_fold().  cli_classifier.py still refuses `-mt rf`;
this is the forest's own entry point, as train_rf_fold is beside train().

    python -m l3embedding_amd.cli_forest -rfne 100 <features_dir> <output_dir> <fold_num>
"""
import argparse
import logging
import sys

# (short flag, long flag, dest, argparse settings, help) -- flags, dests and defaults are those of 06_train_classifier.py
_OPTIONS = [
    ('-rfne', '--rf-num-estimators', 'n_estimators', dict(type=int, default=100), 'trees of the forest'),
    ('-r', '--random-state', 'random_state', dict(type=int, default=20171021),
     'seed of the tree seeds, the bootstrap samples and the sample of rows the cuts are taken from'),
    ('-v', '--verbose', 'verbose', dict(action='store_true', default=False), 'log at debug level'),
    ('-fm', '--feature-mode', 'feature_mode', dict(type=str, default='framewise', choices=['framewise', 'stats']),
     'framewise: one row per frame; stats: seven statistics per file'),
    ('-no', '--non-overlap', 'non_overlap', dict(action='store_true', default=False),
     'thin each file to every n-th frame (n = --non-overlap-chunk-size)'),
    ('-nocs', '--non-overlap-chunk-size', 'non_overlap_chunk_size', dict(type=int, default=10), 'n of --non-overlap'),
    ('-umm', '--use-min-max', 'use_min_max', dict(action='store_true', default=False),
     'scale features to [0, 1] (fitted on the training rows) before standardising'),
    # not a flag of 06_train_classifier.py: the folds are preprocessed on this GPU and handed to the forest there
    ('-ppd', '--preprocess-device', 'preprocess_device', dict(type=int, default=None),
     'preprocess the folds on this GPU instead of in NumPy on the host'),
]
_POSITIONALS = [
    ('features_dir', str, 'directory holding fold1 .. foldN of .npz feature files; its path names the dataset after features/'),
    ('output_dir', str, 'where the classifier/... run directory is created'),
    ('fold_num', int, 'test fold, counted from 1'),
]


def build_parser():
    p = argparse.ArgumentParser(description='Train a random forest sound classifier on L3 embedding features on the GPU '
                                            '(one test fold per run).')
    for short, long_, dest, settings, text in _OPTIONS:
        p.add_argument(short, long_, dest=dest, help=text, **settings)
    for name, kind, text in _POSITIONALS:
        p.add_argument(name, type=kind, help=text)
    return p


def parse_arguments(argv=None):
    """-> dict of the parsed flags: the keyword arguments of classifier.train_rf_fold"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    if args['n_estimators'] < 1:
        p.error('-rfne: at least one tree')
    return args


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args['verbose'] else logging.INFO, stream=sys.stderr)
    from .classifier import train_rf_fold
    train_rf_fold(**args)


if __name__ == '__main__':
    main()
