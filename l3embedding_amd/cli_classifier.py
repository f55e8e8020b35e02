"""Command line of the reference's 06_train_classifier.py (same flags, same defaults: 06_train_classifier.py:5-203) driving
l3embedding_amd.classifier.train().  The fold driver runs the MLP alone: `-mt svm` (the default, as in the reference; the SVM
itself is classifier.train_svm) and `-mt rf` fail at once, and so does `-psnv` without `--parameter-search-split-seed N`: the
stratified cut of the training rows it searches on is drawn from that seed (usc.stratified_shuffle_split; the reference draws an
unseeded one with sklearn's StratifiedShuffleSplit).

    python -m l3embedding_amd.cli_classifier -mt mlp -e 150 -lr 1e-4 -wd 1e-5 <features_dir> <output_dir> <fold_num>
"""
import argparse
import logging
import sys

from .classifier import NO_SSS, ONLY_MLP


# (short flag, long flag, dest, argparse settings, help) -- flags, dests and defaults are those of 06_train_classifier.py
_OPTIONS = [
    ('-e', '--num-epochs', 'num_epochs', dict(type=int, default=150), 'MLP: epoch limit (early stopping may end sooner)'),
    ('-tbs', '--train-batch-size', 'train_batch_size', dict(type=int, default=64), 'MLP: rows per Adam step'),
    ('-eap', '--early-stopping-patience', 'patience', dict(type=int, default=20),
     'MLP: epochs without a lower val_loss tolerated before stopping'),
    ('-ps', '--parameter-search', 'parameter_search', dict(action='store_true'),
     'grid-search learning rate and weight decay on the validation fold'),
    ('-psnv', '--parameter-search-no-valid-fold', 'parameter_search_valid_fold', dict(action='store_false'),
     'search on a stratified split of the training folds instead of the validation fold (needs --parameter-search-split-seed)'),
    ('-psvr', '--parameter-search-valid-ratio', 'parameter_search_valid_ratio', dict(type=float, default=0.15),
     'share of the training rows such a split holds out'),
    ('-pstwv', '--parameter-search-train-without-valid', 'parameter_search_train_with_valid', dict(action='store_false'),
     'after the search keep the chosen run instead of retraining on train + validation'),
    ('-lr', '--learning-rate', 'learning_rate', dict(type=float, default=1e-4), 'MLP: Adam learning rate'),
    ('-wd', '--weight-decay', 'weight_decay', dict(type=float, default=1e-5), 'MLP: L2 factor on the three kernels'),
    ('-npf', '--norm-penalty-factor', 'C', dict(type=float, default=1.0), 'SVM only (classifier.train_svm): C'),
    ('-sct', '--svm-conv-tolerance', 'tol', dict(type=float, default=0.00001), 'SVM only (classifier.train_svm): tolerance'),
    ('-smi', '--svm-max-iterations', 'max_iterations', dict(type=int, default=-1), 'SVM only (classifier.train_svm): iteration cap'),
    ('-skt', '--svm-kernel-type', 'kernel', dict(type=str, default='rbf', choices=['rbf', 'sigmoid', 'linear', 'poly']),
     'SVM only (classifier.train_svm): kernel'),
    ('-rfne', '--rf-num-estimators', 'n_estimators', dict(type=int, default=100), 'random forest only (not built): trees'),
    ('-gsid', '--gsheet-id', 'gsheet_id', dict(type=str), 'accepted and ignored (no spreadsheet logging)'),
    ('-gdan', '--google-dev-app-name', 'google_dev_app_name', dict(type=str), 'accepted and ignored'),
    ('-r', '--random-state', 'random_state', dict(type=int, default=20171021),
     'seed of the initial weights and of the per-epoch shuffle'),
    ('-v', '--verbose', 'verbose', dict(action='store_true', default=False), 'log every epoch'),
    ('-fm', '--feature-mode', 'feature_mode', dict(type=str, default='framewise', choices=['framewise', 'stats']),
     'framewise: one row per frame; stats: seven statistics per file'),
    ('-mt', '--model-type', 'model_type', dict(type=str, default='svm', choices=['svm', 'mlp', 'rf']),
     'classifier; only mlp is built'),
    ('-no', '--non-overlap', 'non_overlap', dict(action='store_true', default=False),
     'thin each file to every n-th frame (n = --non-overlap-chunk-size)'),
    ('-nocs', '--non-overlap-chunk-size', 'non_overlap_chunk_size', dict(default=10), 'n of --non-overlap'),
    ('-umm', '--use-min-max', 'use_min_max', dict(action='store_true', default=False),
     'scale features to [0, 1] (fitted on the training rows) before standardising'),
    # not a flag of 06_train_classifier.py: the folds are preprocessed on this GPU and handed to the MLP there
    ('-ppd', '--preprocess-device', 'preprocess_device', dict(type=int, default=None),
     'preprocess the folds on this GPU instead of in NumPy on the host'),
    # not a flag of 06_train_classifier.py either: the reference's stratified split is unseeded, here every draw has a seed
    ('-psss', '--parameter-search-split-seed', 'parameter_search_split_seed', dict(type=int, default=None),
     'seed of the stratified split -psnv searches on; -psnv is refused without it'),
]
_POSITIONALS = [
    ('features_dir', str, 'directory holding fold1 .. foldN of .npz feature files; its path names the dataset after features/'),
    ('output_dir', str, 'where the classifier/... run directory is created'),
    ('fold_num', int, 'test fold, counted from 1'),
]


def build_parser():
    p = argparse.ArgumentParser(description='Train and cross-validate a sound classifier on L3 embedding features '
                                            '(one test fold per run).')
    for short, long_, dest, settings, text in _OPTIONS:
        p.add_argument(short, long_, dest=dest, help=text, **settings)
    for name, kind, text in _POSITIONALS:
        p.add_argument(name, type=kind, help=text)
    return p


def parse_arguments(argv=None):
    """-> dict of the parsed flags; exits with status 2 and a message for what is not built (svm, rf, -psnv without a split seed)"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    if args['model_type'] != 'mlp':
        p.error(ONLY_MLP.format(args['model_type']))
    if not args['parameter_search_valid_fold'] and args['parameter_search_split_seed'] is None:
        p.error('-psnv: ' + NO_SSS)
    return args


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args['verbose'] else logging.INFO, stream=sys.stderr)
    from .classifier import train
    train(**args)


if __name__ == '__main__':
    main()
