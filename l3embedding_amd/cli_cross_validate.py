"""Command line of classifier.cross_validate: every fold of a dataset in one run, from folds read once and kept on the GPU.  The flags
are those of cli_classifier (the reference's 06_train_classifier.py) without the positional fold number, plus --folds and
--fold-seed; `-mt svm` (the default) and `-mt mlp` run, `-mt rf` fails at once as it does there, and so does `-psnv` without
`--parameter-search-split-seed N` (with it, both classifiers search on a stratified cut of the training rows drawn from that seed).

    python -m l3embedding_amd.cli_cross_validate -mt svm -ppd 0 <features_dir> <output_dir>
"""
import argparse
import logging
import sys

from .classifier import NO_SSS, ONLY_MLP
from .cli_classifier import _OPTIONS, _POSITIONALS


def build_parser():
    p = argparse.ArgumentParser(description='Cross-validate a sound classifier on L3 embedding features (all test folds in one run).')
    for short, long_, dest, settings, text in _OPTIONS:
        if dest == 'preprocess_device':          # here the folds live on a GPU unless told otherwise
            settings, text = dict(settings, default=0), 'GPU that keeps and preprocesses the folds (-1: the host, in NumPy)'
        if dest == 'model_type':
            text = 'classifier; svm and mlp are built'
        p.add_argument(short, long_, dest=dest, help=text, **settings)
    p.add_argument('--folds', dest='folds', type=int, nargs='+', default=None, metavar='N',
                   help='test folds to run, counted from 1 (default: all of the dataset\'s)')
    p.add_argument('--fold-seed', dest='fold_seed', type=int, default=None,
                   help='seed NumPy\'s global state with this before every fold (default: leave it alone)')
    for name, kind, text in _POSITIONALS:
        if name != 'fold_num':
            p.add_argument(name, type=kind, help=text)
    return p


def parse_arguments(argv=None):
    """-> dict of cross_validate's arguments; exits with status 2 and a message for what is not built (rf, -psnv without a split seed)"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    if args['model_type'] not in ('svm', 'mlp'):
        p.error(ONLY_MLP.format(args['model_type']))
    if not args['parameter_search_valid_fold'] and args['parameter_search_split_seed'] is None:
        p.error('-psnv: ' + NO_SSS)
    if args['preprocess_device'] is not None and args['preprocess_device'] < 0:
        args['preprocess_device'] = None
    return args


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args['verbose'] else logging.INFO, stream=sys.stderr)
    from .classifier import cross_validate
    print(cross_validate(**args))


if __name__ == '__main__':
    main()
