"""Command line of the reference's 06_train_classifier.py for `-mt rf -ps` (06_train_classifier.py:5-203: the flags that apply to the
random forest's parameter search, with their defaults) driving l3embedding_amd.classifier.train_rf_oob_fold(): the search over
n_estimators (classifier/train.py:623-630) decided by out-of-bag accuracy, one fit of the largest forest and one out-of-bag pass at
every size on the GPU.  cli_forest_search.py decides on validation rows; here no row is held out, so with -psnv nothing is cut off
and the cut's ratio and seed (-psvr, -psss) are gone.

    python -m l3embedding_amd.cli_forest_oob -psnv --rf-num-estimators-grid 100 500 1000 <features_dir> <output_dir> <fold_num>
"""
import argparse
import logging
import sys

from . import cli_forest, cli_forest_search

_CUT_FLAGS = ('-psvr', '-psss')
_OPTIONS = [o for o in cli_forest_search._OPTIONS if o[0] not in _CUT_FLAGS]
_POSITIONALS = cli_forest._POSITIONALS


def build_parser():
    p = argparse.ArgumentParser(description='Search the number of trees of a random forest sound classifier on L3 embedding '
                                            'features by out-of-bag accuracy on the GPU (one test fold per run).')
    for short, long_, dest, settings, text in _OPTIONS:
        p.add_argument(short, long_, dest=dest, help=text, **settings)
    for name, kind, text in _POSITIONALS:
        p.add_argument(name, type=kind, help=text)
    return p


def parse_arguments(argv=None):
    """-> dict of the parsed flags: the keyword arguments of classifier.train_rf_oob_fold"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    grid = args['n_estimators_grid']
    if not grid or min(grid) < 1 or len(set(grid)) != len(grid):
        p.error('--rf-num-estimators-grid: distinct forest sizes of at least one tree, one at least')
    return args


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args['verbose'] else logging.INFO, stream=sys.stderr)
    from .classifier import train_rf_oob_fold
    train_rf_oob_fold(**args)


if __name__ == '__main__':
    main()
