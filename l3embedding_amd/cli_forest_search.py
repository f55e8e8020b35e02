"""Command line of the reference's 06_train_classifier.py for `-mt rf -ps` (06_train_classifier.py:5-203: the flags that apply to the
random forest's parameter search, with their defaults) driving l3embedding_amd.classifier.train_rf_search_fold(): the search over
n_estimators (classifier/train.py:623-630) fitted in one pass on the GPU.  cli_forest.py trains one forest of -rfne trees; here the
search sets the number of trees, so that flag is gone and the grid has one of its own.

    python -m l3embedding_amd.cli_forest_search --rf-num-estimators-grid 100 500 1000 <features_dir> <output_dir> <fold_num>
"""
import argparse
import logging
import sys

from . import cli_classifier, cli_forest

_SEARCH_FLAGS = ('-psnv', '-psvr', '-pstwv', '-psss')
# cli_forest's flags without -rfne, the search's flags as cli_classifier has them, and the grid
_OPTIONS = [o for o in cli_forest._OPTIONS if o[0] != '-rfne'] + [o for o in cli_classifier._OPTIONS if o[0] in _SEARCH_FLAGS] + [
    ('-rfneg', '--rf-num-estimators-grid', 'n_estimators_grid', dict(type=int, nargs='*', default=[100, 500, 1000]),
     'the forest sizes searched (classifier/train.py:626); the earlier one wins a tie'),
]
_POSITIONALS = cli_forest._POSITIONALS


def build_parser():
    p = argparse.ArgumentParser(description='Search the number of trees of a random forest sound classifier on L3 embedding '
                                            'features on the GPU (one test fold per run).')
    for short, long_, dest, settings, text in _OPTIONS:
        p.add_argument(short, long_, dest=dest, help=text, **settings)
    for name, kind, text in _POSITIONALS:
        p.add_argument(name, type=kind, help=text)
    return p


def parse_arguments(argv=None):
    """-> dict of the parsed flags: the keyword arguments of classifier.train_rf_search_fold"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    grid = args['n_estimators_grid']
    if not grid or min(grid) < 1 or len(set(grid)) != len(grid):
        p.error('--rf-num-estimators-grid: distinct forest sizes of at least one tree, one at least')
    if not args['parameter_search_valid_fold'] and args['parameter_search_split_seed'] is None:
        p.error('-psnv: ' + cli_classifier.NO_SSS)
    return args


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args['verbose'] else logging.INFO, stream=sys.stderr)
    from .classifier import train_rf_search_fold
    train_rf_search_fold(**args)


if __name__ == '__main__':
    main()
