"""Command line of the reference's 06_train_classifier.py for `-mt mlp -ps` (06_train_classifier.py:5-203: the flags that apply to the
MLP's parameter search, with their defaults) driving l3embedding_amd.classifier.train_mlp_search_fold(): the search over learning
rate and weight decay (classifier/train.py:638-651) fitted as one group of models on the GPU.  cli_classifier.py -mt mlp -ps runs the
same search one fit after the other; the results are the same, bit for bit.  -lr and -wd are accepted and recorded as there; the
search sets both.

    python -m l3embedding_amd.cli_mlp_search -e 150 -ppd 0 <features_dir> <output_dir> <fold_num>
"""
import argparse
import logging
import sys

from . import cli_classifier

# cli_classifier's flags without the model type, the switch that turns the search on and the other models' own
_NOT_HERE = ('-mt', '-ps', '-npf', '-sct', '-smi', '-skt', '-rfne')
_OPTIONS = [o for o in cli_classifier._OPTIONS if o[0] not in _NOT_HERE]
_POSITIONALS = cli_classifier._POSITIONALS


def build_parser():
    p = argparse.ArgumentParser(description='Search the learning rate and weight decay of an MLP sound classifier on L3 embedding '
                                            'features as one group of models on the GPU (one test fold per run).')
    for short, long_, dest, settings, text in _OPTIONS:
        p.add_argument(short, long_, dest=dest, help=text, **settings)
    for name, kind, text in _POSITIONALS:
        p.add_argument(name, type=kind, help=text)
    return p


def parse_arguments(argv=None):
    """-> dict of the parsed flags: the keyword arguments of classifier.train_mlp_search_fold"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    if not args['parameter_search_valid_fold'] and args['parameter_search_split_seed'] is None:
        p.error('-psnv: ' + cli_classifier.NO_SSS)
    return args


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args['verbose'] else logging.INFO, stream=sys.stderr)
    from .classifier import train_mlp_search_fold
    train_mlp_search_fold(**args)


if __name__ == '__main__':
    main()
