"""Command line of the reference's 05_generate_embedding_samples.py (same flags, same defaults: 05_...py:15-106) driving
l3embedding_amd.usc_generate: the L3 embedding feature folds of UrbanSound8K, ESC-50 or DCASE 2013, written under
<output_dir>/features/<dataset>/l3/<pooling>/<embedding desc>/fold<k>/ where classifier.train reads them.  `-f vggish -vrd DIR`
writes the VGGish baseline's features under <output_dir>/features/<dataset>/vggish/ (05_...py:160) from the two .npz files in DIR
(vggish.py); `-f vggish` without -vrd fails at once.

    python -m l3embedding_amd.cli_embedding_samples -lmp <.../embedding/<desc>/model.h5> esc50 <data_dir> <output_dir>
"""
import argparse
import json
import logging
import os
import sys

from . import usc_generate

LOGGER = logging.getLogger('cls-data-generation')

# (short flag, long flag, dest, argparse settings, help) -- flags, dests and defaults are those of 05_generate_embedding_samples.py
_OPTIONS = [
    ('-r', '--random-state', 'random_state', dict(type=int, default=20171021), 'seed of the per-fold RNG state (seed + fold)'),
    ('-v', '--verbose', 'verbose', dict(action='store_true', default=False), 'log every file'),
    ('-f', '--features', 'features', dict(type=str, default='l3'), 'feature type: l3, or vggish with -vrd'),
    ('-lmp', '--l3embedding-model-path', 'l3embedding_model_path', dict(type=str),
     'L3 weights file; its path below ".../embedding/" names the output directory and the model type'),
    ('-lpt', '--l3embedding-pooling-type', 'l3embedding_pooling_type', dict(type=str, default='original'),
     'pooling of the last convolution of the embedding'),
    ('-hs', '--hop-size', 'hop_size', dict(type=float, default=0.1), 'hop between 1-second frames, in seconds'),
    ('-nrs', '--num-random-samples', 'num_random_samples', dict(type=int), 'accepted; L3 features do not use it'),
    ('-g', '--gpus', 'gpus', dict(type=int, default=0), 'number of GPUs the embedding model is loaded for'),
    ('--fold', None, 'fold', dict(type=int), 'fold to generate, counted from 1; all folds when absent'),
    ('-vrd', '--vggish-resources-dir', 'vggish_resources_dir', dict(type=str, default=argparse.SUPPRESS),
     'directory of vggish_model.npz and vggish_pca_params.npz (with -f vggish)'),
    ('-ump', '--us8k-metadata-path', 'us8k_metadata_path', dict(type=str), 'UrbanSound8K metadata CSV (us8k only)'),
]
# -vrd is this project's own flag: absent from the parsed dict unless given, so the reference's set of keys stays as it is
_POSITIONALS = [
    ('dataset_name', dict(type=str, choices=['us8k', 'esc50', 'dcase2013']), 'dataset'),
    ('data_dir', dict(type=str), 'directory holding fold1 .. foldN of audio files'),
    ('output_dir', dict(type=str), 'where features/<dataset>/... is created'),
]


def build_parser():
    p = argparse.ArgumentParser(description='Generate L3 embedding feature folds of a sound-classification dataset.')
    for short, long_, dest, settings, text in _OPTIONS:
        p.add_argument(*([short] + ([long_] if long_ else [])), dest=dest, help=text, **settings)
    for name, settings, text in _POSITIONALS:
        p.add_argument(name, help=text, **settings)
    return p


def parse_arguments(argv=None):
    """-> dict of the parsed flags; exits with status 2 and a message for what is not built (-f other than l3) or missing"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    if args['features'] == 'vggish' and not args.get('vggish_resources_dir'):
        p.error('-f vggish: needs -vrd, the directory of vggish_model.npz and vggish_pca_params.npz (reading the TF '
                'checkpoint itself needs TensorFlow)')
    if args['features'] not in ('l3', 'vggish'):
        p.error('-f {}: only l3 and vggish features are built'.format(args['features']))
    if args['features'] == 'l3' and not args['l3embedding_model_path']:
        p.error('Must provide model path is L3 embedding features are used')
    if args['dataset_name'] == 'us8k' and not args['us8k_metadata_path']:
        p.error('Must provide metadata file for UrbanSound8k')
    return args


def embedding_desc(model_path):
    """05_...py:137-139: the part of the weights path after 'embedding/' up to the file's directory"""
    return model_path[model_path.rindex('embedding') + 10:os.path.dirname(model_path).rindex('/')]


def features_dir(args):
    if args['features'] == 'vggish':
        return os.path.join(args['output_dir'], 'features', args['dataset_name'], args['features'])      # 05_...py:160
    return os.path.join(args['output_dir'], 'features', args['dataset_name'], args['features'],
                        args['l3embedding_pooling_type'], embedding_desc(args['l3embedding_model_path']))


def main(argv=None):
    args = parse_arguments(argv)
    logging.basicConfig(level=logging.DEBUG if args['verbose'] else logging.INFO, stream=sys.stderr)
    LOGGER.info('Configuration: {}'.format(str(args)))
    from . import model
    out = features_dir(args)
    l3model = vggish_model = None
    if args['features'] == 'vggish':
        from . import vggish
        LOGGER.info('Loading VGGish model...')
        vggish_model = vggish.VGGishModel(args['vggish_resources_dir'])
    else:
        desc = embedding_desc(args['l3embedding_model_path'])
        LOGGER.info('Loading embedding model...')
        l3model = model.load_embedding(args['l3embedding_model_path'], desc.split('/')[-1], 'audio',
                                       args['l3embedding_pooling_type'], tgt_num_gpus=args['gpus'])
    if not os.path.isdir(out):
        os.makedirs(out)
    args['features_dir'] = out
    config_path = os.path.join(out, 'config_{}.json'.format(args['fold']))
    with open(config_path, 'w') as f:
        json.dump(args, f)
    LOGGER.info('Saved configuration to {}'.format(config_path))

    kw = dict(l3embedding_model=l3model, features=args['features'], random_state=args['random_state'],
              hop_size=args['hop_size'], num_random_samples=args['num_random_samples'])
    if vggish_model is not None:
        kw['vggish_model'] = vggish_model
    name, fold = args['dataset_name'], args['fold']
    if name == 'us8k':
        if fold is not None:
            usc_generate.generate_us8k_fold_data(args['us8k_metadata_path'], args['data_dir'], fold - 1, out, **kw)
        else:
            usc_generate.generate_us8k_folds(args['us8k_metadata_path'], args['data_dir'], out, **kw)
    else:
        one = getattr(usc_generate, 'generate_{}_fold_data'.format(name))
        every = getattr(usc_generate, 'generate_{}_folds'.format(name))
        if fold is not None:
            one(args['data_dir'], fold - 1, out, **kw)
        else:
            every(args['data_dir'], out, **kw)
    LOGGER.info('Done!')
    return out


if __name__ == '__main__':
    main()
