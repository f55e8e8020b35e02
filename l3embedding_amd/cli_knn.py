"""Command line of the nearest-neighbour read-outs of an embedding (knn.py).

    python -m l3embedding_amd.cli_knn fold [-knn 5] [--metric cosine] [-ps] <features_dir> <output_dir> <fold_num>

One cross-validation fold of the k-nearest-neighbour classifier (classifier.train_knn_fold, or train_knn_search_fold with -ps): the
flags of cli_forest that apply, plus --n-neighbors, --metric and the parameter search's.

    python -m l3embedding_amd.cli_knn neighbors --database A.npz [...] --queries B.npz [...] --k 5 --metric cosine --out lists.npz

Query by example on the embedding files that cli_embedding_samples wrote (X: the frames of one clip, y: its class): every frame of
the query files against every frame of the database files.  A path may be a directory of such files.  Each file is one entry and
the entries are the groups: a query frame is not given neighbours from the database entry of its own name, so a set may be
queried against itself.  lists.npz holds idx and dist (n_query_frames, k), the entry and frame of every query and database row
(query_entry, query_frame, database_entry, database_frame), the entries' names and the database rows' labels.
"""
import argparse
import logging
import os
import sys

import numpy as np

# (short flag, long flag, dest, argparse settings, help) -- the shared flags, dests and defaults are those of cli_forest
_FOLD_OPTIONS = [
    ('-knn', '--n-neighbors', 'n_neighbors', dict(type=int, default=5), 'neighbours that vote (ignored with --parameter-search)'),
    ('-m', '--metric', 'metric', dict(type=str, default='sqeuclidean', choices=['cosine', 'sqeuclidean']), 'distance'),
    ('-ps', '--parameter-search', 'parameter_search', dict(action='store_true', default=False),
     'choose n_neighbors among 1, 3, 5, 10, 20, 50 by validation accuracy'),
    ('-psnv', '--parameter-search-no-valid-fold', 'parameter_search_valid_fold', dict(action='store_false', default=True),
     'search on a cut of the training rows instead of the validation fold (needs --parameter-search-split-seed)'),
    ('-psvr', '--parameter-search-valid-ratio', 'parameter_search_valid_ratio', dict(type=float, default=0.15), 'size of that cut'),
    ('-pstwv', '--parameter-search-train-with-valid', 'parameter_search_train_with_valid', dict(action='store_true', default=False),
     'refit the chosen size on the training and validation rows together'),
    ('-psss', '--parameter-search-split-seed', 'parameter_search_split_seed', dict(type=int, default=None), 'seed of that cut'),
    ('-r', '--random-state', 'random_state', dict(type=int, default=20171021), 'recorded in config.json; nothing here is random'),
    ('-v', '--verbose', 'verbose', dict(action='store_true', default=False), 'log at debug level'),
    ('-fm', '--feature-mode', 'feature_mode', dict(type=str, default='framewise', choices=['framewise', 'stats']),
     'framewise: one row per frame; stats: seven statistics per file'),
    ('-no', '--non-overlap', 'non_overlap', dict(action='store_true', default=False),
     'thin each file to every n-th frame (n = --non-overlap-chunk-size)'),
    ('-nocs', '--non-overlap-chunk-size', 'non_overlap_chunk_size', dict(type=int, default=10), 'n of --non-overlap'),
    ('-umm', '--use-min-max', 'use_min_max', dict(action='store_true', default=False),
     'scale features to [0, 1] (fitted on the training rows) before standardising'),
    ('-ppd', '--preprocess-device', 'preprocess_device', dict(type=int, default=None),
     'preprocess the folds on this GPU instead of in NumPy on the host'),
]
_FOLD_POSITIONALS = [
    ('features_dir', str, 'directory holding fold1 .. foldN of .npz feature files; its path names the dataset after features/'),
    ('output_dir', str, 'where the classifier/... run directory is created'),
    ('fold_num', int, 'test fold, counted from 1'),
]
_SEARCH_ONLY = ('parameter_search_valid_fold', 'parameter_search_valid_ratio', 'parameter_search_train_with_valid',
                'parameter_search_split_seed')


def build_parser():
    p = argparse.ArgumentParser(description='Nearest neighbours in embedding space on the GPU: a k-NN sound classifier fold, or '
                                            'query by example on embedding files.')
    sub = p.add_subparsers(dest='command')
    sub.required = True
    fold = sub.add_parser('fold', help='one cross-validation fold of the k-nearest-neighbour classifier')
    for short, long_, dest, settings, text in _FOLD_OPTIONS:
        fold.add_argument(short, long_, dest=dest, help=text, **settings)
    for name, kind, text in _FOLD_POSITIONALS:
        fold.add_argument(name, type=kind, help=text)
    nb = sub.add_parser('neighbors', help='the nearest database frames of every query frame')
    nb.add_argument('--database', nargs='+', required=True, help='.npz embedding files (or directories of them) to search in')
    nb.add_argument('--queries', nargs='+', required=True, help='.npz embedding files (or directories of them) to search for')
    nb.add_argument('--k', type=int, default=5, help='neighbours per query frame (1 .. 64)')
    nb.add_argument('--metric', type=str, default='sqeuclidean', choices=['cosine', 'sqeuclidean'], help='distance')
    nb.add_argument('--device', type=int, default=0, help='GPU index')
    nb.add_argument('--out', type=str, required=True, help='the .npz file of the lists')
    return p


def parse_arguments(argv=None):
    """-> (command, dict of the parsed flags): for 'fold' the keyword arguments of classifier.train_knn_fold, or of
    train_knn_search_fold when 'parameter_search' is set (the key is taken out by main); for 'neighbors' those of neighbors()"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    command = args.pop('command')
    if command == 'fold' and not 1 <= args['n_neighbors'] <= 64:
        p.error('-knn: between 1 and 64 neighbours')
    if command == 'neighbors' and not 1 <= args['k'] <= 64:
        p.error('--k: between 1 and 64 neighbours')
    return command, args


def _entries(paths):
    """the .npz files that the paths name (a directory: its .npz files, sorted), in order"""
    files = []
    for path in paths:
        if os.path.isdir(path):
            files.extend(os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith('.npz'))
        else:
            files.append(path)
    if not files:
        raise ValueError('no .npz files under %s' % (paths,))
    return files


def _load(files):
    """-> (rows (n, D) float32, entry of every row, frame of every row, label of every row, entry names)"""
    rows, entry, frame, label, names = [], [], [], [], []
    for e, path in enumerate(files):
        with np.load(path) as npz:
            X, y = np.asarray(npz['X']), np.asarray(npz['y'])
        X = X.reshape(len(X), -1) if X.ndim != 1 else X.reshape(1, -1)
        rows.append(np.ascontiguousarray(X, np.float32))
        entry.append(np.full(len(X), e, np.int32))
        frame.append(np.arange(len(X), dtype=np.int32))
        label.append(np.broadcast_to(y.reshape(-1), (len(X),)).astype(np.int64))          # one label for the clip, or one per frame
        names.append(os.path.splitext(os.path.basename(path))[0])
    return np.concatenate(rows), np.concatenate(entry), np.concatenate(frame), np.concatenate(label), names


def neighbors(database, queries, k, metric, out, device=0):
    """the `neighbors` command -> the path written"""
    from .knn import NearestNeighbors
    X, x_entry, x_frame, x_label, x_names = _load(_entries(database))
    Q, q_entry, q_frame, _, q_names = _load(_entries(queries))
    if X.shape[1] != Q.shape[1]:
        raise ValueError('the database rows have %d features, the queries %d' % (X.shape[1], Q.shape[1]))
    group_of = {}          # entries of the same name on the two sides share a group
    gx = np.array([group_of.setdefault(x_names[e], len(group_of)) for e in x_entry], np.int32)
    gq = np.array([group_of.setdefault(q_names[e], len(group_of)) for e in q_entry], np.int32)
    nn = NearestNeighbors(n_neighbors=k, metric=metric, device=device).fit(X)
    try:
        dist, idx = nn.kneighbors(Q, groups_q=gq, groups_fit=gx)
    finally:
        nn.close()
    np.savez(out, idx=idx, dist=dist, query_entry=q_entry, query_frame=q_frame, database_entry=x_entry, database_frame=x_frame,
             database_label=x_label, query_names=np.array(q_names), database_names=np.array(x_names), k=k, metric=metric)
    return out


def main(argv=None):
    command, args = parse_arguments(argv)
    if command == 'neighbors':
        logging.basicConfig(level=logging.INFO, stream=sys.stderr)
        return neighbors(**args)
    logging.basicConfig(level=logging.DEBUG if args['verbose'] else logging.INFO, stream=sys.stderr)
    from . import classifier
    if args.pop('parameter_search'):
        args.pop('n_neighbors')
        return classifier.train_knn_search_fold(**args)
    for name in _SEARCH_ONLY:
        args.pop(name)
    return classifier.train_knn_fold(**args)


if __name__ == '__main__':
    main()
