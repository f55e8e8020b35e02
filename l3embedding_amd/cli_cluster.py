"""Command line of the clustering read-out of an embedding (cluster.py).

    python -m l3embedding_amd.cli_cluster fit --features A.npz [...] --clusters K --seed S [--n-init 8] --out model.npz

k-means over the frames of the embedding files that cli_embedding_samples wrote (X: the frames of one clip, y: its class).  A path may
be a directory of such files; each file is one entry.  model.npz holds the centroids, the label, distance, entry and frame of every
row, the entries' names, the history of the winning restart (history_inertia, history_changed, history_empty), inertia, n_iter,
chosen (the seed rows) and, since the files carry class labels, the contingency table with nmi, purity and adjusted_rand.

    python -m l3embedding_amd.cli_cluster histograms --model model.npz --features B.npz [...] --out hist.npz

The bag-of-words rows of other files under the model's codebook: hist (n_files, K) int32 counts of each file's frames per cluster,
the files' names and each file's class (label).
"""
import argparse
import logging
import sys

import numpy as np

from .cli_knn import _entries, _load


def build_parser():
    p = argparse.ArgumentParser(description='Cluster embedding frames on the GPU (k-means) and build per-file histograms of the clusters.')
    sub = p.add_subparsers(dest='command')
    sub.required = True
    fit = sub.add_parser('fit', help='k-means over the frames of embedding files')
    fit.add_argument('--features', nargs='+', required=True, help='.npz embedding files (or directories of them)')
    fit.add_argument('--clusters', type=int, required=True, help='number of clusters K (1 .. 65536, at most the number of frames)')
    fit.add_argument('--seed', type=int, required=True, help='seed of the seeding and the restarts (nothing is drawn unseeded)')
    fit.add_argument('--n-init', type=int, default=8, help='restarts; the lowest inertia wins')
    fit.add_argument('--max-iter', type=int, default=300, help='Lloyd iterations per restart at most')
    fit.add_argument('--init', type=str, default='k-means++', choices=['k-means++', 'random'], help='seeding')
    fit.add_argument('--device', type=int, default=0, help='GPU index')
    fit.add_argument('--out', type=str, required=True, help='the .npz file of the model')
    hist = sub.add_parser('histograms', help="per-file histograms of a model's clusters")
    hist.add_argument('--model', type=str, required=True, help='model.npz written by `fit`')
    hist.add_argument('--features', nargs='+', required=True, help='.npz embedding files (or directories of them)')
    hist.add_argument('--normalize', action='store_true', default=False, help="shares of a file's frames instead of counts")
    hist.add_argument('--device', type=int, default=0, help='GPU index')
    hist.add_argument('--out', type=str, required=True, help='the .npz file of the histograms')
    return p


def parse_arguments(argv=None):
    """-> (command, dict of the parsed flags): the keyword arguments of fit() or histograms()"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    command = args.pop('command')
    if command == 'fit':
        if not 1 <= args['clusters'] <= 65536:
            p.error('--clusters: between 1 and 65536')
        if args['n_init'] < 1 or args['max_iter'] < 1:
            p.error('--n-init and --max-iter: at least 1')
        if not 0 <= args['seed'] < 2 ** 32:
            p.error('--seed: in [0, 2^32)')
    return command, args


def fit(features, clusters, seed, out, n_init=8, max_iter=300, init='k-means++', device=0):
    """the `fit` command -> the path written"""
    from .cluster import KMeans
    X, entry, frame, label, names = _load(_entries(features))
    km = KMeans(clusters, init=init, n_init=n_init, max_iter=max_iter, random_state=seed, device=device)
    try:
        km.fit(X)
        extra = {}
        if label.min() >= 0 and label.max() < 256:
            got = km.scores(label)
            extra = dict(contingency=got['table'], nmi=got['nmi'], purity=got['purity'], adjusted_rand=got['adjusted_rand'])
    finally:
        km.close()
    np.savez(out, centroids=km.cluster_centers_, labels=km.labels_, distances=km.distances_, entry=entry, frame=frame, class_label=label,
             names=np.array(names), history_inertia=km.history_['inertia'], history_changed=km.history_['changed'],
             history_empty=km.history_['empty'], inertia=km.inertia_, n_iter=km.n_iter_, chosen=km.chosen_, seed=seed, init=init, **extra)
    return out


def histograms(model, features, out, normalize=False, device=0):
    """the `histograms` command -> the path written"""
    from .cluster import KMeans
    with np.load(model) as npz:
        centroids = np.ascontiguousarray(npz['centroids'], np.float32)
    X, entry, _, label, names = _load(_entries(features))
    if X.shape[1] != centroids.shape[1]:
        raise ValueError('the model has %d features per centroid, the files %d per frame' % (centroids.shape[1], X.shape[1]))
    starts = np.flatnonzero(np.r_[True, entry[1:] != entry[:-1]])          # a file's rows are consecutive
    file_idxs = np.stack([starts, np.r_[starts[1:], len(entry)]], axis=1).astype(np.int64)
    km = KMeans.from_centroids(centroids, device=device)
    try:
        hist = km.file_histograms(file_idxs, X=X, normalize=normalize)
    finally:
        km.close()
    np.savez(out, hist=hist, names=np.array(names), label=label[starts], file_idxs=file_idxs)
    return out


def main(argv=None):
    command, args = parse_arguments(argv)
    logging.basicConfig(level=logging.INFO, stream=sys.stderr)
    return fit(**args) if command == 'fit' else histograms(**args)


if __name__ == '__main__':
    main()
