"""Command line of the two-dimensional map of an embedding (tsne.py).

    python -m l3embedding_amd.cli_tsne fit --features A.npz [...] --perplexity 20 --seed S --out map.npz [--per-file] [--plot map.png]

t-SNE over the frames of the embedding files that cli_embedding_samples wrote (X: the frames of one clip, y: its class), read as
cli_cluster fit reads them.  A path may be a directory of such files; each file is one entry.  With --per-file a file's frames are
averaged first and the map has one point per file.  map.npz holds the map (embedding, (n, 2) float32), the entry, frame and class of
every point, the entries' names, the KL records (history_iteration, history_kl, history_z), kl_divergence, n_neighbors, the
perplexity and the seed.  --plot draws the map coloured by class; it is the only part that needs matplotlib.
"""
import argparse
import logging
import sys

import numpy as np

from .cli_knn import _entries, _load


def build_parser():
    p = argparse.ArgumentParser(description='Map embedding frames (or file means) to the plane on the GPU (t-SNE).')
    sub = p.add_subparsers(dest='command')
    sub.required = True
    fit = sub.add_parser('fit', help='t-SNE over the frames of embedding files')
    fit.add_argument('--features', nargs='+', required=True, help='.npz embedding files (or directories of them)')
    fit.add_argument('--perplexity', type=float, default=20.0, help='effective number of neighbours, in (1, 21]')
    fit.add_argument('--seed', type=int, required=True, help='seed of the initial map (nothing is drawn unseeded)')
    fit.add_argument('--n-iter', type=int, default=1000, help='iterations in all')
    fit.add_argument('--exaggeration-iter', type=int, default=250, help='iterations of the early exaggeration')
    fit.add_argument('--early-exaggeration', type=float, default=12.0, help='factor on P in the early iterations')
    fit.add_argument('--metric', type=str, default='sqeuclidean', choices=['sqeuclidean', 'cosine'], help='distance of the neighbour lists')
    fit.add_argument('--per-file', action='store_true', default=False, help="map each file's mean frame instead of every frame")
    fit.add_argument('--plot', type=str, default=None, help='also draw the map into this image file (needs matplotlib)')
    fit.add_argument('--device', type=int, default=0, help='GPU index')
    fit.add_argument('--out', type=str, required=True, help='the .npz file of the map')
    return p


def parse_arguments(argv=None):
    """-> (command, dict of the parsed flags): the keyword arguments of fit()"""
    p = build_parser()
    args = vars(p.parse_args(argv))
    command = args.pop('command')
    if not 1.0 < args['perplexity'] <= 21.0:
        p.error('--perplexity: in (1, 21] (a neighbour list holds at most 64 entries)')
    if args['n_iter'] < 1 or not 0 <= args['exaggeration_iter'] <= args['n_iter']:
        p.error('--n-iter: at least 1; --exaggeration-iter: between 0 and --n-iter')
    if not args['early_exaggeration'] >= 1.0:
        p.error('--early-exaggeration: at least 1')
    if not 0 <= args['seed'] < 2 ** 32:
        p.error('--seed: in [0, 2^32)')
    return command, args


def file_means(X, entry):
    """(the float32 mean row of every entry in float64 arithmetic, the first row of every entry); an entry's rows are consecutive"""
    starts = np.flatnonzero(np.r_[True, entry[1:] != entry[:-1]])
    sums = np.add.reduceat(X.astype(np.float64), starts, axis=0)
    counts = np.diff(np.r_[starts, len(entry)])
    return (sums / counts[:, None]).astype(np.float32), starts


def draw(path, Y, label):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(figsize=(8, 8))
    ax.scatter(Y[:, 0], Y[:, 1], c=label, s=4, cmap='tab20', linewidths=0)
    ax.set_xticks([])
    ax.set_yticks([])
    fig.savefig(path, dpi=150, bbox_inches='tight')
    plt.close(fig)
    return path


def fit(features, seed, out, perplexity=20.0, n_iter=1000, exaggeration_iter=250, early_exaggeration=12.0, metric='sqeuclidean', per_file=False,
        plot=None, device=0):
    """the `fit` command -> the path written"""
    from .tsne import TSNE
    X, entry, frame, label, names = _load(_entries(features))
    if per_file:
        X, starts = file_means(X, entry)
        entry, frame, label = entry[starts], np.zeros(len(starts), np.int32), label[starts]
    model = TSNE(perplexity=perplexity, n_iter=n_iter, exaggeration_iter=exaggeration_iter, early_exaggeration=early_exaggeration, metric=metric,
                 random_state=seed, device=device)
    try:
        model.fit(X)
    finally:
        model.close()
    np.savez(out, embedding=model.embedding_, entry=entry, frame=frame, class_label=label, names=np.array(names),
             history_iteration=model.history_['iteration'], history_kl=model.history_['kl'], history_z=model.history_['z'],
             kl_divergence=model.kl_divergence_, n_neighbors=model.n_neighbors_, perplexity=perplexity, seed=seed, per_file=per_file)
    if plot:
        draw(plot, model.embedding_, label)
    return out


def main(argv=None):
    command, args = parse_arguments(argv)
    logging.basicConfig(level=logging.INFO, stream=sys.stderr)
    return fit(**args)


if __name__ == '__main__':
    main()
