"""Command line of the principal components of an embedding (pca.py).

    python -m l3embedding_amd.cli_pca fit --features A.npz [...] --n-components 50 [--whiten] --out model.npz
                                          [--solver full|subspace|auto] [--oversample N] [--tol T] [--max-iter N] [--seed N]

PCA over the frames of the embedding files that cli_embedding_samples wrote (X: the frames of one clip, y: its class).  A path may be a
directory of such files.  --n-components: an integer, a fraction in (0, 1) of the variance to keep, or `all`.  model.npz holds mean,
components, explained_variance, explained_variance_ratio, n_samples and whiten.  --solver subspace finds the components by block
subspace iteration on the GPU instead of an eigendecomposition of the whole covariance on the host (pca.PCA; an integer
--n-components); --oversample, --tol, --max-iter and --seed are its block width beyond the components, its residual tolerance, its
limit of products and the seed of its start.

    python -m l3embedding_amd.cli_pca transform --model model.npz --features F --out G

F: one embedding file, or a directory of them; G: the file, or the directory, of the same layout to write.  Every file of G holds the
projected frames as X (n_frames, k) and every other array of its file of F (y, and whatever else it carries) unchanged, so
cli_cluster, cli_knn and cli_tsne read G as they read F.
"""
import argparse
import logging
import os
import sys

import numpy as np

from .cli_knn import _entries, _load


def _n_components(text):
    if text == 'all':
        return None
    try:
        value = int(text)
    except ValueError:
        try:
            value = float(text)
        except ValueError:
            raise argparse.ArgumentTypeError('an integer, a fraction in (0, 1) or `all`, not %r' % text)
        if not 0.0 < value < 1.0:
            raise argparse.ArgumentTypeError('a fraction of the variance lies in (0, 1), not %r' % text)
        return value
    if value < 1:
        raise argparse.ArgumentTypeError('at least 1 component, not %d' % value)
    return value


def build_parser():
    p = argparse.ArgumentParser(description='Principal components of embedding frames on the GPU: fit a model, project files onto it.')
    sub = p.add_subparsers(dest='command')
    sub.required = True
    fit = sub.add_parser('fit', help='PCA over the frames of embedding files')
    fit.add_argument('--features', nargs='+', required=True, help='.npz embedding files (or directories of them)')
    fit.add_argument('--n-components', type=_n_components, required=True, help='components to keep: an integer, a fraction in (0, 1), or all')
    fit.add_argument('--whiten', action='store_true', default=False, help='projections of unit variance')
    fit.add_argument('--device', type=int, default=0, help='GPU index')
    fit.add_argument('--out', type=str, required=True, help='the .npz file of the model')
    # (absent unless given: the keyword arguments of fit() keep their defaults)
    fit.add_argument('--solver', choices=('full', 'subspace', 'auto'), default=argparse.SUPPRESS, help='eigensolver (default: full)')
    fit.add_argument('--oversample', type=int, default=argparse.SUPPRESS, help='subspace solver: vectors beyond the components (default: max(32, k // 4))')
    fit.add_argument('--tol', type=float, default=argparse.SUPPRESS, help='subspace solver: residual tolerance relative to the largest eigenvalue (default: 1e-9)')
    fit.add_argument('--max-iter', type=int, default=argparse.SUPPRESS, help='subspace solver: limit of products (default: 500)')
    fit.add_argument('--seed', type=int, default=argparse.SUPPRESS, help='subspace solver: seed of the starting block (default: 0)')
    tr = sub.add_parser('transform', help="project embedding files onto a model's components")
    tr.add_argument('--model', type=str, required=True, help='model.npz written by `fit`')
    tr.add_argument('--features', type=str, required=True, help='an .npz embedding file, or a directory of them')
    tr.add_argument('--device', type=int, default=0, help='GPU index')
    tr.add_argument('--out', type=str, required=True, help='the file (or directory) to write, of the same layout')
    return p


def parse_arguments(argv=None):
    """-> (command, dict of the parsed flags): the keyword arguments of fit() or transform()"""
    args = vars(build_parser().parse_args(argv))
    return args.pop('command'), args


def fit(features, n_components, out, whiten=False, device=0, solver='full', oversample=None, tol=1e-9, max_iter=500, seed=0):
    """the `fit` command -> the path written"""
    from .pca import PCA
    model = PCA(n_components, whiten=whiten, device=device, solver=solver, oversample=oversample, tol=tol, max_iter=max_iter, random_state=seed)
    X = _load(_entries(features))[0]
    try:
        model.fit(X)
    finally:
        model.close()
    np.savez(out, mean=model.mean_, components=model.components_, explained_variance=model.explained_variance_,
             explained_variance_ratio=model.explained_variance_ratio_, n_samples=model.n_samples_, whiten=model.whiten)
    return out


def load_model(path, device=0):
    """the PCA that `fit` wrote to `path`"""
    from .pca import PCA
    with np.load(path) as npz:
        return PCA.from_arrays(np.ascontiguousarray(npz['mean'], np.float32), np.ascontiguousarray(npz['components'], np.float32),
                               explained_variance=npz['explained_variance'], whiten=bool(npz['whiten']), device=device)


def _frames(X):
    """a file's X as cli_knn._load takes it: one row per frame"""
    X = np.asarray(X)
    return np.ascontiguousarray(X.reshape(len(X), -1) if X.ndim != 1 else X.reshape(1, -1), np.float32)


def transform(model, features, out, device=0):
    """the `transform` command -> the paths written"""
    pca = load_model(model, device=device)
    if os.path.isdir(features):
        sources = _entries([features])
        os.makedirs(out, exist_ok=True)
        targets = [os.path.join(out, os.path.basename(f)) for f in sources]
    else:
        sources, targets = [features], [out]
    width = pca.components_.shape[1]
    try:
        for src, dst in zip(sources, targets):
            with np.load(src) as npz:
                arrays = {k: npz[k] for k in npz.files}
            rows = _frames(arrays['X'])
            if rows.shape[1] != width:
                raise ValueError('%s: %d features per frame, the model has %d' % (src, rows.shape[1], width))
            arrays['X'] = pca.transform(rows)
            with open(dst, 'wb') as fh:          # (a file object: numpy appends no extension of its own)
                np.savez(fh, **arrays)
    finally:
        pca.close()
    return targets


def main(argv=None):
    command, args = parse_arguments(argv)
    logging.basicConfig(level=logging.INFO, stream=sys.stderr)
    return fit(**args) if command == 'fit' else transform(**args)


if __name__ == '__main__':
    main()
