"""The parameter search without a validation fold (record profiles/r19_param_search_split.txt), in one process, every
timing after a warm-up call.

    python scripts/param_search_throughput.py [--rows 65536] [--dim 6144] [--files 2000] [--frames 41] [--epochs 20] [--reps 5]

1. l3_feat_split alone: a (--rows, --dim) matrix cut 85 / 15 by a random permutation, against the two other ways to the same bytes:
     split              one Features.split: both matrices from one launch
     assemble+gather x2 the only route before l3_feat_split: per part a whole copy of the source (Features.assemble) and an in-place
                        Features.gather of its rows
     assemble (copy)    Features.assemble of the whole source: the same bytes read once and written once, in order
   One JSON line each: best and median wall seconds of a call (allocation, table upload and the final synchronisation included) and
   GB/s of the bytes the two new matrices hold, read + written (2 * 4 * rows * dim).  The three results are compared for equal bits
   first.
2. One ESC-50-shaped fold (--files files of --frames frames, four fifths of them the training side, thinned to every 10th frame) of
   the MLP's nine-point search with parameter_search_valid_fold=False, --epochs epochs per run, through classifier.train:
     resident           preprocess_device=0: the splits are uploaded once, preprocessed and cut on the GPU, and every run takes them there
     host               preprocess_device=None: NumPy preprocesses and cuts, and every run uploads its matrices again
   One JSON line each: wall seconds and the bytes uploaded (feature matrices handed to DeviceFeatures, MLP.set_data and MLP.predict).
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps):
    """-> (best, median) wall seconds of fn() over `reps` calls after one warm-up call; fn returns what is to be closed"""
    seconds = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        made = fn()
        dt = time.perf_counter() - t0
        for m in made:
            m.close()
        if rep:
            seconds.append(dt)
    return min(seconds), float(np.median(seconds))


def split_rate(rows, dim, reps):
    import torch  # noqa: F401  (one HIP runtime for torch and libl3hip)
    from l3embedding_amd import _lib
    x = np.random.default_rng(0).standard_normal((rows, dim), dtype=np.float32)
    src = _lib.Features(x, device=0)
    perm = np.random.RandomState(1).permutation(rows)
    cut = rows - int(np.ceil(0.15 * rows))
    rows_a, rows_b = perm[:cut], perm[cut:]

    def split():
        return src.split(rows_a, rows_b)

    def parent_route():
        parts = []
        for table in (rows_a, rows_b):
            part = _lib.Features.assemble([(src, 0, rows)], device=0)
            parts.append(part)
            part.gather(table)
        return parts

    def plain_copy():
        return [_lib.Features.assemble([(src, 0, rows)], device=0)]

    # the same bits by either route, before anything is timed
    a, b = split()
    pa, pb = parent_route()
    same = all(np.array_equal(g.download().view(np.uint32), w.download().view(np.uint32)) and
               np.array_equal(g.download().view(np.uint32), x[t].view(np.uint32)) for g, w, t in ((a, pa, rows_a), (b, pb, rows_b)))
    for f in (a, b, pa, pb):
        f.close()
    if not same:
        print(json.dumps({'part': 'split', 'failed': 'the routes differ'}), flush=True)
        return 1
    moved = 2 * 4 * rows * dim
    lines = {}
    for name, fn in (('split', split), ('assemble+gather x2', parent_route), ('assemble (copy)', plain_copy)):
        best, median = timed(fn, reps)
        lines[name] = best
        print(json.dumps({'part': 'split', 'route': name, 'rows': rows, 'D': dim, 'rows_a': int(cut), 'rows_b': int(rows - cut),
                          'GB_read_and_written': round(moved / 1e9, 3), 'best_call_s': round(best, 6), 'median_call_s': round(median, 6),
                          'GBps': round(moved / best / 1e9, 1)}), flush=True)
    print(json.dumps({'part': 'split', 'split_over_parent_route': round(lines['split'] / lines['assemble+gather x2'], 3),
                      'split_over_plain_copy': round(lines['split'] / lines['assemble (copy)'], 3),
                      'split_slower_than_parent_route': bool(lines['split'] > lines['assemble+gather x2'])}), flush=True)
    src.close()
    return 0


def search_fold(files, frames, dim, epochs):
    import torch  # noqa: F401
    from l3embedding_amd import _lib, classifier, usc
    r = np.random.default_rng(2)
    n_test = files // 5

    def side(n_files, first_label):
        labels = (first_label + np.arange(n_files)) % 50
        X = r.standard_normal((n_files * frames, dim), dtype=np.float32)
        X += (labels.repeat(frames) % 7).astype(np.float32)[:, None] * 0.25
        return {'features': X, 'labels': labels, 'file_idxs': usc._row_ranges(np.full(n_files, frames)), 'filenames': []}
    train_side, test_side = side(files - n_test, 0), side(n_test, 3)
    classifier.get_split = lambda *a, **k: (dict(train_side), None, dict(test_side))

    uploaded = [0]

    def counting(fn, picks):
        def counted(self, *args, **kwargs):
            for i in picks:
                if i < len(args) and isinstance(args[i], np.ndarray):
                    uploaded[0] += args[i].astype(np.float32, copy=False).nbytes
            return fn(self, *args, **kwargs)
        return counted
    usc.DeviceFeatures.__init__ = counting(usc.DeviceFeatures.__init__, (0,))
    _lib.MLP.set_data = counting(_lib.MLP.set_data, (0, 2))
    _lib.MLP.predict = counting(_lib.MLP.predict, (0,))

    feats = os.path.join('synthetic', 'features', 'esc50', 'l3', 'synthetic_%d' % dim)
    args = dict(model_type='mlp', parameter_search=True, parameter_search_valid_fold=False, parameter_search_split_seed=7,
                parameter_search_train_with_valid=False, non_overlap=True, non_overlap_chunk_size=10, num_epochs=epochs, random_state=1)
    out = tempfile.mkdtemp(prefix='param_search_out_')
    try:
        results = {}
        for route, device in (('warm-up', 0), ('resident', 0), ('host', None), ('resident', 0), ('host', None)):
            uploaded[0] = 0
            np.random.seed(5)
            t0 = time.perf_counter()
            fold_dir = classifier.train(feats, out, 1, preprocess_device=device, **(dict(args, num_epochs=1) if route == 'warm-up' else args))
            wall = time.perf_counter() - t0
            if route == 'warm-up':
                continue
            with open(os.path.join(fold_dir, 'results.pkl'), 'rb') as fh:
                import pickle
                best = pickle.load(fh)['valid']['search_params_best_values']
            results.setdefault(route, []).append(wall)
            print(json.dumps({'part': 'search', 'route': route, 'files': files, 'frames': frames, 'D': dim, 'epochs': epochs,
                              'training_rows_after_thinning': int((files - n_test) * len(range(0, frames, 10))), 'wall_s': round(wall, 3),
                              'GB_uploaded': round(uploaded[0] / 1e9, 3), 'chosen': list(best)}), flush=True)
        print(json.dumps({'part': 'search', 'resident_over_host_wall': round(min(results['resident']) / min(results['host']), 3)}),
              flush=True)
    finally:
        shutil.rmtree(out, ignore_errors=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rows', type=int, default=65536)
    ap.add_argument('--dim', type=int, default=6144)
    ap.add_argument('--files', type=int, default=2000)
    ap.add_argument('--frames', type=int, default=41)
    ap.add_argument('--epochs', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', choices=['split', 'search'])
    args = ap.parse_args()
    if args.only != 'search':
        rc = split_rate(args.rows, args.dim, args.reps)
        if rc:
            return rc          # nothing more is started on the GPU after a failure
    if args.only != 'split':
        return search_fold(args.files, args.frames, args.dim, args.epochs)
    return 0


if __name__ == '__main__':
    sys.exit(main())
