"""Cross-validation of a US8K-shaped synthetic dataset, the per-fold loop against classifier.cross_validate.

    python scripts/crossval_throughput.py --dims 512 6144 --files-per-fold 60

writes a tree of 10 folds (files of 1 to 31 frames, `--augmented` augmented copies per file with '_' in their names, 10 classes) per D
and times, each in a process of its own:

  loop       the per-fold way: train_svm_fold(preprocess_device=0) for fold 1 .. 10, every call reading its folds through get_split
  crossval   cross_validate(model_type='svm', preprocess_device=0): one FoldBank, every split assembled on the GPU

One JSON line each: wall_s; the phases read_s (np.load of feature files), upload_s (host matrix -> l3_feat), assemble_s
(l3_feat_assemble), preprocess_s (preprocess_split_data without the uploads inside it), fit_score_s (train_svm); files_read;
assemble_TBps (bytes read + written by the copy / its seconds, launch and table upload included, to hold against the ~5.2 TB/s of the
project's streaming kernels; --copy-rows N times the copy alone on a matrix of N rows); device_high_water_GiB (the largest drop of free device memory below its value at start, sampled
at the end of every phase, so a peak inside a fit is not seen); dataset_GiB.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_tree(root, D, files_per_fold, augmented, seed=0):
    r = np.random.RandomState(seed)
    centres = r.randn(10, D).astype(np.float32)
    feats = os.path.join(root, 'features', 'us8k', 'l3', 'synthetic_%d' % D)
    rows = 0
    for fold in range(1, 11):
        d = os.path.join(feats, 'fold%d' % fold)
        os.makedirs(d)
        for i in range(files_per_fold):
            label = (fold + i) % 10
            for copy in range(1 + augmented):
                n = int(r.randint(1, 32))
                X = centres[label] + 2.0 * r.randn(n, D).astype(np.float32)
                name = '%d-%d.npz' % (label, i) if copy == 0 else '%d-%d_aug%d.npz' % (label, i, copy)
                np.savez(os.path.join(d, name), X=X, y=np.array(label))
                rows += n
    return feats, rows


class Phases(object):
    """seconds spent inside the wrapped functions, nested time taken off the enclosing phase"""

    def __init__(self):
        import torch
        self.torch = torch
        self.seconds = {k: 0.0 for k in ('read', 'upload', 'assemble', 'preprocess', 'fit_score')}
        self.files_read = 0
        self.assemble_bytes = 0
        self.stack = []
        self.free_at_start = torch.cuda.mem_get_info(0)[0]
        self.min_free = self.free_at_start

    def wrap(self, phase, fn, after=None):
        def timed(*args, **kwargs):
            self.stack.append(0.0)
            t0 = time.perf_counter()
            try:
                out = fn(*args, **kwargs)
            finally:
                dt = time.perf_counter() - t0
                inner = self.stack.pop()
                self.seconds[phase] += dt - inner
                if self.stack:
                    self.stack[-1] += dt
                self.min_free = min(self.min_free, self.torch.cuda.mem_get_info(0)[0])
            if after:
                after(out)
            return out
        return timed


def run(mode, feats):
    import torch  # noqa: F401  (one HIP runtime for torch and libl3hip)
    from l3embedding_amd import classifier, usc
    ph = Phases()

    def count_file(_):
        ph.files_read += 1

    def count_bytes(out):
        n, d = out.shape
        ph.assemble_bytes += 8 * n * d
    usc.load_feature_file = ph.wrap('read', usc.load_feature_file, count_file)
    usc.DeviceFeatures.__init__ = ph.wrap('upload', usc.DeviceFeatures.__init__)
    assemble = usc.DeviceFeatures.assemble.__func__
    usc.DeviceFeatures.assemble = classmethod(ph.wrap('assemble', assemble, count_bytes))
    classifier.preprocess_split_data = ph.wrap('preprocess', classifier.preprocess_split_data)
    classifier.train_svm = ph.wrap('fit_score', classifier.train_svm)
    out = tempfile.mkdtemp(prefix='crossval_out_')
    t0 = time.perf_counter()
    try:
        if mode == 'loop':
            for fold in range(1, 11):
                classifier.train_svm_fold(feats, out, fold, preprocess_device=0)
        else:
            classifier.cross_validate(feats, out, model_type='svm', preprocess_device=0)
        wall = time.perf_counter() - t0
    finally:
        shutil.rmtree(out, ignore_errors=True)
    line = {'mode': mode, 'wall_s': round(wall, 3), 'files_read': ph.files_read}
    line.update({k + '_s': round(v, 3) for k, v in ph.seconds.items()})
    line['other_s'] = round(wall - sum(ph.seconds.values()), 3)
    if ph.seconds['assemble'] > 0:
        line['assemble_TBps'] = round(ph.assemble_bytes / ph.seconds['assemble'] / 1e12, 4)
        line['assemble_GiB_moved'] = round(ph.assemble_bytes / 2 ** 30, 3)
    line['device_high_water_GiB'] = round((ph.free_at_start - ph.min_free) / 2 ** 30, 3)
    return line


def copy_rate(n_rows, D, reps=5):
    """l3_feat_assemble alone at a training split's shape (nine whole folds) and at a held-out US8K fold's (one range per kept file,
    every third file dropped): best wall seconds of a call, the new matrix's allocation and the final synchronisation included"""
    import torch  # noqa: F401
    from l3embedding_amd import _lib
    r = np.random.RandomState(0)
    per_fold = n_rows // 10
    block = r.randn(per_fold, D).astype(np.float32)
    folds = [_lib.Features(block, device=0) for _ in range(10)]
    ends = np.minimum(np.cumsum(r.randint(1, 32, size=per_fold)), per_fold)
    ends = np.unique(ends)
    files = [(int(lo), int(hi)) for i, (lo, hi) in enumerate(zip(np.r_[0, ends[:-1]], ends)) if i % 3]
    shapes = {'train (9 segments)': [(f, 0, per_fold) for f in folds[:9]],
              'per file (%d segments)' % (9 * len(files)): [(f, lo, hi) for f in folds[:9] for lo, hi in files]}
    for name, segs in shapes.items():
        best, moved = None, 0
        for _ in range(reps):
            t0 = time.perf_counter()
            out = _lib.Features.assemble(segs, device=0)
            dt = time.perf_counter() - t0
            moved = 8 * out.shape[0] * out.shape[1]
            out.close()
            best = dt if best is None else min(best, dt)
        print(json.dumps({'mode': 'copy', 'shape': name, 'D': D, 'rows': moved // (8 * D), 'GiB_moved': round(moved / 2 ** 30, 3),
                          'best_call_s': round(best, 6), 'TBps': round(moved / best / 1e12, 3)}), flush=True)
    for f in folds:
        f.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--dims', type=int, nargs='+', default=[512, 6144])
    ap.add_argument('--files-per-fold', type=int, default=60)
    ap.add_argument('--augmented', type=int, default=2, help='augmented copies per file')
    ap.add_argument('--copy-rows', type=int, default=0, help='also time l3_feat_assemble alone on about this many rows per D')
    ap.add_argument('--mode', choices=['loop', 'crossval', 'copy'], help='(internal) run one mode on --tree and print its line')
    ap.add_argument('--tree')
    args = ap.parse_args()
    if args.mode == 'copy':
        for D in args.dims:
            copy_rate(args.copy_rows, D)
        return 0
    if args.mode:
        print(json.dumps(run(args.mode, args.tree)), flush=True)
        return 0
    root = tempfile.mkdtemp(prefix='crossval_tree_')
    try:
        for D in args.dims:
            feats, rows = write_tree(root, D, args.files_per_fold, args.augmented)
            for mode in ('loop', 'crossval'):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--mode', mode, '--tree', feats], stdout=subprocess.PIPE)
                if r.returncode != 0:
                    print(json.dumps({'mode': mode, 'D': D, 'failed': r.returncode}), flush=True)
                    return r.returncode          # nothing more is started on the GPU after a failure
                line = json.loads(r.stdout.decode().strip().splitlines()[-1])
                line.update(D=D, rows=rows, files=10 * args.files_per_fold * (1 + args.augmented),
                            dataset_GiB=round(4.0 * rows * D / 2 ** 30, 3))
                print(json.dumps(line), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if args.copy_rows:
        return subprocess.run([sys.executable, os.path.abspath(__file__), '--mode', 'copy', '--copy-rows', str(args.copy_rows),
                               '--dims'] + [str(D) for D in args.dims]).returncode
    return 0


if __name__ == '__main__':
    sys.exit(main())
