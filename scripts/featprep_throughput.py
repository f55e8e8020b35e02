"""Fold preprocessing, host against device (record profiles/r15_featprep.txt): seconds of usc.preprocess_split_data on
US8K-shaped splits (files of 31 frames) in NumPy on the host and with device=0 (uploads included), the hand-off to the MLP that
follows either (l3_mlp_set_data's upload / l3_mlp_set_data_dev's copy), peak host RSS, and each kernel's achieved HBM rate.

    python scripts/featprep_throughput.py [--dims 512 6144] [--n-train 200000] [--n-held 28000] [--reps 3]

Every (D, feature mode, path) runs in a process of its own, so that ru_maxrss is that path's peak; a JSON line per process."""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES = 31


def make_split(rng, n, D):
    n_files = n // FRAMES
    n = n_files * FRAMES
    x = rng.standard_normal((n, D), dtype=np.float32)
    ends = np.arange(1, n_files + 1, dtype=np.int64) * FRAMES
    return {'features': x, 'labels': rng.integers(0, 10, size=n_files), 'file_idxs': np.stack((ends - FRAMES, ends), axis=1),
            'filenames': []}


def fresh(master):
    return [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()} for d in master]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def child(a):
    from l3embedding_amd import _lib, usc
    rng = np.random.default_rng(a.D)
    master = [make_split(rng, n, a.D) for n in (a.n_train, a.n_held, a.n_held)]
    device = 0 if a.path == 'device' else None
    rec = dict(D=a.D, mode=a.mode, path=a.path, rows=[len(d['features']) for d in master], preprocess_s=[], handoff_s=[])
    _lib.MLP(8, 2, 2).close()          # the HIP runtime and the code objects are loaded before anything is timed
    for _ in range(a.reps):
        splits = fresh(master)
        np.random.seed(1)
        t, _ = timed(lambda: usc.preprocess_split_data(*splits, feature_mode=a.mode, use_min_max=True, device=device))
        rec['preprocess_s'].append(round(t, 4))
        tr, va, _ = splits
        width = tr['features'].shape[1]
        m = _lib.MLP(width, 10, 64)
        yt, yv = np.asarray(tr['labels'], np.int32), np.asarray(va['labels'], np.int32)
        if device is None:
            t, _ = timed(lambda: m.set_data(tr['features'], yt, va['features'], yv))
        else:
            t, _ = timed(lambda: m.set_data_dev(tr['features'].handle, 0, len(yt), yt, va['features'].handle, 0, len(yv), yv))
        rec['handoff_s'].append(round(t, 4))
        m.close()
        del splits, tr, va
    if device is not None:
        # each kernel on the training matrix alone (every call waits for the device): bytes the algorithm moves / seconds
        x = master[0]['features']
        n, D = x.shape
        f = _lib.Features(x)
        B = 4.0 * n * D
        ops = [('minmax', f.minmax, B), ('affine32', lambda: f.affine32(np.ones(D, np.float32), np.zeros(D, np.float32)), 2 * B),
               ('moments', f.moments, 2 * B), ('standardize', lambda: f.standardize(np.zeros(D), np.ones(D)), 2 * B),
               ('gather', lambda: f.gather(np.random.RandomState(0).permutation(n)), 2 * B),
               ('file_stats', lambda: f.file_stats(master[0]['file_idxs']), B + 28.0 * len(master[0]['file_idxs']) * D)]
        rec['kernels_TBps'] = {}
        for name, fn, nbytes in ops:
            if name != 'file_stats':
                fn()          # warm
            best = min(timed(fn)[0] for _ in range(1 if name == 'file_stats' else 3))
            rec['kernels_TBps'][name] = round(nbytes / best / 1e12, 3)
        f.close()
    rec['peak_rss_GiB'] = round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20, 2)
    rec['input_GiB'] = round(sum(d['features'].nbytes for d in master) / 2.0 ** 30, 2)
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--dims', type=int, nargs='+', default=[512, 6144])
    p.add_argument('--n-train', type=int, default=200000)
    p.add_argument('--n-held', type=int, default=28000)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--child', nargs=3, metavar=('D', 'MODE', 'PATH'))
    a = p.parse_args()
    if a.child:
        a.D, a.mode, a.path = int(a.child[0]), a.child[1], a.child[2]
        return child(a)
    for D in a.dims:
        for mode in ('framewise', 'stats'):
            for path in ('host', 'device'):
                subprocess.check_call([sys.executable, os.path.abspath(__file__), '--n-train', str(a.n_train), '--n-held',
                                       str(a.n_held), '--reps', str(a.reps), '--child', str(D), mode, path])


if __name__ == '__main__':
    main()
