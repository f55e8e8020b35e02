"""Throughput of embedding clips that are not at 48 kHz (data/usc/features.py:18-28 + 256-306) on one GPU, two paths:

  (a) resample every clip on the host with the NumPy restatement of resampy (tests/resample_ref.py), then
      EmbeddingModel.predict_clips on the 48 kHz clips;
  (b) EmbeddingModel.predict_clips(clips, hop, rates=...): native-rate clips uploaded, resampled on the GPU
      (csrc/resample.hip) into the buffer the frames are cut from.

Seeded weights (cnn_L3_melspec2, pooling original), hop 0.1 s, engine batch --batch.  Two synthetic US8K-shaped sets drawn from a
fixed seed: --clips clips of 1-4 s at 44.1 kHz, and the same count at rates drawn from 8 / 16 / 22.05 / 32 / 44.1 / 48 / 96 kHz.
Reported per set and path: frames/s over a host clock (calls return host arrays; (a) timed once, (b) the median of --rounds),
and whether (a) and (b) agree bit for bit.
The resample kernel's output samples and filter taps per call of (b) are counted on the host from the filter geometry.

--only-b runs path (b) on the 44.1 kHz set alone, --rounds times: the run to put under
`rocprofv3 --kernel-trace --stats`; --kernel-stats <...kernel_stats.csv> then reports the resample kernel's share of kernel time,
its output samples/s and taps/s.

    python scripts/resample_throughput.py [--clips 64] [--batch 64] [--rounds 3] [--out FILE]
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from l3embedding_amd import model, resample  # noqa: E402
from l3embedding_amd.features import frame_table  # noqa: E402

HOP = 4800
MIXED = [8000, 16000, 22050, 32000, 44100, 48000, 96000]


def make_set(n_clips, rates, seed):
    r = np.random.RandomState(seed)
    sr = [int(rates[i]) for i in r.randint(0, len(rates), size=n_clips)]
    secs = r.uniform(1.0, 4.0, size=n_clips)
    return [(0.1 * r.randn(int(s * q))).astype(np.float32) for s, q in zip(secs, sr)], sr


def taps(n, sr_o, sr_n=48000, num_table=512, nwin=32769):
    """(outputs, filter taps) of resampling n native samples at sr_o, exact output times (csrc/resample.hip)"""
    if sr_o == sr_n:
        return n, 0
    ratio = float(sr_n) / sr_o
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    t = np.arange(int(n * ratio), dtype=np.int64)
    nn = t * sr_o // sr_n
    frac = scale * ((t * sr_o - nn * sr_n) / float(sr_n))
    left = np.minimum(nn + 1, (nwin - (frac * num_table).astype(np.int64)) // step)
    right = np.minimum(n - nn - 1, (nwin - ((scale - frac) * num_table).astype(np.int64)) // step)
    return t.size, int(left.sum() + np.maximum(right, 0).sum())


def path_a(emb, clips, rates):
    from resample_ref import resample_ref
    win, nt = resample.kaiser_best()
    host = [c if r == 48000 else resample_ref(c, r, 48000, win, nt) for c, r in zip(clips, rates)]
    return emb.predict_clips(host, HOP)


def path_b(emb, clips, rates):
    return emb.predict_clips(clips, HOP, rates=rates)


def kernel_stats(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    rs = [r for r in rows if 'resample_kernel' in r['Name']]
    ns = sum(float(r['TotalDurationNs']) for r in rs)
    return ns, total, sum(int(r['Calls']) for r in rs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only-b', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    sets = [('44.1 kHz', make_set(args.clips, [44100], 1)), ('mixed', make_set(args.clips, MIXED, 2))]
    lines = []
    if args.kernel_stats:
        clips, rates = sets[0][1]
        outs, tp = map(sum, zip(*[taps(c.size, r) for c, r in zip(clips, rates)]))
        ns, total, calls = kernel_stats(args.kernel_stats)
        n_runs = args.rounds + 1                           # the warm-up pass + the timed rounds of --only-b
        lines.append('resample_kernel: %d launches, %.3f ms of %.3f ms kernel time (%.2f %%); %d outputs and %d taps per pass '
                     '-> %.3g output samples/s, %.3g taps/s'
                     % (calls, ns / 1e6, total / 1e6, 100.0 * ns / total, outs, tp, outs * n_runs / (ns * 1e-9),
                        tp * n_runs / (ns * 1e-9)))
    else:
        m = model.L3Model('cnn_L3_melspec2', seed=20180123)
        emb = model.EmbeddingModel(m, 'audio', model.AUDIO_POOLING['cnn_L3_melspec2']['original'])
        m._ensure_engine(args.batch)
        for name, (clips, rates) in (sets[:1] if args.only_b else sets):
            lengths = [c.size if r == 48000 else resample.output_length(c.size, r, 48000) for c, r in zip(clips, rates)]
            frames = int(frame_table(lengths, HOP)[1].sum())
            outs, tp = map(sum, zip(*[taps(c.size, r) for c, r in zip(clips, rates)]))
            path_b(emb, clips, rates)                      # warm-up: one whole pass
            t = {'a': [], 'b': []}
            equal = True
            for rnd in range(args.rounds):
                for p, fn in (() if args.only_b or rnd else (('a', path_a),)) + (('b', path_b),):    # (a) once: it takes minutes
                    t0 = time.perf_counter()
                    out = fn(emb, clips, rates)
                    t[p].append(time.perf_counter() - t0)
                    if p == 'a':
                        ref = out
                    elif not args.only_b:
                        equal = equal and all(np.array_equal(x, y) for x, y in zip(ref, out))
            r = {'set': name, 'clips': len(clips), 'frames': frames, 'batch': args.batch, 'outputs': outs, 'taps': tp,
                 'b_frames_per_s': frames / np.median(t['b']), 'b_s': t['b']}
            if not args.only_b:
                r.update(a_frames_per_s=frames / np.median(t['a']), a_s=t['a'], bit_equal=bool(equal))
            lines.append(json.dumps(r))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'a') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
