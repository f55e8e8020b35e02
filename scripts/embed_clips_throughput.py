"""Throughput of audio embeddings of whole clips (data/usc/features.py:256-306) on one GPU, two paths in one process:

  (a) what a user does without predict_clips: frame each clip on the host (the reference's padding + librosa.util.frame,
      restated with NumPy), then EmbeddingModel.predict on the frames, one call per clip;
  (b) EmbeddingModel.predict_clips on all clips: every clip sent once, frames cut on the GPU, frames of consecutive clips
      packed into engine batches (db_max_scope = 'sample').

Seeded weights (cnn_L3_melspec2), a synthetic set shaped like US8K: 512 clips of 1-4 s drawn from a fixed seed, plus one
60 s clip; hop 0.1 s.  For each engine batch the two paths alternate, --rounds rounds each, after one warm-up pass each.
Reported per path: frames/s (useful frames over a host clock around calls that return host arrays, i.e. device-synchronised),
counted host-to-device bytes, computed frames / useful frames, and whether (a) and (b) agree bit for bit (else their largest
difference relative to the largest embedding value).  (a) and (b) place a frame at different rows of an engine batch; with the
solo F(4x4,3x3) tail split on (the default) the rows whose tiles fall into a launch's last partial round are summed in channel
slices, so a frame's last bits depend on its row -- for l3_embed_audio as much as for predict_clips.

    python scripts/embed_clips_throughput.py [--batches 32,64,128] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from l3embedding_amd import model  # noqa: E402
from l3embedding_amd.features import FRAME_LENGTH, frame_table  # noqa: E402

HOP = 4800


def host_frames(audio, hop_length):
    """features.py:276-300: pad (short clips) and cut into overlapping 1 s frames, (n, 1, 48000) float32 on the host."""
    L = len(audio)
    if L < FRAME_LENGTH:
        pad = FRAME_LENGTH - L
        audio = np.pad(audio, (pad // 2, pad - pad // 2), mode='constant')
    n = 1 + (len(audio) - FRAME_LENGTH) // hop_length
    x = np.lib.stride_tricks.as_strided(audio, shape=(n, FRAME_LENGTH), strides=(audio.strides[0] * hop_length, audio.strides[0]))
    return np.ascontiguousarray(x).reshape(n, 1, FRAME_LENGTH)


def make_clips(n_clips=512, seed=0):
    r = np.random.RandomState(seed)
    lengths = list(r.randint(1 * 48000, 4 * 48000 + 1, size=n_clips)) + [60 * 48000]
    return [(0.1 * r.randn(n)).astype(np.float32) for n in lengths]


def path_a(emb, clips):
    return [emb.predict(host_frames(c, HOP)) for c in clips]


def path_b(emb, clips):
    return emb.predict_clips(clips, HOP)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='32,64,128')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--model', default='cnn_L3_melspec2')
    ap.add_argument('--out', default=None, help='also write the report here')
    args = ap.parse_args()
    clips = make_clips()
    counts = frame_table([len(c) for c in clips], HOP)[1]
    useful = int(counts.sum())
    m = model.L3Model(args.model, seed=20180123)
    emb = model.EmbeddingModel(m, 'audio', model.AUDIO_POOLING[args.model]['original'])
    lines = ['# %d clips (%d of 1-4 s + one of 60 s), %.1f s of audio, %d frames at hop %d; model %s, pooling original'
             % (len(clips), len(clips) - 1, sum(len(c) for c in clips) / 48000.0, useful, HOP, args.model)]
    results = []
    for B in [int(b) for b in args.batches.split(',')]:
        e = m._ensure_engine(B)
        # counted host-to-device traffic and computed rows of each path (from the shapes each path hands the engine)
        h2d_a = sum(int(n) * FRAME_LENGTH * 4 for n in counts)
        rows_a = sum(-(-int(n) // B) * B for n in counts)
        calls = []
        real = e.embed_audio_frames

        def counting(samples, table, pool, out=None):
            calls.append((np.asarray(samples).size, len(table)))
            return real(samples, table, pool, out=out)

        e.embed_audio_frames = counting
        path_b(emb, clips[:8])                  # warm-up (both paths, every shape of the timed window's engine)
        path_a(emb, clips[:8] + clips[-1:])
        del calls[:]
        ref = None
        t = {'a': [], 'b': []}
        equal, maxrel = True, 0.0
        for rnd in range(args.rounds):
            for name, fn in (('a', path_a), ('b', path_b)):
                n_calls = len(calls)
                t0 = time.perf_counter()
                out = fn(emb, clips)
                t[name].append(time.perf_counter() - t0)
                if name == 'a':
                    ref = out
                else:
                    equal = equal and all(np.array_equal(x, y) for x, y in zip(ref, out))
                    maxrel = max([maxrel] + [float(np.abs(x - y).max() / (np.abs(x).max() + 1e-30)) for x, y in zip(ref, out)])
                    if rnd == 0:
                        first_calls = calls[n_calls:]
        e.embed_audio_frames = real
        h2d_b = sum(s * 4 + n * 24 for s, n in first_calls)
        rows_b = sum(-(-n // B) * B for _, n in first_calls)
        fa, fb = useful / np.median(t['a']), useful / np.median(t['b'])
        r = {'batch': B, 'useful_frames': useful,
             'a_frames_per_s': fa, 'b_frames_per_s': fb, 'b_over_a': fb / fa,
             'a_s': t['a'], 'b_s': t['b'],
             'a_h2d_bytes': h2d_a, 'b_h2d_bytes': h2d_b,
             'a_computed_over_useful': rows_a / useful, 'b_computed_over_useful': rows_b / useful,
             'b_calls': len(first_calls), 'bit_equal': bool(equal), 'max_rel_diff': maxrel}
        results.append(r)
        lines.append('batch %3d: (a) %7.1f frames/s  (b) %7.1f frames/s  b/a %.3f | H2D (a) %.1f MB (b) %.1f MB | '
                     'computed/useful (a) %.3f (b) %.3f | %d call(s) | bit-equal %s (max |a - b| / max |a| %.1e)'
                     % (B, fa, fb, fb / fa, h2d_a / 1e6, h2d_b / 1e6, rows_a / useful, rows_b / useful, len(first_calls), equal,
                        maxrel))
    for r in results:
        lines.append(json.dumps(r))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
