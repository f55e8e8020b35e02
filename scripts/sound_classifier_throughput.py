"""Time of classifying audio clips end to end on one GPU, two ways (profiles/r27_sound_classifier.txt):

  pieces    what a user assembles without sound.SoundClassifier: EmbeddingModel.predict_clips to the host, MinMaxScaler.transform and
            StandardScaler.transform in NumPy, MLPModel.predict on the host rows, NumPy's per-file mean and arg-max;
  resident  SoundClassifier.predict_clips: the pooled rows stay on the GPU, the transforms and the per-file reduction run there.

Workload: 64 clips of 4 s at 44.1 kHz (resampled on the GPU), cnn_L3_melspec2 with seeded weights, 'original' pooling (D = 6144),
hop 0.1 s (1984 frames), a seeded MLP of 10 classes, engine batch 32.  Each way is split into the embedding (up to the rows being
on the host / in the device matrix, device-synchronised either way) and the tail after it; a host clock around each.

One process times one way: --mode pieces|resident [--tree DIR] (DIR: the source tree to import, so that `pieces` can run on another
checkout, e.g. the parent commit) -> one JSON line.  The driver alternates the two in fresh processes and writes the record:

    python scripts/sound_classifier_throughput.py --alternate PARENT_TREE [--rounds 4] [--reps 5] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MT, HOP, BATCH, CLASSES = 'cnn_L3_melspec2', 4800, 32, 10


def make_clips(n_clips=64, seconds=4, rate=44100, seed=0):
    r = np.random.RandomState(seed)
    return [(0.1 * r.randn(seconds * rate)).astype(np.float32) for _ in range(n_clips)], [rate] * n_clips


def run_one(mode, tree, reps, warmup):
    sys.path.insert(0, tree)
    from l3embedding_amd import classifier, model, usc
    clips, rates = make_clips()
    m = model.L3Model(MT, seed=20180123)
    m._ensure_engine(BATCH)
    emb = model.EmbeddingModel(m, 'audio', model.AUDIO_POOLING[MT]['original'])
    D = 6144
    r = np.random.RandomState(1)
    mm = usc.MinMaxScaler().fit(r.rand(64, D).astype(np.float32))
    std = usc.StandardScaler().fit(r.rand(64, D).astype(np.float32))
    mlp = classifier.MLPModel(D, num_classes=CLASSES, seed=3)
    mlp.predict(np.zeros((1, D), np.float32))          # the handle and its weights
    if mode == 'resident':
        from l3embedding_amd import sound
        sc = sound.SoundClassifier(emb, mlp, std, min_max_scaler=mm, hop_size=HOP / 48000.0)
    t_embed, t_tail, proba = [], [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        if mode == 'resident':
            X, file_idxs = emb.predict_clips(clips, HOP, rates=rates, to_device=True)
            t1 = time.perf_counter()
            got = sc._score(X, file_idxs)
            proba, pred = got['file_proba'], got['file_predict']
            X.close()
        else:
            rows = emb.predict_clips(clips, HOP, rates=rates)
            file_idxs = usc._row_ranges([len(x) for x in rows])
            X = np.concatenate(rows)
            t1 = time.perf_counter()
            probs = mlp.predict(std.transform(mm.transform(X)))
            proba = np.stack([probs[s:e].mean(axis=0) for s, e in file_idxs])
            pred = classifier._file_predictions(probs, file_idxs)
        t2 = time.perf_counter()
        if i >= warmup:
            t_embed.append(t1 - t0)
            t_tail.append(t2 - t1)
    frames = int(file_idxs[-1][1])
    print(json.dumps(dict(mode=mode, frames=frames, embed_s=t_embed, tail_s=t_tail,
                          sha=hashlib.sha256(np.ascontiguousarray(proba).tobytes() + np.asarray(pred, np.int64).tobytes()).hexdigest())))


def _stats(v):
    v = np.sort(np.asarray(v))
    return float(np.median(v)), float(v[0]), float(v[-1])


def alternate(parent, rounds, reps, warmup, out):
    runs = {'pieces': [], 'resident': []}
    for _ in range(rounds):
        for mode, tree in (('pieces', os.path.abspath(parent)), ('resident', HERE)):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), '--mode', mode, '--tree', tree, '--reps', str(reps),
                                  '--warmup', str(warmup)], cwd=tree, stdout=subprocess.PIPE, timeout=600, check=True)
            runs[mode].append(json.loads(res.stdout.decode().strip().splitlines()[-1]))
    frames = runs['resident'][0]['frames']
    lines = ['# 64 clips of 4 s at 44.1 kHz, %s original pooling (D = 6144), hop %d, %d frames, MLP of %d classes, engine batch %d'
             % (MT, HOP, frames, CLASSES, BATCH),
             '# pieces: predict_clips to the host + NumPy transforms + MLPModel.predict + NumPy per-file mean, run on the tree %s' % parent,
             '# resident: SoundClassifier.predict_clips on this tree.  %d alternating fresh processes each, %d warm-up + %d timed calls '
             'per process; median [min, max] over all timed calls, seconds' % (rounds, warmup, reps)]
    med = {}
    for mode in ('pieces', 'resident'):
        e = [t for r in runs[mode] for t in r['embed_s']]
        t = [t for r in runs[mode] for t in r['tail_s']]
        tot = [a + b for a, b in zip(e, t)]
        med[mode] = _stats(tot)
        lines.append('%-8s embedding %.4f [%.4f, %.4f]  tail %.4f [%.4f, %.4f]  total %.4f [%.4f, %.4f]'
                     % ((mode,) + _stats(e) + _stats(t) + _stats(tot)))
    shas = {r['sha'] for rs in runs.values() for r in rs}
    lines.append('results bit-equal between the two ways and across processes: %s' % (len(shas) == 1))
    lines.append('resident / pieces, medians of the totals: %.4f; the ranges %s' % (
        med['resident'][0] / med['pieces'][0],
        'overlap' if med['resident'][1] <= med['pieces'][2] and med['pieces'][1] <= med['resident'][2] else 'do not overlap'))
    for mode in ('pieces', 'resident'):
        for r in runs[mode]:
            lines.append(json.dumps(r))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if out:
        with open(out, 'w') as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['pieces', 'resident'])
    ap.add_argument('--tree', default=HERE)
    ap.add_argument('--alternate', default=None, metavar='PARENT_TREE')
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.alternate:
        alternate(args.alternate, args.rounds, args.reps, args.warmup, args.out)
    elif args.mode:
        run_one(args.mode, args.tree, args.reps, args.warmup)
    else:
        ap.error('--mode or --alternate')


if __name__ == '__main__':
    main()
