"""Throughput of vision embeddings from raw frames on one GPU: 256 uint8 frames of 360 x 640, cnn_L3_melspec2, engine batch 32,
pooling (7, 7), two ways, each in fresh processes that alternate:

  images  EmbeddingModel.predict_images on this tree: the bytes go to the device, csrc/frames.hip resizes (shorter side 256),
          crops (centre 224 x 224) and scales them there;
  host    what a user does without it: every frame resized on the host to 256 x 456 by torch's float64 antialiased bilinear
          interpolation (the arithmetic of tests/image_ref.py, vectorised), rounded half up to uint8, cropped, scaled to
          [-1, 1] in float32, and EmbeddingModel.predict on the rows.  --baseline-root names a checkout of another commit (the
          parent) whose library is built; the host processes then import that tree.  Without it they import this tree, whose
          predict is unchanged.

Each process: the model with seeded weights, one warm-up call, five timed calls around a host clock (the calls return host
arrays: device-synchronised).  Reported: seconds per call and frames/s, median [min, max] over all timed calls of a way; for
`host` also the share of the host-side resize; for `images` the frame kernel's own time from the engine's profiler (one further
call with profiling on: the frame kernel is the only kernel of a vision call in the front-end family) beside the towers'.

    python scripts/image_embedding_throughput.py [--baseline-root DIR] [--rounds 2] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W, BATCH, MT, POOL = 256, 360, 640, 32, 'cnn_L3_melspec2', (7, 7)
TIMED = 5


def child(way, root):
    import torch          # before libl3hip: one HIP runtime in the process
    import numpy as np
    sys.path.insert(0, root)
    from l3embedding_amd import model
    frames = np.random.RandomState(0).randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    m = model.L3Model(MT, seed=20180123)
    emb = model.EmbeddingModel(m, 'vision', POOL)
    e = m._ensure_engine(BATCH)
    prep = []

    def host_call():
        t0 = time.perf_counter()
        scaling = 256.0 / min(W, H)
        Wo, Ho = int(np.ceil(scaling * W)), int(np.ceil(scaling * H))
        y0, x0 = (Ho - 224) // 2, (Wo - 224) // 2
        x = np.empty((N, 224, 224, 3), np.float32)
        for i0 in range(0, N, BATCH):
            p = torch.from_numpy(frames[i0:i0 + BATCH]).permute(0, 3, 1, 2).to(torch.float64)
            v = torch.nn.functional.interpolate(p, size=(Ho, Wo), mode='bilinear', antialias=True, align_corners=False)
            v = v[:, :, y0:y0 + 224, x0:x0 + 224].permute(0, 2, 3, 1).numpy()
            u8 = np.clip(np.floor(v + 0.5), 0.0, 255.0).astype(np.uint8)
            x[i0:i0 + BATCH] = np.float32(2.0) * (u8.astype(np.float64) / 255.0).astype(np.float32) - np.float32(1.0)
        prep.append(time.perf_counter() - t0)
        return emb.predict(x, batch_size=BATCH)

    call = host_call if way == 'host' else lambda: emb.predict_images(frames, batch_size=BATCH)
    out = call()
    del prep[:]
    times = []
    for _ in range(TIMED):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    r = {'way': way, 's': times, 'host_prep_s': list(prep), 'sum': float(np.abs(out).sum(dtype=np.float64))}
    if way == 'images':
        e.profile_enable(True)
        call()
        prof = e.profile_read()
        e.profile_enable(False)
        r['frame_kernel_ms'] = prof['frontend']['ms']
        r['frame_kernel_launches'] = prof['frontend']['launches']
        r['kernels_ms'] = {k: v['ms'] for k, v in prof.items() if v['launches']}
    print(json.dumps(r), flush=True)


def stats(xs):
    xs = sorted(xs)
    n = len(xs)
    med = xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])
    return med, xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', default=None)
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--baseline-root', default=None, help='a built checkout of the commit the host way runs on (default: this tree)')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the report here')
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.root)
    roots = {'images': HERE, 'host': os.path.abspath(args.baseline_root) if args.baseline_root else HERE}
    runs = {'images': [], 'host': []}
    for _ in range(args.rounds):
        for way in ('images', 'host'):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', way, '--root', roots[way]],
                               stdout=subprocess.PIPE, timeout=600)
            if p.returncode != 0:
                raise SystemExit('the %s process ended with status %d' % (way, p.returncode))
            runs[way].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    lines = ['# %d frames of %d x %d x 3 uint8 -> 256 x 456 -> centre 224 x 224; %s, engine batch %d, pooling %s; %d fresh processes '
             'per way, alternating, 1 warm-up + %d timed calls each' % (N, H, W, MT, BATCH, POOL, args.rounds, TIMED)]
    for way in ('images', 'host'):
        med, lo, hi = stats([t for r in runs[way] for t in r['s']])
        lines.append('%-6s (%s): %.4f s per call [%.4f, %.4f]  %.0f frames/s [%.0f, %.0f]'
                     % (way, 'the --baseline-root tree' if roots[way] != HERE else 'this tree', med, lo, hi, N / med, N / hi, N / lo))
        if way == 'host':
            pm, plo, phi = stats([t for r in runs[way] for t in r['host_prep_s']])
            lines.append('       of which the host-side resize, crop and scaling: %.4f s [%.4f, %.4f]' % (pm, plo, phi))
        else:
            km, klo, khi = stats([r['frame_kernel_ms'] for r in runs[way]])
            tm = stats([sum(r['kernels_ms'].values()) for r in runs[way]])[0]
            lines.append('       frame kernel (profiled call, %d launches): %.3f ms [%.3f, %.3f] of %.1f ms of kernels, %.2f %% of the call'
                         % (runs[way][0]['frame_kernel_launches'], km, klo, khi, tm, 100.0 * km / (1000.0 * med)))
    a = stats([t for r in runs['images'] for t in r['s']])[0]
    b = stats([t for r in runs['host'] for t in r['s']])[0]
    lines.append('host / images: %.2f' % (b / a))
    for way in ('images', 'host'):
        for r in runs[way]:
            lines.append(json.dumps(r))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
