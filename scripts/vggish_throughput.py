"""Throughput of the VGGish feature path (profiles/r12_vggish.txt): 64 four-second clips at 44.1 kHz, hop 0.1, seeded He-normal
weights.  `time`: examples/s and files/s of VGGishModel.predict_clips per convolution algorithm (wall clock around calls that end in
the library's host wait), the distance between the algorithms' embeddings, and the torch-CPU network at 16 threads as the
comparison.  `trace <algo>`: a few calls, to run under `rocprofv3 --kernel-trace --stats`."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import vggish_ref as ref
from l3embedding_amd import vggish

mode = sys.argv[1]
rng = np.random.RandomState(0)
clips = [(0.3 * rng.standard_normal(4 * 44100)).astype(np.float32) for _ in range(64)]
rates = [44100] * 64
w = ref.he_weights(3)
pca, means = np.eye(128, dtype=np.float32), np.zeros(128, np.float32)
algos = ['f4x4', 'f2x2', 'direct'] if mode == 'time' else [sys.argv[2]]
outs = {}
for algo in algos:
    m = vggish.VGGishModel(weights=w, pca_matrix=pca, pca_means=means, conv=algo)
    out = m.predict_clips(clips, rates, hop_size=0.1)            # warm-up of every shape
    n_ex = sum(o.shape[0] for o in out)
    outs[algo] = np.concatenate(m.predict_clips(clips, rates, hop_size=0.1, postprocess=False))
    reps = 5 if mode == 'time' else 2
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.predict_clips(clips, rates, hop_size=0.1)               # returns after the device-to-host copy and the host wait
        ts.append(time.perf_counter() - t0)
    print('%s: batch %d, %d examples of 64 files per call; calls %s s -> best %.0f examples/s, %.1f files/s (median %.0f examples/s)'
          % (algo, m.net.batch, n_ex, ' '.join('%.4f' % t for t in ts), n_ex / min(ts), 64 / min(ts), n_ex / float(np.median(ts))), flush=True)
    m.close()
if mode == 'time':
    for a in ('f4x4', 'f2x2'):
        print('raw embedding %s vs direct: max abs difference %.3e (|emb| max %.2f)' % (a, np.abs(outs[a] - outs['direct']).max(), np.abs(outs['direct']).max()))
    torch.set_num_threads(16)
    ex = np.random.RandomState(1).standard_normal((256, 96, 64)).astype(np.float32)
    ref.network_torch32(ex[:32], w)
    t0 = time.perf_counter()
    ref.network_torch32(ex, w)
    dt = time.perf_counter() - t0
    print('torch-CPU network alone (16 threads, 256 examples, no resampling / log-mel / postprocessing): %.3f s -> %.0f examples/s' % (dt, 256 / dt))
