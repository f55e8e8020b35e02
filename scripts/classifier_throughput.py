"""Seconds per epoch of the downstream MLP classifier (classifier/train.py:230-391) on a synthetic UrbanSound8K-shaped set:
200 k training rows and 28 k validation rows, C = 10, batch 64, at D = 512 and 6144.  The GPU epoch (l3_mlp_epoch: all steps +
the validation pass) against the same training step in torch on the CPU (16 threads), timed over --cpu-steps steps and scaled to
an epoch.  One JSON line per width.  Per-kernel times: run a short configuration under `rocprofv3 --kernel-trace --stats`.

    python scripts/classifier_throughput.py [--widths 512 6144] [--epochs 2] [--cpu-steps 200]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libl3hip: one HIP runtime)

from l3embedding_amd import _lib  # noqa: E402


def cpu_epoch_seconds(X, y, Xv, C, batch, steps, threads, lr=1e-4, wd=1e-5):
    torch.set_num_threads(threads)
    D = X.shape[1]
    net = torch.nn.Sequential(torch.nn.Linear(D, 512), torch.nn.ReLU(), torch.nn.Linear(512, 128), torch.nn.ReLU(),
                              torch.nn.Linear(128, C))
    opt = torch.optim.Adam(net.parameters(), lr=lr, eps=1e-8)
    xt, yt = torch.from_numpy(X), torch.from_numpy(y.astype(np.int64))
    kernels = [net[0].weight, net[2].weight, net[4].weight]

    def step(i):
        s = (i * batch) % (len(X) - batch)
        out = net(xt[s:s + batch])
        loss = torch.nn.functional.cross_entropy(out, yt[s:s + batch]) + wd * sum((k * k).sum() for k in kernels)
        opt.zero_grad()
        loss.backward()
        opt.step()
    for i in range(5):
        step(i)
    t = time.perf_counter()
    for i in range(steps):
        step(i)
    per_step = (time.perf_counter() - t) / steps
    with torch.no_grad():
        t = time.perf_counter()
        for s in range(0, len(Xv), 4096):
            net(torch.from_numpy(Xv[s:s + 4096]))
        val = time.perf_counter() - t
    return per_step, val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--widths', type=int, nargs='+', default=[512, 6144])
    ap.add_argument('--n-train', type=int, default=200000)
    ap.add_argument('--n-valid', type=int, default=28000)
    ap.add_argument('--classes', type=int, default=10)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--cpu-steps', type=int, default=200, help='0: no torch-CPU baseline')
    ap.add_argument('--threads', type=int, default=16)
    a = ap.parse_args()
    for D in a.widths:
        gen, rs = np.random.default_rng(D), np.random.RandomState(D)
        X = gen.standard_normal((a.n_train, D), dtype=np.float32)
        y = rs.randint(0, a.classes, a.n_train).astype(np.int32)
        Xv = gen.standard_normal((a.n_valid, D), dtype=np.float32)
        yv = rs.randint(0, a.classes, a.n_valid).astype(np.int32)
        m = _lib.MLP(D, a.classes, a.batch, weight_decay=1e-5, seed=0)
        t = time.perf_counter()
        m.set_data(X, y, Xv, yv)
        upload = time.perf_counter() - t
        steps = -(-a.n_train // a.batch)
        times, logs = [], None
        for e in range(a.epochs):
            perm = rs.permutation(a.n_train)
            t = time.perf_counter()
            logs = m.epoch(perm, 1e-4, e * steps)
            times.append(time.perf_counter() - t)
        m.close()
        rec = dict(D=D, C=a.classes, batch=a.batch, n_train=a.n_train, n_valid=a.n_valid, steps_per_epoch=steps,
                   upload_s=round(upload, 3), gpu_epoch_s=[round(x, 4) for x in times], gpu_step_us=round(1e6 * min(times) / steps, 2),
                   last_logs={k: round(v, 6) for k, v in logs.items()})
        if a.cpu_steps:
            per_step, val = cpu_epoch_seconds(X, y, Xv, a.classes, a.batch, a.cpu_steps, a.threads)
            cpu_epoch = per_step * steps + val
            rec.update(cpu_threads=a.threads, cpu_steps_timed=a.cpu_steps, cpu_step_ms=round(1e3 * per_step, 3),
                       cpu_val_s=round(val, 3), cpu_epoch_s=round(cpu_epoch, 2), speedup=round(cpu_epoch / min(times), 1))
        print(json.dumps(rec), flush=True)
        del X, Xv


if __name__ == '__main__':
    main()
