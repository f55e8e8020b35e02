"""Seconds per epoch of the downstream MLP classifier (classifier/train.py:230-391) on a synthetic UrbanSound8K-shaped set:
200 k training rows and 28 k validation rows, C = 10, batch 64, at D = 512 and 6144.  The GPU epoch (l3_mlp_epoch: all steps +
the validation pass) against the same training step in torch on the CPU (16 threads), timed over --cpu-steps steps and scaled to
an epoch.  One JSON line per width.  Per-kernel times: run a short configuration under `rocprofv3 --kernel-trace --stats`.

--group N (record profiles/r24_mlp_group.txt) times instead, per width and alternating --reps times after a warm-up
of each: one epoch of an N-member group (l3_mlp_group_epoch, members with the rates and weight decays of the reference's grid)
and N epochs of the single model one after the other, which is what the loop over the grid runs.  --search-epochs E adds the whole
search on the same set as one fold (the validation rows as the validation fold and, in files of 28 frames, as the test fold):
classifier.train_mlp_search against train_param_search(train_func=train_mlp), E epochs per point with patience E, the results
compared for equality.  On a checkout without the group handle only the single model and the loop are timed, so the same file
measures an earlier commit.

    python scripts/classifier_throughput.py [--widths 512 6144] [--epochs 2] [--cpu-steps 200]
    python scripts/classifier_throughput.py --group 9 --reps 3 --search-epochs 10 --cpu-steps 0
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


GRID = [(lr, wd) for lr in (1e-5, 1e-4, 1e-3) for wd in (1e-5, 1e-4, 1e-3)]          # classifier/train.py:638-651


def group_against_singles(a, D, X, y, Xv, yv, rs):
    """--group: one group epoch against a.group single-model epochs -> the fields of the width's JSON line"""
    steps = -(-a.n_train // a.batch)
    points = [GRID[i % len(GRID)] for i in range(a.group)]
    single = _lib.MLP(D, a.classes, a.batch, weight_decay=points[0][1], seed=0)
    single.set_data(X, y, Xv, yv)
    group = None
    if hasattr(_lib, 'MLPGroup'):
        group = _lib.MLPGroup(D, a.classes, a.batch, [wd for _, wd in points], [0] * a.group)
        group.set_data(X, y, Xv, yv)
    group_s, singles_s, epoch = [], [], 0
    for rep in range(a.reps + 1):          # rep 0 warms up both
        perm = rs.permutation(a.n_train)
        if group is not None:
            t = time.perf_counter()
            group.epoch(perm, [lr for lr, _ in points], epoch * steps)
            group_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        for k in range(1 if rep == 0 else a.group):
            single.epoch(perm, points[k][0], (epoch + k) * steps)
        singles_s.append(time.perf_counter() - t)
        epoch += a.group
    single.close()
    rec = dict(members=a.group, singles_epochs_s=[round(x, 4) for x in singles_s[1:]],
               single_step_us=round(1e6 * min(singles_s[1:]) / (a.group * steps), 2))
    if group is not None:
        group.close()
        rec.update(group_epoch_s=[round(x, 4) for x in group_s[1:]], group_step_us=round(1e6 * min(group_s[1:]) / steps, 2),
                   singles_over_group=round(min(singles_s[1:]) / min(group_s[1:]), 2))
    return rec


def search_against_loop(a, X, y, Xv, yv):
    """--search-epochs: the whole nine-point search as one group and as the loop -> the fields of a JSON line"""
    import shutil
    import tempfile
    from l3embedding_amd import classifier
    frames = 28
    files = len(Xv) // frames
    train, valid = {'features': X, 'labels': y}, {'features': Xv, 'labels': yv}
    test = {'features': Xv[:files * frames], 'labels': yv[:files * frames:frames],
            'file_idxs': [(i * frames, (i + 1) * frames) for i in range(files)]}
    args = dict(batch_size=a.batch, num_epochs=a.search_epochs, patience=a.search_epochs, num_classes=a.classes, random_state=1,
                train_with_valid=False)
    grid = {'learning_rate': [1e-5, 1e-4, 1e-3], 'weight_decay': [1e-5, 1e-4, 1e-3]}
    routes = {'loop': lambda d: classifier.train_param_search(train, valid, test, d, train_func=classifier.train_mlp,
                                                              search_space=grid, **args)}
    if hasattr(classifier, 'train_mlp_search'):
        routes['group'] = lambda d: classifier.train_mlp_search(train, valid, test, d, search_space=grid, **args)
    wall, outcome = {}, {}
    for rep in range(a.reps):
        for name, run in routes.items():
            d = tempfile.mkdtemp(prefix='mlp_search_')
            try:
                t = time.perf_counter()
                outcome[name] = run(d)
                wall.setdefault(name, []).append(round(time.perf_counter() - t, 3))
            finally:
                shutil.rmtree(d, ignore_errors=True)
    rec = dict(part='search', epochs_per_point=a.search_epochs, points=9, wall_s=wall,
               chosen=list(outcome['loop'][1]['search_params_best_values']))
    if 'group' in outcome:
        same = all(np.array_equal(g, w) for g, w in zip(outcome['group'][0].get_weights(), outcome['loop'][0].get_weights()))
        same = same and all(outcome['group'][k]['search'][p]['loss_history'] == outcome['loop'][k]['search'][p]['loss_history']
                            for k in (1, 2) for p in outcome['loop'][k]['search'])
        rec.update(equal_weights_and_histories=bool(same), loop_over_group=round(min(wall['loop']) / min(wall['group']), 2))
    return rec


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
    ap.add_argument('--group', type=int, default=0, help='N > 0: an N-member group epoch against N single-model epochs')
    ap.add_argument('--reps', type=int, default=3, help='--group / --search-epochs: timed repetitions, alternating')
    ap.add_argument('--search-epochs', type=int, default=0, help='E > 0: the whole search, E epochs per point, group against loop')
    a = ap.parse_args()
    for D in a.widths:
        gen, rs = np.random.default_rng(D), np.random.RandomState(D)
        X = gen.standard_normal((a.n_train, D), dtype=np.float32)
        y = rs.randint(0, a.classes, a.n_train).astype(np.int32)
        Xv = gen.standard_normal((a.n_valid, D), dtype=np.float32)
        yv = rs.randint(0, a.classes, a.n_valid).astype(np.int32)
        if a.group or a.search_epochs:
            rec = dict(D=D, C=a.classes, batch=a.batch, n_train=a.n_train, n_valid=a.n_valid, steps_per_epoch=-(-a.n_train // a.batch))
            if a.group:
                print(json.dumps(dict(rec, **group_against_singles(a, D, X, y, Xv, yv, rs))), flush=True)
            if a.search_epochs:
                print(json.dumps(dict(rec, **search_against_loop(a, X, y, Xv, yv))), flush=True)
            del X, Xv
            continue
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
