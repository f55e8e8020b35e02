"""Device time of the t-SNE kernels of csrc/tsne.hip at the sizes a user runs: a small map (2 000 points), 10 000, 50 000
and the framewise US8K job (240 000).  Times are l3_tsne_time's: hipEvents around back-to-back rounds on a resident map, one untimed
round first.  Per size: the pair kernel alone, the repulsive pass (pair kernel, finish, Z), the attractive pass, the update and a
whole iteration; the calibration of the conditional probabilities (wall time of the operator, with its copies) and the host's
symmetrisation.

  pairs        n^2 pairs per pass; pairs/s from the pair kernel's time.  For four pairs (one staged point against a lane's four rows)
               the compiled loop holds 22 VALU instructions (the compiler packs two pairs into v_pk_* where it can) and 4 v_rcp_f32;
               a wave's VALU instruction holds its SIMD's issue for 4 cycles and a v_rcp_f32 for 8, so 64 x 4 pairs cost 22 * 4 + 4 * 8
               = 120 cycles of one SIMD: valu_share = pairs/s * (120 / 256) / (1024 SIMDs * 2.4e9 cycles/s)
  --torch      the same iteration in torch on the same GPU: the n x n pair terms in row chunks (float32), the attractive term by
               index_add_ over the entries of P, the update elementwise (torch's own events)

The map is a seeded Gaussian cloud and P a ring of 90 neighbours per point (the entry count of perplexity 20), which costs what a real
P costs.  One JSON line per (size, round).

    python scripts/tsne_throughput.py [--sizes 2000 10000 50000 240000] [--reps 3] [--rounds 2] [--torch]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIMD_CYCLES_PER_PAIR = 120.0 / 256.0
SIMD_CYCLES_PER_S = 1024 * 2.4e9


def ring(n, half=45):
    """a symmetric P: every point with its `half` successors and predecessors on a ring, equal weights"""
    off = np.r_[-np.arange(half, 0, -1), np.arange(1, half + 1)]
    cols = np.sort((np.arange(n)[:, None] + off[None, :]) % n, axis=1).astype(np.int32)
    indptr = np.arange(n + 1, dtype=np.int64) * (2 * half)
    return indptr, cols.reshape(-1), np.full(cols.size, 1.0 / cols.size, np.float32)


def torch_iteration(torch, y, u, gains, rows, cols, vals, chunk, lr):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    R, Z = torch.zeros_like(y), torch.zeros((), dtype=torch.float64, device=y.device)
    for lo in range(0, y.shape[0], chunk):
        d = y[lo:lo + chunk, None, :] - y[None, :, :]
        q = 1.0 / (1.0 + (d * d).sum(2))
        Z += q.sum(dtype=torch.float64) - q.shape[0]          # (the self terms are 1 each)
        R[lo:lo + chunk] = ((q * q)[:, :, None] * d).sum(1)
    d = y[rows] - y[cols]
    pq = vals / (1.0 + (d * d).sum(1))
    A = torch.zeros_like(y).index_add_(0, rows, pq[:, None] * d)
    g = 4.0 * (A - R / Z.to(y.dtype))
    inc = (u * g) < 0
    gains = torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01)
    u = 0.8 * u - lr * gains * g
    y = y + u
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), y, u, gains


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='+', type=int, default=[2000, 10000, 50000, 240000])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--torch', action='store_true')
    ap.add_argument('--chunk-pairs', type=int, default=1 << 27, help='pairs of one torch chunk')
    args = ap.parse_args()
    if args.torch:
        import torch          # before libl3hip: one HIP runtime in the process
    from l3embedding_amd import _lib, tsne
    for n in args.sizes:
        rng = np.random.default_rng(n)
        Y = (10.0 * rng.standard_normal((n, 2))).astype(np.float32)
        indptr, cols, vals = ring(n)
        k = 61
        dist = np.sort(rng.gamma(2.0, 3.0, size=(n, k)).astype(np.float32), axis=1)
        idx = ((np.arange(n)[:, None] + np.arange(1, k + 1)[None, :]) % n).astype(np.int32)
        _lib.op_tsne_conditional(dist[:256], 20.0)          # the library and the device are up
        t0 = time.perf_counter()
        p, _, _ = _lib.op_tsne_conditional(dist, 20.0)
        t1 = time.perf_counter()
        tsne.joint_affinities(idx, p)
        t2 = time.perf_counter()
        h = _lib.TSNE(n)
        h.set_affinities(indptr, cols, vals)
        h.set_embedding(Y)
        row_block, segments = _lib.tsne_geometry(n)
        if args.torch:
            ty = torch.from_numpy(Y).cuda()
            tu, tg = torch.zeros_like(ty), torch.ones_like(ty)
            trows = torch.from_numpy(np.repeat(np.arange(n), np.diff(indptr))).cuda()
            tcols, tvals = torch.from_numpy(cols.astype(np.int64)).cuda(), torch.from_numpy(vals).cuda()
            chunk = max(1, args.chunk_pairs // n)
            torch_iteration(torch, ty, tu, tg, trows, tcols, tvals, chunk, 1.0)          # warm-up
        for rnd in range(args.rounds):
            h.set_embedding(Y)
            t = {what: h.time(what, reps=args.reps) for what in ('pairs', 'repulsive', 'attractive', 'update', 'iteration')}
            rate = float(n) * n / (t['pairs'] * 1e-3)
            rec = dict(n=n, round=rnd, row_block=row_block, segments=segments, entries=int(indptr[-1]))
            rec.update({'%s_ms' % key: round(v, 4) for key, v in t.items()})
            rec.update(gpairs_per_s=round(rate * 1e-9, 1), valu_share=round(rate * SIMD_CYCLES_PER_PAIR / SIMD_CYCLES_PER_S, 3),
                       calibration_ms=round((t1 - t0) * 1e3, 2), symmetrisation_ms=round((t2 - t1) * 1e3, 2))
            if args.torch:
                tms, _, _, _ = torch_iteration(torch, ty, tu, tg, trows, tcols, tvals, chunk, 1.0)
                rec.update(torch_iteration_ms=round(tms, 3), torch_over_iteration=round(tms / t['iteration'], 2))
            print(json.dumps(rec), flush=True)
        h.close()
        if args.torch:
            del ty, tu, tg, trows, tcols, tvals
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
