"""The library's own data-parallel step (l3_comm_init -> l3_step_dp -> l3_step_results_enqueue(reduce=1), the default path of
cli_train --gpus N and bench.py --comm native) across real processes that hold DIFFERENT shards, on one GPU.

Every rank is a process of tests/dp_native_worker.py; libl3hip binds the collective double tests/fake_rccl/libfake_rccl.so in its
inter-process mode (FAKE_RCCL_IPC_DIR): its all-reduce adds the ranks' buffers in rank order in their own precision, its
all-gather puts rank r's data in slot r.  The reference is the in-process emulation of test_dp_world2_one_gpu_gloo: one engine per
shard, forward and every backward bucket, the gradient arenas summed in rank order, the packed BatchNorm batch statistics
concatenated rank-major into bn_stats_replicas(world), step_update.  It does the same additions in the same order, so the native
run must equal it bit for bit; the float64 oracle (oracle.dp_train_step) then anchors the whole step.  Controls computed here show
that the comparison sees the rank order of the statistics, the assignment of shards to ranks and a collective that does not
combine the ranks' data."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dp_native_worker import DATA_SEED, SEED, live_head
from l3embedding_amd import _lib
from oracle import l3_oracle as o

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = os.path.join(HERE, 'fake_rccl', 'libfake_rccl.so')
WORKER = os.path.join(HERE, 'dp_native_worker.py')


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def _env(**kw):
    assert os.path.exists(FAKE), 'tests/fake_rccl/libfake_rccl.so missing: __graft_entry__.build() makes it'
    env = dict(os.environ, L3_RCCL_LIB=FAKE)
    for k in [k for k in env if k.startswith('FAKE_RCCL_')] + ['L3_DP_FAULT', 'L3_DP_ARENA_ORDER']:
        env.pop(k, None)
    env.update(kw)
    return env


def _run_ranks(tmp_path, mt, GB, world, steps, lr, port):
    ipc = tmp_path / 'ipc'
    ipc.mkdir()
    env = _env(FAKE_RCCL_IPC_DIR=str(ipc), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, WORKER, 'train', str(tmp_path), mt, str(GB), str(steps), repr(lr)],
                              env=dict(env, RANK=str(r))) for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=600) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert os.listdir(str(ipc)) == []            # rank 0's ncclCommDestroy removed the communicator's file
    return [dict(np.load(os.path.join(str(tmp_path), 'rank%d.npz' % r))) for r in range(world)]


def _emulate(mt, GB, world, steps, lr, reverse_stats=False, swap01=False):
    """The data-parallel step by hand, in-process (test_dp_world2_one_gpu_gloo's emulation).  reverse_stats: the replicas'
    statistics applied in reverse rank order; swap01: engine 0 holds rank 1's shard and engine 1 rank 0's."""
    import torch
    from l3embedding_amd.training_utils import _DevArray, get_slice_bounds
    v, a, l = o.synthetic_batch(GB, seed=DATA_SEED)
    engs, flats, sizes = [], [], []
    for r in range(world):
        lo, hi = get_slice_bounds(GB, world, 1 - r if swap01 and r < 2 else r)
        e = _lib.Engine(mt, hi - lo, seed=SEED, global_batch=GB)
        live_head(e)
        e.upload_batch(v[lo:hi], a[lo:hi], l[lo:hi])
        ptr, n = e.grad_arena()
        engs.append(e)
        flats.append(torch.as_tensor(_DevArray(ptr, n), device='cuda:0'))
        sizes.append(hi - lo)
    losses, accs = [], []
    for _ in range(steps):
        for e in engs:
            e.step_forward(True)
            for b in range(1, e.bucket_count()):
                e.step_backward_bucket(b)
            e.sync()
        own = [f.cpu().numpy() for f in flats]
        total = flats[0] + flats[1]                  # rank order: ((f0 + f1) + f2) + ...
        for f in flats[2:]:
            total = total + f
        for f in flats:
            f.copy_(total)
        packed = []
        for e in engs:
            ptr, n = e.bn_stats_pack()
            e.sync()
            packed.append(torch.as_tensor(_DevArray(ptr, n), device='cuda:0').clone())
        gathered = torch.cat(packed[::-1] if reverse_stats else packed)
        for e in engs:
            torch.as_tensor(_DevArray(e.bn_stats_replicas(world), gathered.numel()), device='cuda:0').copy_(gathered)
        torch.cuda.synchronize()
        for e in engs:
            e.step_update(lr, 1.0)
            e.sync()
        res = [e.step_results() for e in engs]
        losses.append(sum(n * r[0] for n, r in zip(sizes, res)) / GB)
        accs.append(sum(n * r[1] for n, r in zip(sizes, res)) / GB)
    Ws = [e.get_params() for e in engs]
    assert all(np.array_equal(W[k], Ws[0][k]) for W in Ws[1:] for k in W)
    out = dict(params=Ws[0], arena=flats[0].cpu().numpy(), own=own, losses=losses, accs=accs, steps=engs[0].optimizer_steps())
    for e in engs:
        e.close()
    return out


def _check_native(z, em, world, steps):
    """Every rank: the same bits as every other rank and as the emulation.  Returns the parameter names."""
    names = [k for k in z[0] if k.startswith('p:')]
    assert any('moving_mean' in k for k in names) and any('moving_variance' in k for k in names)
    for r in range(1, world):
        diff = [k for k in z[0] if not np.array_equal(z[r][k], z[0][k]) and k != 'shard']
        assert diff == [], (r, diff)           # parameters, moving statistics, reduced arena, losses, accuracies, counters
    diff = [k for k in names if not np.array_equal(z[0][k], em['params'][k[2:]])]
    assert diff == [], diff
    assert np.array_equal(z[0]['arena'], em['arena'])
    live = np.count_nonzero(z[0]['arena']) / z[0]['arena'].size
    for got, want in ((z[0]['losses'], em['losses']), (z[0]['accs'], em['accs'])):
        assert len(got) == steps
        assert np.all(np.abs(got - np.asarray(want)) <= 1e-6 * np.maximum(1.0, np.abs(want))), (got, want)
    assert z[0]['optimizer_steps'].tolist() == [steps, world * steps] == list(em['steps'])
    print('non-zero share of the reduced gradient arena after the last step: %.3f' % live)
    assert live > 0.5                          # an exchange of zeros would check nothing
    s = sum(range(world))
    assert z[0]['host_sum'].tolist() == [s, -s, world * 2.0 ** 40 + s]
    assert z[0]['host_max'].tolist() == [world - 1, 0.0, 2.0 ** 40 + world - 1]
    return names


def _controls(z, em, names, mt, GB, world, steps, lr):
    """Each of these faults must change bits the native comparison covers.  Returns the sizes of the differences."""
    moving = [k for k in names if 'moving_' in k]
    rev = _emulate(mt, GB, world, steps, lr, reverse_stats=True)
    d_rev = max(relerr(z[0][k], rev['params'][k[2:]]) for k in moving)
    swap = _emulate(mt, GB, world, steps, lr, swap01=True)
    d_swap = max(relerr(z[0][k], swap['params'][k[2:]]) for k in names)
    # what the in-process double computes: every rank holds this rank's data, the sum is world x this rank's arena
    d_own = min(relerr(z[0]['arena'], np.float32(world) * g) for g in em['own'])
    assert d_rev > 0 and d_swap > 0 and d_own > 0, (d_rev, d_swap, d_own)
    return d_rev, d_swap, d_own


def _oracle(mt, GB, world, steps, lr):
    P = o.init_params(mt, seed=SEED)
    e0 = _lib.Engine(mt, 2, seed=SEED)
    live_head(e0)
    P.update(e0.get_params())                        # the engine's own initial weights
    e0.close()
    v, a, l = o.synthetic_batch(GB, seed=DATA_SEED)
    adam, bn = o.AdamState(), o.BNMovingState(zero_debias=True)
    losses = [o.dp_train_step(mt, P, adam, bn, v, a, l, lr, world)['loss'] for _ in range(steps)]
    return P, losses


def _report(tag, z, oracle_losses, d_stats, d_ctl):
    print('\n%s: shards %s, reduced losses %s (oracle %s), accuracies %s' % (
        tag, [zz['shard'].tolist() for zz in z], ['%.6f' % x for x in z[0]['losses']], ['%.6f' % x for x in oracle_losses],
        z[0]['accs'].tolist()))
    print('  %-52s %s' % ('oracle distance of the moving statistics', '  '.join('%s %.1e' % kv for kv in d_stats.items())))
    print('  %-52s %.1e' % ('worst loss distance to the oracle / max(1, |loss|)',
                            max(abs(g - w) / max(1.0, abs(w)) for g, w in zip(z[0]['losses'], oracle_losses))))
    print('  %-52s %.1e' % ('control: statistics in reverse rank order', d_ctl[0]))
    print('  %-52s %.1e' % ('control: shards of ranks 0 and 1 swapped', d_ctl[1]))
    print('  %-52s %.1e' % ('control: arena = world x one rank\'s own (closest rank)', d_ctl[2]))


def test_native_dp_world2_uneven_shards(gpu_required, tmp_path):
    """cnn_L3_melspec2, two ranks, global batch 7 (shards 3 and 4: the last rank takes the remainder), two steps at lr 1e-3,
    default dp_moving='replicas', tower overlap on (the alternated bucket order, decided by each process and compared at
    l3_comm_init).  Bounds against the oracle: those of test_dp_world2_one_gpu_gloo (moving variances) and of the goldens (loss);
    weight-level oracle bounds at this batch are Adam sign noise and are left to the bit-exact emulation."""
    mt, GB, world, steps, lr = 'cnn_L3_melspec2', 7, 2, 2, 1e-3
    z = _run_ranks(tmp_path, mt, GB, world, steps, lr, port=29547)
    assert [zz['shard'].tolist() for zz in z] == [[0, 3], [3, 7]]
    em = _emulate(mt, GB, world, steps, lr)
    names = _check_native(z, em, world, steps)
    d_ctl = _controls(z, em, names, mt, GB, world, steps, lr)
    P, oracle_losses = _oracle(mt, GB, world, steps, lr)
    d_var = max(relerr(z[0][k], P[k[2:]]) for k in names if 'moving_variance' in k)
    _report('cnn_L3_melspec2 world 2', z, oracle_losses, {'variances': d_var}, d_ctl)
    assert d_var < 2e-3
    for got, want in zip(z[0]['losses'], oracle_losses):
        assert abs(got - want) < 1e-3 * max(1.0, abs(want)), (got, want)


def test_native_dp_world3_uneven_shards(gpu_required, tmp_path):
    """tiny_L3, three ranks, global batch 8 (shards 2, 2, 4), three steps at lr 0 (frozen weights: the BatchNorm moving statistics
    then depend on the data alone -- test_dp_moving_statistics_take_one_update_per_replica), the same bit-exact checks, every moving
    statistic within 2e-5 of the oracle's three virtual replicas, and the host all-reduce of values that differ between the ranks."""
    mt, GB, world, steps, lr = 'tiny_L3', 8, 3, 3, 0.0
    z = _run_ranks(tmp_path, mt, GB, world, steps, lr, port=29548)
    assert [zz['shard'].tolist() for zz in z] == [[0, 2], [2, 4], [4, 8]]
    em = _emulate(mt, GB, world, steps, lr)
    names = _check_native(z, em, world, steps)
    d_ctl = _controls(z, em, names, mt, GB, world, steps, lr)
    P, oracle_losses = _oracle(mt, GB, world, steps, lr)
    d_mean = max(relerr(z[0][k], P[k[2:]]) for k in names if 'moving_mean' in k)
    d_var = max(relerr(z[0][k], P[k[2:]]) for k in names if 'moving_variance' in k)
    _report('tiny_L3 world 3', z, oracle_losses, {'means': d_mean, 'variances': d_var}, d_ctl)
    assert d_mean < 2e-5 and d_var < 2e-5, (d_mean, d_var)
    for got, want in zip(z[0]['losses'], oracle_losses):
        assert abs(got - want) < 1e-3 * max(1.0, abs(want)), (got, want)


def _orphan(world, **env):
    r = subprocess.run([sys.executable, WORKER, 'orphan', str(world)], env=_env(**env), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    text = r.stdout.decode(errors='replace')
    assert r.returncode == 0, text[-3000:]
    return json.loads([ln for ln in text.splitlines() if ln.startswith('RESULT ')][-1][7:])


def _check_orphan(res):
    assert res['world_after'] == 0, res                                   # no communicator left behind
    assert res['step_dp_error'] is not None and 'before l3_comm_init' in res['step_dp_error'], res
    assert res['retry_error'] is None, res                                # a second l3_comm_init succeeds
    assert 'fake_rccl' in res['library'] and res['world_retry'] == 1, res
    assert res['results_equal'] and res['param_mismatch'] == [] and res['n_tensors'] > 10, res


def test_comm_init_cleans_up_after_a_failed_collective(gpu_required):
    """The agreement all-reduce inside l3_comm_init (the first collective of the process: FAKE_RCCL_FAIL_AT=1) fails: l3_comm_init
    raises and leaves no communicator -- a half-built one used to stay, a retry answered "already initialised" and l3_step_dp ran on
    it -- and a second l3_comm_init at world 1 gives a step equal to l3_step_resident bit for bit."""
    res = _orphan(1, FAKE_RCCL_FAIL_AT='1', FAKE_RCCL_DELAY_US='0')
    assert res['error'] is not None and 'ncclAllReduce' in res['error'], res
    _check_orphan(res)
    assert res['collectives'] >= 2, res            # the retry's agreement all-reduce and the step's buckets ran


def test_comm_init_fails_when_a_peer_never_arrives(gpu_required, tmp_path):
    """World 2 with only rank 0 started: ncclCommInitRank gives up after FAKE_RCCL_IPC_TIMEOUT_S (5 s) instead of hanging,
    l3_comm_init fails and leaves no communicator, and the engine can still join a communicator of one rank."""
    ipc = tmp_path / 'ipc'
    ipc.mkdir()
    res = _orphan(2, FAKE_RCCL_IPC_DIR=str(ipc), FAKE_RCCL_IPC_TIMEOUT_S='5')
    assert res['error'] is not None and 'ncclCommInitRank' in res['error'], res
    assert 4.0 < res['init_s'] < 60.0, res
    _check_orphan(res)
    assert os.listdir(str(ipc)) == []


def test_bn_stats_replicas_refuses_without_a_packed_training_forward(gpu_required):
    """l3_bn_stats_replicas_dev arms `world` moving-average updates for the next l3_step_update: it must refuse (and arm nothing)
    unless a training forward is current and l3_bn_stats_pack_dev ran behind it -- else the update would apply
    `world` replicas of whatever the gathered buffer held."""
    import torch
    from l3embedding_amd.training_utils import _DevArray
    mt, B = 'tiny_L3', 2
    v, a, l = o.synthetic_batch(B, seed=71)
    e = _lib.Engine(mt, B, seed=5)
    with pytest.raises(_lib.L3Error, match='no packed training forward'):
        e.bn_stats_replicas(2)                        # fresh engine: no forward at all
    e.train_step(v, a, l, 1e-3)
    assert e.optimizer_steps() == (1, 1)              # one ordinary step: one moving-average update
    e.upload_batch(v, a, l)

    def forward_backward():
        e.step_forward(True)
        for b in range(1, e.bucket_count()):
            e.step_backward_bucket(b)
    forward_backward()
    with pytest.raises(_lib.L3Error, match='no packed training forward'):
        e.bn_stats_replicas(2)                        # a training forward whose statistics were not packed
    e.step_update(1e-3)
    assert e.optimizer_steps() == (2, 2)              # still exactly one update
    # packed behind the current forward: armed, two replica updates
    forward_backward()
    ptr, n = e.bn_stats_pack()
    e.sync()
    mine = torch.as_tensor(_DevArray(ptr, n), device='cuda:0').clone()
    torch.as_tensor(_DevArray(e.bn_stats_replicas(2), 2 * n), device='cuda:0').copy_(torch.cat([mine, mine]))
    torch.cuda.synchronize()
    e.step_update(1e-3)
    assert e.optimizer_steps() == (3, 4)
    e.close()
