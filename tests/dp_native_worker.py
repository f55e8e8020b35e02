"""Worker of tests/test_dp_native_gpu.py: ranks of the library's own data-parallel step (l3_comm_init -> l3_step_dp ->
l3_step_results_enqueue(reduce=1)) in separate processes that hold different shards, all on GPU 0.  libl3hip binds the
collective double tests/fake_rccl/libfake_rccl.so (L3_RCCL_LIB) in its inter-process mode (FAKE_RCCL_IPC_DIR): its
all-reduce and all-gather really combine what the ranks hold, in rank order.

  train <out_dir> <model> <global_batch> <steps> <lr>   one rank (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT); gloo carries
                                                        the unique id and the final barrier only -> <out_dir>/rank<r>.npz
  orphan <world>                                        l3_comm_init that fails (FAKE_RCCL_FAIL_AT, or a peer that never
                                                        arrives), then what the engine is left with -> RESULT <json>
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

SEED, DATA_SEED = 13, 31        # engine initialisation / synthetic batch: the test's emulation uses the same


def live_head(eng):
    """dense_2/kernel x 1/64 (bench.py live_head): with the untouched head every synthetic sample lies outside the probability clip
    of the loss, and every gradient would be zero -- a gradient exchange of zeros checks nothing."""
    shape = dict((n, s) for n, s, _ in eng.param_table())['dense_2/kernel']
    eng.set_param('dense_2/kernel', eng.get_param('dense_2/kernel', shape) * np.float32(1.0 / 64))


def train(out_dir, mt, GB, steps, lr):
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    import torch                # before libl3hip: one HIP runtime in the process (_lib.require_single_hip_runtime)
    import torch.distributed as dist
    from l3embedding_amd import _lib
    from l3embedding_amd.training_utils import NativeDataParallelTrainer, _DevArray, get_slice_bounds
    from oracle import l3_oracle as o
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    v, a, l = o.synthetic_batch(GB, seed=DATA_SEED)
    lo, hi = get_slice_bounds(GB, world, rank)
    eng = _lib.Engine(mt, hi - lo, seed=SEED, global_batch=GB)
    live_head(eng)
    tr = NativeDataParallelTrainer(eng, world, rank)        # the unique id travels through share_unique_id (gloo broadcast)
    info = eng.comm_info()
    assert 'fake_rccl' in info['library'] and info['world'] == world and info['rank'] == rank, info
    eng.upload_batch(v[lo:hi], a[lo:hi], l[lo:hi])
    res = []
    for k in range(steps):
        tr.step(lr)
        eng.results_enqueue(k & 1, reduce=True)
        if k:
            res.append(eng.results_wait((k - 1) & 1))
    res.append(eng.results_wait((steps - 1) & 1))
    eng.sync()
    ptr, n = eng.grad_arena()
    arena = torch.as_tensor(_DevArray(ptr, n), device='cuda:0').cpu().numpy()
    W = eng.get_params()
    host_sum = tr.allreduce([rank, -rank, 2.0 ** 40 + rank], 'sum')
    host_max = tr.allreduce([rank, -rank, 2.0 ** 40 + rank], 'max')
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), losses=np.asarray([r[0] for r in res], np.float32),
             accs=np.asarray([r[1] for r in res], np.float32), arena=arena, optimizer_steps=np.asarray(eng.optimizer_steps()),
             host_sum=np.asarray(host_sum), host_max=np.asarray(host_max), shard=np.asarray([lo, hi]),
             **{'p:' + k: W[k] for k in W})
    dist.barrier()
    dist.destroy_process_group()
    eng.comm_destroy()
    eng.close()


def orphan(world):
    """l3_comm_init(world, rank 0) that fails; then: no communicator is left, l3_step_dp refuses, and a second l3_comm_init
    (world 1) gives a data-parallel step equal to the resident step bit for bit."""
    from l3embedding_amd import _lib
    from oracle import l3_oracle as o
    mt, B = 'tiny_L3', 2
    e1 = _lib.Engine(mt, B, seed=5, global_batch=B)
    live_head(e1)
    e2 = _lib.Engine(mt, B, seed=5)
    e2.set_params(e1.get_params())
    out = {}
    t0 = time.perf_counter()
    try:
        e1.comm_init(_lib.comm_unique_id(), world, 0)   # no gloo group: a lone rank would block in it
        out['error'] = None
    except _lib.L3Error as exc:
        out['error'] = str(exc)
    out['init_s'] = time.perf_counter() - t0
    out['world_after'] = e1.comm_info()['world']
    try:
        e1.step_dp(1e-3)
        out['step_dp_error'] = None
    except _lib.L3Error as exc:
        out['step_dp_error'] = str(exc)
    try:
        e1.comm_init(_lib.comm_unique_id(), 1, 0)
        out['retry_error'] = None
    except _lib.L3Error as exc:
        out['retry_error'] = str(exc)
        print('RESULT ' + json.dumps(out))
        return
    info = e1.comm_info()
    out['library'], out['world_retry'] = info['library'], info['world']
    v, a, l = o.synthetic_batch(B, seed=71)
    e1.upload_batch(v, a, l)
    e2.upload_batch(v, a, l)
    e1.step_dp(1e-3)
    e2.step_resident(1e-3)
    out['results_equal'] = e1.step_results() == e2.step_results()
    Wa, Wb = e1.get_params(), e2.get_params()
    out['param_mismatch'] = [k for k in Wb if not np.array_equal(Wa[k], Wb[k])]
    out['n_tensors'] = len(Wb)
    fake = ctypes.CDLL(info['library'])
    fake.fake_rccl_launches.restype = ctypes.c_long
    out['collectives'] = int(fake.fake_rccl_launches())
    e1.comm_destroy()
    e1.close()
    e2.close()
    print('RESULT ' + json.dumps(out))


def main():
    if sys.argv[1] == 'train':
        return train(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), float(sys.argv[6]))
    if sys.argv[1] == 'orphan':
        return orphan(int(sys.argv[2]))
    raise SystemExit('unknown mode %r' % sys.argv[1])


if __name__ == '__main__':
    main()
