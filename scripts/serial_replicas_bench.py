"""l3_step_replicas against l3_step_resident (the record profiles/r25_serial_replicas.txt): cnn_L3_melspec2, R slices of B pairs.
One process, in this order: the resident step at batch B, then the replicas step at global batch R * B; hipEvents on the engines'
stream between the steps (a step's time = the distance of the events around it), warm-up steps first.  Also the device memory
each engine adds.  usage: python scripts/serial_replicas_bench.py [dtype f32|bf16] [B] [R] [timed steps] [warm-up steps]
(under rocprofv3 --kernel-trace --stats: a few steps are enough; arena_fold_kernel's rows give the fold's own time)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch  # first: one HIP runtime in the process

from l3embedding_amd import _lib

dtype = sys.argv[1] if len(sys.argv) > 1 else 'f32'
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
R = int(sys.argv[3]) if len(sys.argv) > 3 else 8
STEPS = int(sys.argv[4]) if len(sys.argv) > 4 else 20
WARM = int(sys.argv[5]) if len(sys.argv) > 5 else 5
MT, LR = 'cnn_L3_melspec2', 1e-4


def used_mib():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 2.0 ** 20


def live_head(eng):
    shape = dict((n, s) for n, s, _ in eng.param_table())['dense_2/kernel']
    eng.set_param('dense_2/kernel', eng.get_param('dense_2/kernel', shape) * np.float32(1.0 / 64))


def raw_batch(rows, seed):
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, 2, rows)
    return (rs.randint(0, 256, (rows, 224, 224, 3), dtype=np.uint8), rs.randint(-32768, 32768, (rows, 1, 48000)).astype(np.int16),
            np.stack([lab, 1 - lab], 1).astype(np.int32))


def timed(eng, stream, step):
    for _ in range(WARM):
        step(LR)
    eng.sync()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS + 1)]
    evs[0].record(stream)
    for k in range(STEPS):
        step(LR)
        evs[k + 1].record(stream)
    eng.sync()
    return np.array([evs[k].elapsed_time(evs[k + 1]) for k in range(STEPS)])


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), p10=float(np.percentile(ms, 10)),
                p90=float(np.percentile(ms, 90)))


torch.cuda.set_device(0)
stream = torch.cuda.Stream(device=0)
base = used_mib()
e1 = _lib.Engine(MT, B, dtype=dtype, stream=stream.cuda_stream)
live_head(e1)
e1.upload_batch_raw(*raw_batch(B, 0))
res = timed(e1, stream, e1.step_resident)
mem_resident = used_mib() - base
arena_bytes = 4 * e1.grad_arena()[1]
e1.close()
del e1
base = used_mib()
e2 = _lib.Engine(MT, B, global_batch=R * B, dtype=dtype, stream=stream.cuda_stream)
live_head(e2)
e2.replicas_upload_raw(*raw_batch(R * B, 1), R)
rep = timed(e2, stream, e2.step_replicas)
mem_replicas = used_mib() - base
loss, acc = e2.step_results()
assert np.isfinite(loss) and e2.optimizer_steps() == (WARM + STEPS, R * (WARM + STEPS))
e2.close()
r, p = stats(res), stats(rep)
out = dict(model=MT, dtype=dtype, B=B, R=R, steps=STEPS, warmup=WARM, resident_ms=r, replicas_ms=p,
           resident_pairs_per_s=B / r['median'] * 1e3, replicas_pairs_per_s=R * B / p['median'] * 1e3,
           ratio_to_R_resident=p['median'] / (R * r['median']), resident_spread=(r['p90'] - r['p10']) / r['median'],
           arena_bytes=arena_bytes, fold_bytes_per_launch=3 * arena_bytes, mem_resident_mib=mem_resident, mem_replicas_mib=mem_replicas)
print('%s B %d R %d: resident %.3f ms/step (p10 %.3f, p90 %.3f), %.0f pairs/s; replicas %.3f ms/global step (p10 %.3f, p90 %.3f), '
      '%.0f pairs/s; ratio to %d x resident %.4f; device memory +%.0f MiB (resident engine), +%.0f MiB (replicas engine)'
      % (dtype, B, R, r['median'], r['p10'], r['p90'], out['resident_pairs_per_s'], p['median'], p['p10'], p['p90'],
         out['replicas_pairs_per_s'], R, out['ratio_to_R_resident'], mem_resident, mem_replicas))
print('RESULT ' + json.dumps(out))
