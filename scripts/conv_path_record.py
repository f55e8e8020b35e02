"""SHA-256 digests of everything that runs through the per-convolution kernel path (csrc/conv_path.h): the convolution operators,
the engine's passes and embeddings, VGGish.  Run it on two commits (same GPU, same ROCm, a clean build and a process of its own
for each) and compare: a change that only moves host dispatch leaves every digest equal.

    python scripts/conv_path_record.py --out a.json [--root TREE]       # TREE: the built checkout to load (default: this one)
    python scripts/conv_path_record.py --compare a.json b.json          # prints the verdict; exit status 1 unless all equal

Every case runs twice in the process; a tensor that does not repeat is flagged ('repeats': false) and, where it is an
operator's weight or bias gradient, its distance from the float64 oracle is recorded instead (relative to the range, the
measure of tests/test_layer_parity_gpu.py).  Forward and data-gradient tensors must repeat.  Also the launch counts per kernel
family (Engine.profile_read) of one fp32 and one bf16 training step."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

OP_SHAPES = [  # (n, h, w, cin, cout, k, same)
    (2, 9, 33, 3, 64, 3, True), (1, 8, 40, 1, 64, 3, True),          # first layer, a ragged 32-pixel run
    (2, 12, 20, 64, 64, 3, True), (1, 7, 9, 64, 128, 3, True),       # F(4x4,3x3), ragged tiles
    (2, 10, 6, 16, 64, 3, True),                                     # F(2x2,3x3) by channel count
    (2, 6, 7, 10, 10, 5, False), (1, 9, 9, 4, 12, 3, False)]         # direct
OP_DTYPES = ['f32', 'bf16', 'bf16_stored', 'bf16_stored_out']
# fp32 algorithm of the operators: the product's, F(2x2,3x3) as tests/test_layer_parity_gpu.py sets it, and through l3_config's knob
OP_ENVS = [('product', {}), ('wino4=0', {'L3_WINO4': '0'}), ('fp32_conv=f2x2', {'L3_FP32_CONV': 'f2x2'})]


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


class Recorder(object):
    def __init__(self):
        self.cases = {}

    def run(self, name, fn, oracle=None):
        """fn() -> {tensor name: array}, called twice; oracle(tensor name) -> float64 array for a tensor that does not repeat"""
        first, second = fn(), fn()
        out = {}
        for k in first:
            rep = np.array_equal(first[k], second[k])
            out[k] = {'sha256': digest(first[k]), 'repeats': bool(rep)}
            if not rep and oracle is not None:
                ref = oracle(k)
                out[k]['oracle_relerr'] = [relerr(first[k], ref), relerr(second[k], ref)]
        self.cases[name] = out
        bad = [k for k, v in out.items() if not v['repeats']]
        print('%-64s %2d tensors%s' % (name, len(out), ', NOT repeating: %s' % bad if bad else ''), flush=True)


def op_cases(rec, _lib, o):
    for n, h, w, ci, co, k, same in OP_SHAPES:
        rng = np.random.RandomState(n + 3 * h + 5 * w + 7 * ci + 11 * co)
        x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
        wt = (rng.standard_normal((k, k, ci, co)) * np.sqrt(2.0 / (k * k * ci))).astype(np.float32)
        b = (0.1 * rng.standard_normal(co)).astype(np.float32)
        ho, wo = (h, w) if same else (h - k + 1, w - k + 1)
        dy = (rng.standard_normal((n, ho, wo, co)) * 1e-3).astype(np.float32)
        pad = 'same' if same else 'valid'

        def oracle(name):
            dx, dw, db = o.conv2d_bwd(x.astype(np.float64), wt.astype(np.float64), dy.astype(np.float64), pad)
            return {'dx': dx, 'dw': dw, 'db': db}[name]

        for env_name, env in OP_ENVS:
            for key in ('L3_WINO4', 'L3_FP32_CONV'):
                os.environ.pop(key, None)
            os.environ.update(env)
            for dt in OP_DTYPES:
                tag = '%dx%dx%dx%d->%d k%d %s %s %s' % (n, h, w, ci, co, k, pad, dt, env_name)
                rec.run('op_conv2d_fwd ' + tag, lambda: {'y': _lib.op_conv2d_fwd(x, wt, b, same, dtype=dt)})
                rec.run('op_conv2d_bwd ' + tag, lambda: dict(zip(('dx', 'dw', 'db'), _lib.op_conv2d_bwd(x, wt, dy, same, dtype=dt))),
                        oracle)
    for key in ('L3_WINO4', 'L3_FP32_CONV'):
        os.environ.pop(key, None)


def engine_cases(rec, _lib, o, plan):
    launches = {}
    for mt, B, dtype, conv in [('cnn_L3_melspec2', 2, 'f32', 'f4x4'), ('cnn_L3_melspec2', 2, 'f32', 'f2x2'),
                               ('cnn_L3_melspec2', 2, 'bf16', 'f4x4'), ('tiny_L3', 3, 'f32', 'f4x4')]:
        tag = '%s b%d %s %s' % (mt, B, dtype, conv)
        P = o.init_params(mt, seed=7)
        P['dense_2/kernel'] = (P['dense_2/kernel'] / np.float32(64)).astype(np.float32)      # a live head (tests/test_tower_plan_gpu.py)
        batch = o.synthetic_batch(B, seed=11)
        eng = _lib.Engine(mt, B, seed=0, dtype=dtype, fp32_conv=conv)
        eng.set_params(P)
        rec.run('engine pass ' + tag, lambda: plan._pass(eng, batch))

        def tower(tw):
            eng.upload_batch(*batch)
            eng.tower_step(tw, backward=True)
            eng.sync()
            return {'grad ' + n: g for n, g in eng.get_grads().items()}

        for tw in ('vision', 'audio'):
            rec.run('engine tower_step %s %s' % (tw, tag), lambda: tower(tw))
        rec.run('engine forward ' + tag, lambda: dict(zip(('probs', 'logits'), eng.forward(batch[0], batch[1], training=False))))
        if mt == 'cnn_L3_melspec2':
            v3, a3, _ = o.synthetic_batch(3, seed=52)
            for pooling in ('original', 'short'):
                rec.run('engine embed_audio %s %s' % (pooling, tag), lambda: {'emb': eng.embed_audio(a3, o.AUDIO_POOLING[mt][pooling])})
            rec.run('engine embed_vision ' + tag, lambda: {'emb': eng.embed_vision(v3)})
            if conv == 'f4x4':
                eng.profile_enable(True)
                eng.train_step(batch[0], batch[1], batch[2], 1e-4)
                eng.sync()
                launches['%s step' % dtype] = {fam: r['launches'] for fam, r in eng.profile_read().items()}
                eng.profile_enable(False)
        eng.close()
    return launches


def vggish_cases(rec, _lib):
    from l3embedding_amd import resample, vggish
    rng = np.random.RandomState(5)
    x = np.maximum(rng.standard_normal((2, 8, 12, 64)), 0).astype(np.float32)
    k = (rng.standard_normal((3, 3, 64, 128)) * np.sqrt(2.0 / (9 * 64))).astype(np.float32)
    b = (rng.standard_normal(128) * 0.05).astype(np.float32)
    for algo in ('f4x4', 'f2x2', 'direct'):
        for pool in (0, 1):
            rec.run('op_vggish_conv 2x8x12x64->128 pool %d %s' % (pool, algo), lambda: {'y': _lib.op_vggish_conv(x, k, b, pool, algo)})
    layers = [('conv1', 1, 64), ('conv2', 64, 128), ('conv3/conv3_1', 128, 256), ('conv3/conv3_2', 256, 256), ('conv4/conv4_1', 256, 512),
              ('conv4/conv4_2', 512, 512)]
    dense = [('fc1/fc1_1', 12288, 4096), ('fc1/fc1_2', 4096, 4096), ('fc2', 4096, 128)]
    rng = np.random.RandomState(3)
    clip = rng.standard_normal(44100).astype(np.float32) * 0.1          # one second at 44.1 kHz
    win, nt = resample.kaiser_best()
    n16 = resample.output_length(clip.size, 44100, 16000)
    pads, rows, _ = vggish.example_table([n16], 0.96)
    for algo in ('direct', 'f4x4', 'f2x2'):
        net = _lib.VGGish(batch=4)
        net.set_conv(algo)
        wr = np.random.RandomState(3)
        for name, cin, cout in layers:
            net.set_weight('vggish/%s/weights' % name, (wr.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
            net.set_weight('vggish/%s/biases' % name, (wr.standard_normal(cout) * 0.05).astype(np.float32))
        for name, cin, cout in dense:
            net.set_weight('vggish/%s/weights' % name, (wr.standard_normal((cin, cout)) * np.sqrt(2.0 / cin)).astype(np.float32))
            net.set_weight('vggish/%s/biases' % name, (wr.standard_normal(cout) * 0.05).astype(np.float32))
        rec.run('vggish embed_clips_resampled 1 s %s' % algo, lambda: {'emb': net.embed_clips_resampled(
            clip, [[0, clip.size, 44100, 0, n16, int(pads[0, 0])]], win, nt, int(pads[0, 1]), [[0, int(pads[0, 1])]], rows, 'raw')})
        net.close()


def record(root, out):
    root = os.path.abspath(root)
    sys.path[:0] = [root, os.path.join(root, 'tests')]
    from l3embedding_amd import _lib
    from oracle import l3_oracle as o
    import test_tower_plan_gpu as plan
    assert os.path.abspath(_lib.__file__).startswith(root + os.sep), _lib.__file__
    rec = Recorder()
    op_cases(rec, _lib, o)
    launches = engine_cases(rec, _lib, o, plan)
    vggish_cases(rec, _lib)
    with open(out, 'w') as fh:
        json.dump({'cases': rec.cases, 'launches': launches}, fh, indent=1, sort_keys=True)
    print('%d cases -> %s' % (len(rec.cases), out))


def compare(path_a, path_b, oracle_bound=3e-6):
    a, b = json.load(open(path_a)), json.load(open(path_b))
    ok = a['cases'].keys() == b['cases'].keys()
    print('cases: %d and %d%s' % (len(a['cases']), len(b['cases']), '' if ok else ' -- DIFFERENT LISTS'))
    tensors = differ = set_aside = 0
    for name in sorted(set(a['cases']) & set(b['cases'])):
        for k, ta in a['cases'][name].items():
            tb = b['cases'][name][k]
            tensors += 1
            if ta['repeats'] and tb['repeats']:
                if ta['sha256'] != tb['sha256']:
                    differ += 1
                    print('DIFFERS      %s: %s' % (name, k))
                continue
            # a tensor that does not repeat on the first commit: only an operator's weight / bias gradient may be set aside
            set_aside += 1
            errs = ta.get('oracle_relerr', []) + tb.get('oracle_relerr', [])
            fine = k in ('dw', 'db') and not ta['repeats'] and errs and max(errs) < oracle_bound
            print('%s %s: %s repeats %s / %s, float64 oracle distances %s (bound %.1e)'
                  % ('SET ASIDE   ' if fine else 'NOT REPEATING', name, k, ta['repeats'], tb['repeats'], errs, oracle_bound))
            ok = ok and bool(fine)
    same_launches = a['launches'] == b['launches']
    for step in sorted(a['launches']):
        print('launches %s: %s' % (step, json.dumps(a['launches'][step], sort_keys=True)))
        if b['launches'].get(step) != a['launches'][step]:
            print('      second: %s' % json.dumps(b['launches'].get(step), sort_keys=True))
    ok = ok and differ == 0 and same_launches
    print('%d tensors compared, %d differ, %d set aside, launch counts %s: %s'
          % (tensors, differ, set_aside, 'equal' if same_launches else 'DIFFERENT', 'ALL EQUAL' if ok else 'NOT EQUAL'))
    return 0 if ok else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out')
    ap.add_argument('--root', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error('--out or --compare')
    record(args.root, args.out)
