"""bench.py's command line: what a plain run prints, `--dump-outputs` (the arrays of the last timed step) and its size cap."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_float32_arrays_whole_under_the_cap(tmp_path):
    bench = _bench()
    arrays = [('loss', 0.5), ('probs', np.arange(6, dtype=np.float64).reshape(3, 2)), ('param.a.kernel', np.ones((4, 5), np.float32))]
    bench.dump_outputs(str(tmp_path / 'out'), arrays)
    got = {f[:-4]: np.load(str(tmp_path / 'out' / f)) for f in os.listdir(str(tmp_path / 'out'))}
    assert sorted(got) == ['loss', 'param.a.kernel', 'probs']
    assert all(a.dtype == np.float32 for a in got.values())
    assert got['loss'] == np.float32(0.5) and np.array_equal(got['probs'], arrays[1][1]) and got['param.a.kernel'].shape == (4, 5)


def test_dump_outputs_samples_the_same_elements_when_over_the_cap(tmp_path):
    """Over the cap every large array becomes a fixed sample of its elements: the files stay within the cap and two runs
    (or two builds) write the same indices."""
    bench = _bench()
    rng = np.random.RandomState(0)
    arrays = [('small', np.ones(10)), ('big1', rng.rand(5000)), ('big2', rng.rand(70, 90))]
    cap = 3 * 4 * 1000
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays, max_bytes=cap)
    total = sum(os.path.getsize(str(tmp_path / 'a' / f)) - 128 for f in os.listdir(str(tmp_path / 'a')))   # minus the .npy headers
    assert total <= cap
    for name, a in arrays:
        x, y = np.load(str(tmp_path / 'a' / (name + '.npy'))), np.load(str(tmp_path / 'b' / (name + '.npy')))
        assert np.array_equal(x, y)
        flat = np.asarray(a, np.float32).ravel()
        assert np.isin(x.ravel(), flat).all() and (x.size == flat.size) == (name == 'small')


def test_bench_rejects_zero_steps(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '0', '--warmup', '1'])
    with pytest.raises(SystemExit):
        bench.main()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(gpu_required, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` times exactly K steps and prints the headline fields without any of what
    --full adds; --dump-outputs holds the last timed step's loss (the line's final_loss), probabilities and parameters."""
    out = tmp_path / 'dump'
    env = dict(os.environ)
    env.pop('L3_DEBUG_KNOBS', None)          # the product configuration, as the benchmark is run
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(out)],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors='replace')[-3000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line, k
    assert line['steps'] == 3 and line['warmup'] == 1 and line['unit'] == 'pairs/s' and line['dtype'] == 'f32'
    assert abs(line['value'] - 64 * 1e3 / line['ms_per_step']) < 1e-6 * line['value']
    for k in ('roofline', 'kernels', 'secondary', 'value_saturated_head', 'x_cpu_baseline'):
        assert k not in line, k
    assert line['cpu_baseline'] is None
    files = sorted(os.listdir(str(out)))
    assert {'loss.npy', 'accuracy.npy', 'probs.npy', 'logits.npy'} <= set(files)
    assert sum(os.path.getsize(str(out / f)) for f in files) <= 64 * 10 ** 6
    loss, probs = np.load(str(out / 'loss.npy')), np.load(str(out / 'probs.npy'))
    assert loss.dtype == np.float32 and loss == np.float32(line['final_loss'])
    assert probs.shape == (64, 2) and np.allclose(probs.sum(axis=1), 1.0, atol=1e-5)
    params = [f for f in files if f.startswith('param.')]
    assert 'param.dense_2.kernel.npy' in params and len(params) > 100
    assert all(np.isfinite(np.load(str(out / f))).all() for f in params)
