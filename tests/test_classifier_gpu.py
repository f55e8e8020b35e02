"""The downstream MLP classifier on the GPU (classifier/train.py:230-391): kernel parity against the float64 restatement in
tests/mlp_ref.py, the fused weight-gradient + Adam kernel bit for bit against the gradient followed by the engine's Adam kernel,
a three-epoch trajectory, determinism, argument validation, and the 06_train_classifier.py-style CLI end to end."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import mlp_ref as ref
from l3embedding_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gather_idx(r, rows, n_x):
    """unsorted row indices with repeats (the first two rows picked twice)"""
    idx = r.randint(0, n_x, size=rows)
    if rows > 3:
        idx[-1] = idx[0]
        idx[-2] = idx[1]
    return idx.astype(np.int32)


def _rel_err(got, exact, scale):
    return float(np.max(np.abs(got.astype(np.float64) - exact) / np.maximum(scale, 1e-30)))


# bound 1e-6 of sum|a*b|; measured on MI355X: at most 8.5e-8 (D = 512, B = 64), 1.5e-8 at D = 57344 (split-K in fixed order)
@pytest.mark.parametrize('D', [512, 6144, 57344])
@pytest.mark.parametrize('B', [64, 17, 1])
def test_dense_fwd_first_layer_gathered(gpu_required, D, B):
    r = np.random.RandomState(D + B)
    n_x = B + 9
    x = r.randn(n_x, D).astype(np.float32)
    w = (r.randn(D, 512) / np.sqrt(D)).astype(np.float32)
    b = r.randn(512).astype(np.float32) * 0.1
    idx = _gather_idx(r, B, n_x)
    got = _lib.op_mlp_dense_fwd(x, w, b, idx=idx, relu=False)
    xa = x[idx].astype(np.float64)
    exact = xa @ w.astype(np.float64) + b
    scale = np.abs(xa) @ np.abs(w.astype(np.float64)) + np.abs(b)
    err = _rel_err(got, exact, scale)
    print('fwd D=%d B=%d: max err / sum|ab| = %.3g' % (D, B, err))
    assert err < 1e-6
    relu = _lib.op_mlp_dense_fwd(x, w, b, idx=idx, relu=True)
    np.testing.assert_array_equal(relu, np.maximum(got, 0))


# bound 1e-6 of sum|a*b|; measured on MI355X: at most 2.0e-7
@pytest.mark.parametrize('C', [10, 50])
@pytest.mark.parametrize('B', [64, 17, 1])
def test_dense_fwd_hidden_layers(gpu_required, C, B):
    r = np.random.RandomState(C * 100 + B)
    for K, N in ((512, 128), (128, C)):
        x = np.maximum(r.randn(B, K), 0).astype(np.float32)
        w = (r.randn(K, N) / np.sqrt(K)).astype(np.float32)
        b = r.randn(N).astype(np.float32)
        got = _lib.op_mlp_dense_fwd(x, w, b, relu=False)
        exact = x.astype(np.float64) @ w + b
        scale = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)) + np.abs(b)
        err = _rel_err(got, exact, scale)
        print('fwd K=%d N=%d B=%d: max err / sum|ab| = %.3g' % (K, N, B, err))
        assert err < 1e-6, (K, N)


# bound 1e-6 of sum|a*b|; measured on MI355X: at most 2.7e-7
@pytest.mark.parametrize('C', [10, 50])
@pytest.mark.parametrize('B', [64, 17, 1])
def test_dense_bwd_x(gpu_required, C, B):
    r = np.random.RandomState(7 * C + B)
    for K, N in ((128, C), (512, 128)):
        dy = r.randn(B, N).astype(np.float32)
        w = r.randn(K, N).astype(np.float32)
        h = np.maximum(r.randn(B, K), 0).astype(np.float32)
        got = _lib.op_mlp_dense_bwd_x(dy, w, h)
        full = dy.astype(np.float64) @ w.T.astype(np.float64)
        scale = np.abs(dy.astype(np.float64)) @ np.abs(w.T.astype(np.float64))
        exact = full * (h > 0)
        err = _rel_err(got, exact, scale)
        print('bwd_x K=%d N=%d B=%d: max err / sum|ab| = %.3g' % (K, N, B, err))
        assert err < 1e-6, (K, N)
        assert np.all(got[h == 0] == 0)


# bound 1e-6 of sum|a*b|; measured on MI355X: at most 3.9e-7 (D = 57344, B = 64), 6.0e-8 at B = 1
@pytest.mark.parametrize('D', [512, 6144, 57344])
@pytest.mark.parametrize('B', [64, 17, 1])
def test_wgrad_gathered(gpu_required, D, B):
    r = np.random.RandomState(3 * D + B)
    n_x = B + 5
    x = r.randn(n_x, D).astype(np.float32)
    dy = r.randn(B, 512).astype(np.float32) / 64
    idx = _gather_idx(r, B, n_x)
    dw, db = _lib.op_mlp_wgrad(x, dy, idx=idx)
    xa, dya = x[idx].astype(np.float64), dy.astype(np.float64)
    err = _rel_err(dw, xa.T @ dya, np.abs(xa.T) @ np.abs(dya))
    print('wgrad D=%d B=%d: max err / sum|ab| = %.3g' % (D, B, err))
    assert err < 1e-6
    assert _rel_err(db, dya.sum(0), np.abs(dya).sum(0)) < 1e-6


@pytest.mark.parametrize('K,N', [(512, 512), (6144, 512), (128, 10), (128, 50), (512, 128)])
@pytest.mark.parametrize('B', [64, 17, 1])
def test_wgrad_adam_bitwise(gpu_required, K, N, B):
    """the fused update equals l3_op_mlp_wgrad followed by the engine's adam_kernel bit for bit"""
    r = np.random.RandomState(K + N + B)
    n_x = B + 3
    x = r.randn(n_x, K).astype(np.float32)
    dy = (r.randn(B, N) / 64).astype(np.float32)
    idx = _gather_idx(r, B, n_x)
    w = r.randn(K, N).astype(np.float32) * 0.05
    b = r.randn(N).astype(np.float32) * 0.05
    mw, vw = (r.randn(K, N) * 1e-3).astype(np.float32), (r.rand(K, N) * 1e-6).astype(np.float32)
    mb, vb = (r.randn(N) * 1e-3).astype(np.float32), (r.rand(N) * 1e-6).astype(np.float32)
    wd, lr_t = 1e-3, 3.7e-4
    (w1, b1, mw1, vw1, mb1, vb1), w2 = _lib.op_mlp_wgrad_adam(x, dy, w, b, mw, vw, mb, vb, wd, lr_t, idx=idx)
    dw, db = _lib.op_mlp_wgrad(x, dy, idx=idx)
    p = np.concatenate([w.ravel(), b])
    g = np.concatenate([dw.ravel(), db])
    pe, me, ve = _lib.op_adam(p, g, np.concatenate([mw.ravel(), mb]), np.concatenate([vw.ravel(), vb]), w.size, 2 * np.float32(wd),
                              lr_t)
    np.testing.assert_array_equal(w1.ravel(), pe[:w.size])
    np.testing.assert_array_equal(b1, pe[w.size:])
    np.testing.assert_array_equal(mw1.ravel(), me[:w.size])
    np.testing.assert_array_equal(vw1.ravel(), ve[:w.size])
    np.testing.assert_array_equal(mb1, me[w.size:])
    np.testing.assert_array_equal(vb1, ve[w.size:])
    assert abs(w2 - float((w.astype(np.float64) ** 2).sum())) < 1e-5 * float((w.astype(np.float64) ** 2).sum())


@pytest.mark.parametrize('C', [2, 10, 50, 64])
def test_softmax_ce(gpu_required, C):
    r = np.random.RandomState(C)
    B = 37
    z = (r.randn(B, C) * 3).astype(np.float32)
    z[0, 1] = 40.0          # p ~ 1: clipped at 1 - 1e-7 (gradient blocked for that entry), the others clipped at 1e-7
    z[1, :] = 0.0           # ties: argmax is the first maximum
    labels = r.randint(0, C, size=B).astype(np.int32)
    labels[0] = 1
    labels[2] = 0
    z[2, 0] = -40.0         # the label's probability clipped at 1e-7
    probs, dz, ce, cor = _lib.op_mlp_softmax_ce(z, labels)
    ce64, dz64, p64, cor64 = ref.softmax_ce(z.astype(np.float64), labels, 1.0 / B)
    np.testing.assert_allclose(probs, p64, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(ce, ce64, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dz, dz64, rtol=1e-4, atol=1e-8)
    np.testing.assert_array_equal(cor, cor64)
    assert np.all(dz[2] == 0)    # q below the clip: no gradient through it
    assert cor[1] == (labels[1] == 0)


def _small_set(D=96, C=10, n=300, nv=70, seed=0):
    r = np.random.RandomState(seed)
    centers = r.randn(C, D) * 1.5
    y = r.randint(0, C, n).astype(np.int32)
    yv = r.randint(0, C, nv).astype(np.int32)
    X = (centers[y] + r.randn(n, D)).astype(np.float32)
    Xv = (centers[yv] + r.randn(nv, D)).astype(np.float32)
    return X, y, Xv, yv


def test_trajectory_three_epochs(gpu_required):
    """Three epochs (B = 32, a partial last batch) against the float64 restatement from the same weights and permutations.
    Measured on MI355X: loss / val_loss within 6.5e-7 relative (bound 1e-4; profiles/r08_mlp_classifier.txt); weights
    within 0.002 lr per element (bound 3 lr: Adam's first, sign-like steps move a weight by about lr whatever its gradient,
    so a relative bound would be meaningless)."""
    X, y, Xv, yv = _small_set()
    D, C, B, lr, wd = X.shape[1], 10, 32, 1e-3, 1e-4
    m = _lib.MLP(D, C, B, weight_decay=wd, seed=5)
    m.set_data(X, y, Xv, yv)
    W = [w.astype(np.float64) for w in m.get_weights()]
    mm = [np.zeros_like(w) for w in W]
    vv = [np.zeros_like(w) for w in W]
    rs = np.random.RandomState(1)
    t = 0
    worst = 0.0
    for e in range(3):
        perm = rs.permutation(len(y)).astype(np.int32)
        got = m.epoch(perm, lr, t)
        W, exp = ref.epoch(W, mm, vv, X.astype(np.float64), y, perm, lr, t, B, wd, Xv.astype(np.float64), yv)
        t += -(-len(y) // B)
        for k in ('loss', 'val_loss'):
            rel = abs(got[k] - exp[k]) / abs(exp[k])
            worst = max(worst, rel)
            assert rel < 1e-4, (e, k, got[k], exp[k])
        assert abs(got['acc'] - exp['acc']) <= 1.0 / len(y) + 1e-12
        assert abs(got['val_acc'] - exp['val_acc']) <= 1.0 / len(yv) + 1e-12
    print('trajectory: worst relative loss distance %.3g' % worst)
    dist = max(float(np.max(np.abs(gw - ew))) for gw, ew in zip(m.get_weights(), W)) / lr
    print('trajectory: worst weight distance %.3g lr' % dist)
    assert dist < 3
    probs = m.predict(Xv)
    _, _, z = ref.forward(W, Xv.astype(np.float64))
    np.testing.assert_allclose(probs, ref.softmax(z), atol=1e-3)
    m.close()


def test_determinism(gpu_required):
    X, y, Xv, yv = _small_set(D=600, n=500, seed=3)
    runs = []
    for _ in range(2):
        m = _lib.MLP(X.shape[1], 10, 64, weight_decay=1e-5, seed=11)
        m.set_data(X, y, Xv, yv)
        rs = np.random.RandomState(2)
        hist = [m.epoch(rs.permutation(len(y)), 1e-3, 8 * e) for e in range(2)]
        runs.append((hist, m.get_weights()))
        m.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)


def test_argument_validation(gpu_required):
    def code(fn):
        with pytest.raises(_lib.L3Error) as ei:
            fn()
        return str(ei.value)
    assert 'error -1' in code(lambda: _lib.MLP(16, 65, 8))
    assert 'error -1' in code(lambda: _lib.MLP(16, 10, 0))
    m = _lib.MLP(16, 10, 8)
    X = np.zeros((4, 16), np.float32)
    assert 'error -1' in code(lambda: m.set_data(X, np.array([0, 1, 10, 2])))
    assert 'error -1' in code(lambda: m.set_data(X, np.array([0, -1, 1, 2])))
    assert 'error -1' in code(lambda: m.set_data(X[:0], np.zeros(0, np.int32)))
    lib = _lib.load()
    y = np.zeros(4, np.int32)
    big = lib.l3_mlp_set_data(m.h, X.ctypes.data, y.ctypes.data, 1 << 40, None, None, 0)       # oversized: rejected unread
    assert big == -1
    huge = lib.l3_mlp_set_data(m.h, X.ctypes.data, y.ctypes.data, (1 << 31) - 1, None, None, 0)
    assert huge == -3
    m.set_data(X, np.array([0, 1, 2, 3]))
    assert 'error -1' in code(lambda: m.epoch(np.array([0, 1, 2, 4]), 1e-3, 0))
    assert 'error -1' in code(lambda: _lib.op_mlp_softmax_ce(np.zeros((2, 65), np.float32), np.zeros(2)))
    assert 'error -1' in code(lambda: _lib.op_mlp_softmax_ce(np.zeros((2, 10), np.float32), np.array([0, 10])))
    assert 'error -1' in code(lambda: _lib.op_mlp_dense_fwd(X, np.zeros((16, 8), np.float32), np.zeros(8, np.float32),
                                                            idx=np.array([0, 4]), relu=False))
    m.close()


def _write_us8k(root, D=512, C=10, files_per_class=6, frames=8, plateau=False, seed=0):
    """features/us8k/<desc>/fold1..fold10/*.npz: Gaussian class clusters (or pure noise for a set made to plateau)"""
    r = np.random.RandomState(seed)
    centers = r.randn(C, D) * (0.0 if plateau else 0.8)
    fdir = os.path.join(root, 'features', 'us8k', 'l3', 'synthetic')
    for f in range(10):
        d = os.path.join(fdir, 'fold%d' % (f + 1))
        os.makedirs(d)
        for c in range(C):
            for k in range(files_per_class // 2 if f % 2 else files_per_class // 3 + 1):
                X = (centers[c] + r.randn(frames, D)).astype(np.float32)
                np.savez(os.path.join(d, '%d-%d-%d.npz' % (f, c, k)), X=X, y=np.array(c))
    return fdir


def _run_cli(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, '-m', 'l3embedding_amd.cli_classifier'] + args, cwd=ROOT, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)


def _results(out):
    found = []
    for dp, _, fn in os.walk(os.path.join(out, 'classifier')):
        if 'results.pkl' in fn:
            found.append(dp)
    assert len(found) == 1, found
    return found[0]


def test_cli_end_to_end(gpu_required, tmp_path):
    fdir = _write_us8k(str(tmp_path))
    out = str(tmp_path / 'out')
    p = _run_cli(['-mt', 'mlp', '-e', '30', '-lr', '1e-3', fdir, out, '3'], timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    d = _results(out)
    with open(os.path.join(d, 'results.pkl'), 'rb') as fh:
        res = pickle.load(fh)
    assert res['test']['accuracy'] > 0.9, res['test']
    assert set(res) == {'train', 'valid', 'test'}
    assert {'loss', 'loss_history', 'accuracy', 'accuracy_history', 'class_accuracy', 'average_class_accuracy'} <= set(res['train'])
    from l3embedding_amd import kerasfile
    ws = kerasfile.load_dense_weights(os.path.join(d, 'model.h5'))
    assert [w.shape for w in ws] == [(512, 512), (512,), (512, 128), (128,), (128, 10), (10,)]
    for name in ('config.json', 'stdizer.pkl', 'min_max_scaler.pkl', 'history_checkpoint.pkl', 'history_csvlog.csv'):
        assert os.path.exists(os.path.join(d, name)), name
    assert '/classifier/us8k/l3/synthetic/framewise/overlap/no-min-max/mlp/fold3/' in d + '/'


def test_cli_early_stopping(gpu_required, tmp_path):
    fdir = _write_us8k(str(tmp_path), plateau=True, files_per_class=3, frames=4)
    out = str(tmp_path / 'out')
    p = _run_cli(['-mt', 'mlp', '-e', '60', '-eap', '2', '-lr', '1e-2', fdir, out, '1'], timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    with open(os.path.join(_results(out), 'results.pkl'), 'rb') as fh:
        res = pickle.load(fh)
    assert len(res['train']['loss_history']) < 60
