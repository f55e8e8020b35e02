"""float64 NumPy restatement of the downstream MLP classifier's training step (classifier/train.py:230-391 under keras 2.0.9):
Dense(512, relu) -> Dense(128, relu) -> Dense(C, softmax), L2 kernel_regularizer, categorical_crossentropy, Adam.  The yardstick
of tests/test_classifier_gpu.py."""
import numpy as np

EPS = 1e-7
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


def forward(W, X):
    W1, b1, W2, b2, W3, b3 = W
    h1 = np.maximum(X @ W1 + b1, 0.0)
    h2 = np.maximum(h1 @ W2 + b2, 0.0)
    z = h2 @ W3 + b3
    return h1, h2, z


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softmax_ce(z, labels, gscale):
    """keras categorical_crossentropy on softmax(z): per-row loss, d(sum loss * gscale)/dz, probs, per-row correct"""
    p = softmax(z)
    t = np.zeros_like(p)
    t[np.arange(len(labels)), labels] = 1.0
    sm = p.sum(axis=1, keepdims=True)
    q = p / sm
    c = np.clip(q, EPS, 1 - EPS)
    ce = -(t * np.log(c)).sum(axis=1)
    inside = (q >= EPS) & (q <= 1 - EPS)
    dq = np.where(inside, -t / c * gscale, 0.0)
    dp = dq / sm - (dq * p).sum(axis=1, keepdims=True) / sm ** 2
    dz = p * (dp - (dp * p).sum(axis=1, keepdims=True))
    correct = (p.argmax(axis=1) == labels).astype(np.float64)
    return ce, dz, p, correct


def l2(W, wd):
    return wd * sum(float((W[i] ** 2).sum()) for i in (0, 2, 4))


def grads(W, X, labels):
    """-> (mean ce, correct count, [dW1, db1, dW2, db2, dW3, db3]) of one batch, without the L2 term"""
    h1, h2, z = forward(W, X)
    n = len(labels)
    ce, dz, _, correct = softmax_ce(z, labels, 1.0 / n)
    dh2 = (dz @ W[4].T) * (h2 > 0)
    dh1 = (dh2 @ W[2].T) * (h1 > 0)
    g = [X.T @ dh1, dh1.sum(0), h1.T @ dh2, dh2.sum(0), h2.T @ dz, dz.sum(0)]
    return ce.mean(), correct.sum(), g


def adam(W, g, m, v, lr, t, wd):
    lr_t = lr * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    out = []
    for i in range(6):
        gi = g[i] + (2 * wd * W[i] if i % 2 == 0 else 0.0)
        m[i] = B1 * m[i] + (1 - B1) * gi
        v[i] = B2 * v[i] + (1 - B2) * gi * gi
        out.append(W[i] - lr_t * m[i] / (np.sqrt(v[i]) + ADAM_EPS))
    return out


def epoch(W, m, v, X, y, perm, lr, t0, batch, wd, Xv=None, yv=None):
    """One keras fit epoch -> (W, stats dict, per-step first-layer gradients of the first step)"""
    n = len(perm)
    loss = acc = 0.0
    t = t0
    for s in range(0, n, batch):
        idx = perm[s:s + batch]
        ce, cor, g = grads(W, X[idx], y[idx])
        loss += (ce + l2(W, wd)) * len(idx)
        acc += cor
        t += 1
        W = adam(W, g, m, v, lr, t, wd)
    stats = dict(loss=loss / n, acc=acc / n)
    if Xv is not None:
        _, _, z = forward(W, Xv)
        ce, _, _, cor = softmax_ce(z, yv, 1.0)
        stats.update(val_loss=ce.mean() + l2(W, wd), val_acc=cor.mean())
    return W, stats
