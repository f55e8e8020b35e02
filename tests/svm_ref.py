"""Float64 NumPy restatement of what the SVM classifier computes (libsvm 3.x svm.cpp as bundled by scikit-learn 0.19, and
sklearn 0.19's wrappers): the four kernel functions, the C-SVC solver with libsvm's second-order working-set selection (WSS3)
and its rho, one-vs-one training and decision values, sigmoid_train / sigmoid_predict / multiclass_probability,
_ovr_decision_function and hinge_loss.  Plain loops, written for small n; the oracle of tests/test_svm_*.py."""
import math

import numpy as np

TAU = 1e-12
KINDS = ('linear', 'poly', 'rbf', 'sigmoid')


def kernel_matrix(A, B, kind, gamma, coef0=0.0, degree=3):
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    dot = A @ B.T
    if kind == 'linear':
        return dot
    if kind == 'poly':
        return (gamma * dot + coef0) ** degree
    if kind == 'rbf':
        d = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2 * dot
        return np.exp(-gamma * np.maximum(d, 0.0))
    if kind == 'sigmoid':
        return np.tanh(gamma * dot + coef0)
    raise ValueError(kind)


def dk_ddot(kind, K, dot, gamma, coef0=0.0, degree=3):
    """|dK / d(u.v)| in float64: how far a rounding of the dot product moves the kernel value"""
    if kind == 'linear':
        return np.ones_like(K)
    if kind == 'poly':
        if degree == 0:
            return np.zeros_like(K)
        return np.abs(degree * gamma * (gamma * dot + coef0) ** (degree - 1))
    if kind == 'rbf':
        return 2 * gamma * K
    return gamma * (1 - K * K)


def kernel_rows_bound(A, B, kind, gamma, coef0=0.0, degree=3):
    """-> (K, bK): the float64 kernel matrix and the project's bound on an fp32 MFMA kernel row against it (the comment above
    test_svm_gpu.py: test_kernel_rows_match_float64): 2.5e-7 sqrt(D) |dK/d dot| S + 1e-6 |K| + 1e-7, S = sum |u_k v_k| (rbf:
    + |u|^2 + |v|^2)"""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    K = kernel_matrix(A, B, kind, gamma, coef0, degree)
    S = np.abs(A) @ np.abs(B).T
    if kind == 'rbf':
        S = S + (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :]
    bK = 2.5e-7 * np.sqrt(A.shape[1]) * dk_ddot(kind, K, A @ B.T, gamma, coef0, degree) * S + 1e-6 * np.abs(K) + 1e-7
    return K, bK


def pair_index(i, j, nc):
    """the column of pair (i, j), i < j, in libsvm's order (0, 1), (0, 2), ..., (1, 2), ..."""
    return i * nc - i * (i + 1) // 2 + (j - i - 1)


def ovo_decision_bound(Xt, SV, n_support, coef, rho, kind, gamma, coef0=0.0, degree=3):
    """ovo_decision and the bound on fp32 kernel values summed in float64 against it, per element: sum_s |coef_s| bK[m, s] over
    the pair's two classes' support vectors + 1e-12 (sum_s |coef_s K[m, s]| + |rho|).  -> (dec, bound), both (n, P)"""
    K, bK = kernel_rows_bound(Xt, SV, kind, gamma, coef0, degree)
    coef = np.asarray(coef, np.float64).reshape(len(n_support) - 1, -1)
    absK, absc = np.abs(K), np.abs(coef)
    start = np.concatenate(([0], np.cumsum(n_support))).astype(np.int64)
    nc = len(n_support)
    dec = np.empty((K.shape[0], nc * (nc - 1) // 2))
    bound = np.empty_like(dec)
    p = 0
    for i in range(nc):
        for j in range(i + 1, nc):
            si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
            dec[:, p] = K[:, si] @ coef[j - 1, si] + K[:, sj] @ coef[i, sj] - rho[p]
            bound[:, p] = (bK[:, si] @ absc[j - 1, si] + bK[:, sj] @ absc[i, sj]
                           + 1e-12 * (absK[:, si] @ absc[j - 1, si] + absK[:, sj] @ absc[i, sj] + abs(rho[p])))
            p += 1
    return dec, bound


def ovo_vote(dec, nc):
    """libsvm's one-vs-one vote over decision values (n, P): the class index with the most wins, ties to the lower class"""
    votes = np.zeros((dec.shape[0], nc), np.int64)
    p = 0
    for i in range(nc):
        for j in range(i + 1, nc):
            win = dec[:, p] > 0
            votes[win, i] += 1
            votes[~win, j] += 1
            p += 1
    return votes.argmax(axis=1)


def solve(K, y, C, eps, alpha=None, G=None, max_updates=None, local_rel=0.0):
    """libsvm Solver::Solve (C-SVC, Cp = Cn = C, no shrinking) on the kernel matrix K of the problem's rows, y in {+1, -1}:
    min 1/2 a^T Q a - e^T a, Q = y y^T K, 0 <= a <= C, y^T a = 0.  Starts from alpha / G (default 0 / -1).  Stops when
    m(a) - M(a) < max(eps, local_rel * first gap) (local_rel = 0: libsvm's test), when no pair can move, or after max_updates.
    Ties go to the last index, as libsvm's >= / <= scans do.  -> (alpha, G, updates)"""
    K = np.asarray(K, np.float64)
    y = np.asarray(y, np.float64)
    n = y.size
    a = np.zeros(n) if alpha is None else np.array(alpha, np.float64)
    G = -np.ones(n) if G is None else np.array(G, np.float64)
    QD = np.diag(K).copy()
    upd = 0
    stop_eps = None
    while max_updates is None or upd < max_updates:
        up = ((y > 0) & (a < C)) | ((y < 0) & (a > 0))
        low = ((y > 0) & (a > 0)) | ((y < 0) & (a < C))
        Gmax, i = -math.inf, -1
        if up.any():
            key = np.where(up, -y * G, -np.inf)
            Gmax = key.max()
            i = int(np.flatnonzero(key == Gmax)[-1])          # libsvm's >= scan keeps the last
        Gmax2, j = -math.inf, -1
        if low.any():
            Gmax2 = (y * G)[low].max()
            if i >= 0:
                gd = Gmax + y * G
                ok = low & (gd > 0)
                if ok.any():
                    quad = QD[i] + QD - 2.0 * K[i]
                    obj = np.where(ok, -(gd * gd) / np.where(quad > 0, quad, TAU), np.inf)
                    j = int(np.flatnonzero(obj == obj.min())[-1])
        gap = Gmax + Gmax2
        if stop_eps is None:
            stop_eps = max(eps, local_rel * gap)
        if i < 0 or j < 0 or gap < stop_eps:
            break
        ai, aj = a[i], a[j]
        if y[i] != y[j]:
            quad = QD[i] + QD[j] - 2.0 * K[i, j]
            quad = quad if quad > 0 else TAU
            delta = (-G[i] - G[j]) / quad
            diff = a[i] - a[j]
            a[i] += delta
            a[j] += delta
            if diff > 0:
                if a[j] < 0:
                    a[j], a[i] = 0.0, diff
            elif a[i] < 0:
                a[i], a[j] = 0.0, -diff
            if diff > 0:
                if a[i] > C:
                    a[i], a[j] = C, C - diff
            elif a[j] > C:
                a[j], a[i] = C, C + diff
        else:
            quad = QD[i] + QD[j] - 2.0 * K[i, j]
            quad = quad if quad > 0 else TAU
            delta = (G[i] - G[j]) / quad
            s = a[i] + a[j]
            a[i] -= delta
            a[j] += delta
            if s > C:
                if a[i] > C:
                    a[i], a[j] = C, s - C
            elif a[j] < 0:
                a[j], a[i] = 0.0, s
            if s > C:
                if a[j] > C:
                    a[j], a[i] = C, s - C
            elif a[i] < 0:
                a[i], a[j] = 0.0, s
        dai, daj = a[i] - ai, a[j] - aj
        G += y * y[i] * K[:, i] * dai + y * y[j] * K[:, j] * daj
        upd += 1
    return a, G, upd


def calculate_rho(alpha, G, y, C):
    """libsvm Solver::calculate_rho"""
    ub, lb, s, nf = math.inf, -math.inf, 0.0, 0
    for t in range(y.size):
        yG = y[t] * G[t]
        if alpha[t] >= C:
            if y[t] < 0:
                ub = min(ub, yG)
            else:
                lb = max(lb, yG)
        elif alpha[t] <= 0:
            if y[t] > 0:
                ub = min(ub, yG)
            else:
                lb = max(lb, yG)
        else:
            nf += 1
            s += yG
    return s / nf if nf else (ub + lb) / 2


def optimality(K, y, alpha, C):
    """-> (m(a) - M(a), min alpha, max alpha - C, |y^T a|): the KKT certificate of a C-SVC solution on K"""
    y = np.asarray(y, np.float64)
    G = y * (K @ (y * alpha)) - 1.0
    key = -y * G
    up = ((y > 0) & (alpha < C)) | ((y < 0) & (alpha > 0))
    low = ((y > 0) & (alpha > 0)) | ((y < 0) & (alpha < C))
    m = key[up].max() if up.any() else -math.inf
    M = key[low].min() if low.any() else math.inf
    return m - M, float(alpha.min()), float(alpha.max() - C), abs(float(y @ alpha))


def ovo_fit(X, y, kind, gamma, C, tol, coef0=0.0, degree=3):
    """libsvm svm_train without probability: -> classes, support, n_support, sv_coef (C-1, nSV), rho (P,)"""
    classes, yi = np.unique(y, return_inverse=True)
    nc = classes.size
    groups = [np.flatnonzero(yi == c) for c in range(nc)]
    Kall = kernel_matrix(X, X, kind, gamma, coef0, degree)
    alphas, rhos, pairs = [], [], []
    nonzero = np.zeros(len(y), bool)
    for i in range(nc):
        for j in range(i + 1, nc):
            rows = np.concatenate((groups[i], groups[j]))
            s = np.concatenate((np.ones(groups[i].size), -np.ones(groups[j].size)))
            a, G, _ = solve(Kall[np.ix_(rows, rows)], s, C, tol)
            alphas.append((rows, s * a))
            rhos.append(calculate_rho(a, G, s, C))
            nonzero[rows[a > 0]] = True
            pairs.append((i, j))
    sv = [g[nonzero[g]] for g in groups]
    support = np.concatenate(sv)
    pos = {r: k for k, r in enumerate(support)}
    coef = np.zeros((nc - 1, support.size))
    for (i, j), (rows, ya) in zip(pairs, alphas):
        for r, v in zip(rows, ya):
            if v != 0:
                coef[(j - 1) if y[r] == classes[i] else i, pos[r]] = v
    return classes, support, np.array([s.size for s in sv]), coef, np.array(rhos)


def ovo_decision(Xt, SV, n_support, coef, rho, kind, gamma, coef0=0.0, degree=3):
    """libsvm svm_predict_values: (n, P), positive for the pair's first class"""
    Kt = kernel_matrix(Xt, SV, kind, gamma, coef0, degree)
    start = np.concatenate(([0], np.cumsum(n_support)))
    nc = len(n_support)
    out = []
    p = 0
    for i in range(nc):
        for j in range(i + 1, nc):
            si, sj = slice(start[i], start[i + 1]), slice(start[j], start[j + 1])
            out.append(Kt[:, si] @ coef[j - 1, si] + Kt[:, sj] @ coef[i, sj] - rho[p])
            p += 1
    return np.stack(out, axis=1)


def sigmoid_train(dec, labels):
    """libsvm sigmoid_train, loop for loop"""
    l = len(dec)
    prior1 = sum(1.0 for v in labels if v > 0)
    prior0 = l - prior1
    max_iter, min_step, sigma, eps = 100, 1e-10, 1e-12, 1e-5
    hi, lo = (prior1 + 1.0) / (prior1 + 2.0), 1 / (prior0 + 2.0)
    t = [hi if v > 0 else lo for v in labels]
    A, B = 0.0, math.log((prior0 + 1.0) / (prior1 + 1.0))

    def fun(A, B):
        f = 0.0
        for i in range(l):
            fApB = dec[i] * A + B
            f += t[i] * fApB + math.log(1 + math.exp(-fApB)) if fApB >= 0 else (t[i] - 1) * fApB + math.log(1 + math.exp(fApB))
        return f

    fval = fun(A, B)
    for _ in range(max_iter):
        h11, h22, h21, g1, g2 = sigma, sigma, 0.0, 0.0, 0.0
        for i in range(l):
            fApB = dec[i] * A + B
            if fApB >= 0:
                p, q = math.exp(-fApB) / (1.0 + math.exp(-fApB)), 1.0 / (1.0 + math.exp(-fApB))
            else:
                p, q = 1.0 / (1.0 + math.exp(fApB)), math.exp(fApB) / (1.0 + math.exp(fApB))
            d2 = p * q
            h11 += dec[i] * dec[i] * d2
            h22 += d2
            h21 += dec[i] * d2
            d1 = t[i] - p
            g1 += dec[i] * d1
            g2 += d1
        if abs(g1) < eps and abs(g2) < eps:
            break
        det = h11 * h22 - h21 * h21
        dA = -(h22 * g1 - h21 * g2) / det
        dB = -(-h21 * g1 + h11 * g2) / det
        gd = g1 * dA + g2 * dB
        step = 1.0
        while step >= min_step:
            nA, nB = A + step * dA, B + step * dB
            nf = fun(nA, nB)
            if nf < fval + 0.0001 * step * gd:
                A, B, fval = nA, nB, nf
                break
            step /= 2.0
        if step < min_step:
            break
    return A, B


def sigmoid_predict(dec, A, B):
    fApB = dec * A + B
    return math.exp(-fApB) / (1.0 + math.exp(-fApB)) if fApB >= 0 else 1.0 / (1 + math.exp(fApB))


def multiclass_probability(r):
    """libsvm multiclass_probability for one row: r (k, k) -> p (k,)"""
    k = r.shape[0]
    Q = np.zeros((k, k))
    p = np.full(k, 1.0 / k)
    for t in range(k):
        for j in range(t):
            Q[t, t] += r[j, t] * r[j, t]
            Q[t, j] = Q[j, t]
        for j in range(t + 1, k):
            Q[t, t] += r[j, t] * r[j, t]
            Q[t, j] = -r[j, t] * r[t, j]
    eps = 0.005 / k
    for _ in range(max(100, k)):
        Qp = np.zeros(k)
        pQp = 0.0
        for t in range(k):
            for j in range(k):
                Qp[t] += Q[t, j] * p[j]
            pQp += p[t] * Qp[t]
        if max(abs(Qp[t] - pQp) for t in range(k)) < eps:
            break
        for t in range(k):
            diff = (-Qp[t] + pQp) / Q[t, t]
            p[t] += diff
            pQp = (pQp + diff * (diff * Q[t, t] + 2 * Qp[t])) / (1 + diff) / (1 + diff)
            for j in range(k):
                Qp[j] = (Qp[j] + diff * Q[t, j]) / (1 + diff)
                p[j] /= (1 + diff)
    return p


def predict_proba(dec, probA, probB, n_classes, min_prob=1e-7):
    """libsvm svm_predict_probability from ovo decision values (n, P)"""
    out = np.empty((dec.shape[0], n_classes))
    for m in range(dec.shape[0]):
        r = np.zeros((n_classes, n_classes))
        k = 0
        for i in range(n_classes):
            for j in range(i + 1, n_classes):
                pij = min(max(sigmoid_predict(dec[m, k], probA[k], probB[k]), min_prob), 1 - min_prob)
                r[i, j], r[j, i] = pij, 1 - pij
                k += 1
        out[m] = multiclass_probability(r)
    return out


def ovr_decision_function(predictions, confidences, n_classes):
    """sklearn 0.19 _ovr_decision_function"""
    n = predictions.shape[0]
    votes = np.zeros((n, n_classes))
    conf = np.zeros((n, n_classes))
    k = 0
    for i in range(n_classes):
        for j in range(i + 1, n_classes):
            conf[:, i] -= confidences[:, k]
            conf[:, j] += confidences[:, k]
            votes[predictions[:, k] == 0, i] += 1
            votes[predictions[:, k] == 1, j] += 1
            k += 1
    return votes + conf / (3 * (np.abs(conf) + 1))


def hinge_loss(y, dec, labels):
    """sklearn 0.19 hinge_loss, row by row"""
    labels = list(np.unique(labels))
    dec = np.asarray(dec, np.float64)
    total = 0.0
    for m, t in enumerate(y):
        if dec.ndim == 1:
            margin = (1.0 if t == max(np.unique(y)) else -1.0) * dec[m]
        else:
            c = labels.index(t)
            margin = dec[m, c] - max(dec[m, k] for k in range(dec.shape[1]) if k != c)
        total += max(0.0, 1.0 - margin)
    return total / len(y)
