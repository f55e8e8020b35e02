"""NumPy references of the sound classifier's device steps (l3embedding_amd/sound.py): the per-file mean of float32 class
probabilities with its arg-max, written out addition by addition, and the inputs its tests share."""
import numpy as np

HOP = 4800
F = 48000
# the ragged clips of test_clip_embedding_gpu.py: empty, short, exactly one second, frame counts that straddle batches of 2 and 3
LENGTHS = [30000, 0, F + 4 * HOP + 7, 100, F, F + 2 * HOP]


def clips(lengths, seed):
    r = np.random.RandomState(seed)
    return [(0.5 * r.randn(n)).astype(np.float32) for n in lengths]


def file_mean(probs, file_idxs):
    """-> (mean (F, C) float32, pred (F,) int64) of the rows [s, e) of each file: a float32 sum taken row after row, one float32
    division by float32(e - s), and the first maximum -- what probs[s:e].mean(axis=0).argmax() computes on float32 rows, spelled
    out so that the order of the additions is on the page"""
    probs = np.asarray(probs)
    assert probs.dtype == np.float32 and probs.ndim == 2
    means, preds = [], []
    for s, e in np.asarray(file_idxs, np.int64).reshape(-1, 2):
        acc = np.zeros(probs.shape[1], np.float32)
        for r in range(s, e):
            acc = acc + probs[r]                      # float32 + float32, rounded once
        mean = acc / np.float32(e - s)
        means.append(mean)
        best = 0
        for c in range(1, mean.size):
            if mean[c] > mean[best]:                  # strictly greater: the first maximum stays
                best = c
        preds.append(best)
    return np.stack(means).astype(np.float32), np.array(preds, np.int64)


def softmax32(logits):
    """a float32 softmax of float32 logits, row by row"""
    z = np.asarray(logits, np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True)).astype(np.float32)
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def file_mean_case(C, seed=0):
    """probabilities (n, C) and a table of files of 1, 2, 63, 64, 65 and 1000 rows plus one of 2 rows whose two best classes tie
    exactly (the lower index must win)"""
    sizes = [1, 2, 63, 64, 65, 1000, 2]
    ends = np.cumsum(sizes)
    files = np.stack((ends - sizes, ends), axis=1).astype(np.int64)
    r = np.random.RandomState(1000 * C + seed)
    probs = softmax32(3.0 * r.randn(int(ends[-1]), C))
    # the tie: two rows that mirror each other in the classes hi > lo, every other class smaller
    s = int(files[-1, 0])
    lo, hi = (0, 1) if C == 2 else (1, C - 1)
    row = np.full(C, 0.0, np.float32)
    row[lo], row[hi] = 0.5, 0.25
    if C > 2:
        rest = [c for c in range(C) if c not in (lo, hi)]
        row[rest] = np.float32(0.25) / np.float32(len(rest)) * np.float32(0.5)
    mirrored = row.copy()
    mirrored[lo], mirrored[hi] = row[hi], row[lo]
    probs[s], probs[s + 1] = row, mirrored
    return probs, files
