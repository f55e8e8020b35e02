"""NumPy restatement of resampy 0.2.x resample + resample_f (the numba loop) for 1-D float32 signals: the yardstick of
csrc/resample.hip.  `exact_time=True` puts output t at t * sr_orig / sr_new computed in integers, as the kernel does;
`exact_time=False` keeps resampy's f64 time register, advanced by 1 / ratio once per output, so the deviation can be measured.

Vectorised over the outputs, with the per-output order of the numba loop kept: left wing first, each wing in tap order, and
y = float32(float64(y) + w * float64(x)) after every tap.
"""
import numpy as np


def resample_ref(x, sr_orig, sr_new, win, num_table, exact_time=True):
    x = np.asarray(x, dtype=np.float32)
    sample_ratio = float(sr_new) / sr_orig
    n_out = int(x.size * sample_ratio)
    if n_out < 1:
        raise ValueError('Input signal length={} is too small to resample from {}->{}'.format(x.size, sr_orig, sr_new))
    interp_win = np.array(win, dtype=np.float64)
    if sample_ratio < 1:
        interp_win *= sample_ratio
    interp_delta = np.zeros_like(interp_win)
    interp_delta[:-1] = np.diff(interp_win)
    scale = min(1.0, sample_ratio)
    step = int(scale * num_table)
    nwin = interp_win.shape[0]
    L = x.size
    t = np.arange(n_out, dtype=np.int64)
    if exact_time:
        num = t * int(sr_orig)
        n = num // int(sr_new)
        frac = scale * ((num - n * int(sr_new)).astype(np.float64) / float(sr_new))
    else:
        inc = 1.0 / sample_ratio
        time = np.zeros(n_out, np.float64)
        if n_out > 1:
            time[1:] = np.add.accumulate(np.full(n_out - 1, inc))       # sequential, as the register adds
        n = time.astype(np.int64)
        frac = scale * (time - n)
    xd = x.astype(np.float64)
    y = np.zeros(n_out, np.float32)

    def wing(frac, count, index):
        nonlocal y
        index_frac = frac * num_table
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        cnt = np.minimum(count, (nwin - offset) // step)
        for i in range(int(cnt.max()) if cnt.size else 0):
            m = i < cnt
            j = offset[m] + i * step
            w = interp_win[j] + eta[m] * interp_delta[j]
            y[m] = (y[m].astype(np.float64) + w * xd[index(n[m], i)]).astype(np.float32)

    wing(frac, n + 1, lambda nn, i: nn - i)
    wing(scale - frac, L - n - 1, lambda nn, k: nn + k + 1)
    return y
