"""Band-limited resampling on the GPU -- resampy 0.2.x `resample(x, sr_orig, sr_new, filter='kaiser_best')`, which the
reference's load_audio calls for every clip not at 48 kHz (data/usc/features.py:18-28).

The filter is built here, with NumPy only; the kernel (csrc/resample.hip) takes it as it is.  One deliberate deviation from
resampy: output t sits at the exact rational time t * sr_orig / sr_new, where resampy adds 1 / ratio to an f64 register once per
output.  tests/resample_ref.py restates resampy's loop with either time convention.
"""
import numpy as np

# kaiser_best, as resampy's documentation describes it [3P-UNVERIFIED: from memory of that documentation; resampy's shipped
# table is not compared here]: sinc_window(num_zeros=64, precision=9, window=kaiser(beta=14.769656459379492),
# rolloff=0.9475937167399596)
KAISER_BEST = dict(num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=14.769656459379492)
FILTERS = ('kaiser_best',)

_cache = {}


def kaiser_best():
    """(half_window, num_table): resampy's sinc_window for kaiser_best, float64, 64 * 512 + 1 = 32769 entries, win[0] = rolloff:
    rolloff * sinc(rolloff * linspace(0, 64, 32769)) * kaiser(65537, beta)[32768:].  Cached; do not modify the array."""
    if 'kaiser_best' not in _cache:
        p = KAISER_BEST
        num_table = 2 ** p['precision']
        n = num_table * p['num_zeros']
        sinc_win = p['rolloff'] * np.sinc(p['rolloff'] * np.linspace(0, p['num_zeros'], num=n + 1, endpoint=True))
        taper = np.kaiser(2 * n + 1, p['beta'])[n:]
        win = taper * sinc_win
        win.setflags(write=False)
        _cache['kaiser_best'] = (win, num_table)
    return _cache['kaiser_best']


def get_filter(name):
    if name not in FILTERS:
        raise NotImplementedError('filter %r: only %s is built' % (name, ', '.join(FILTERS)))
    return kaiser_best()


def check_rates(sr_orig, sr_new):
    """resampy's rate checks, and integer rates only (the exact output times are rationals of integers)."""
    if sr_orig <= 0:
        raise ValueError('Invalid sample rate: sr_orig={}'.format(sr_orig))
    if sr_new <= 0:
        raise ValueError('Invalid sample rate: sr_new={}'.format(sr_new))
    for sr in (sr_orig, sr_new):
        if int(sr) != sr:
            raise ValueError('sample rates must be whole numbers of Hz (got {})'.format(sr))
        if int(sr) > 1 << 24:
            raise ValueError('sample rate {} Hz is above 2^24 Hz'.format(sr))
    return int(sr_orig), int(sr_new)


def output_length(n, sr_orig, sr_new):
    """int(n * (float(sr_new) / sr_orig)), resampy's output length; ValueError (resampy's wording) when it is < 1."""
    sr_orig, sr_new = check_rates(sr_orig, sr_new)
    m = int(n * (float(sr_new) / sr_orig))
    if m < 1:
        raise ValueError('Input signal length={} is too small to resample from {}->{}'.format(n, sr_orig, sr_new))
    return m


def resample(x, sr_orig, sr_new, filter='kaiser_best', device=0):
    """resampy.resample for a 1-D signal, on the GPU: float32 in, float32 out of length int(len(x) * sr_new / sr_orig).
    Equal rates still filter, as resampy does (load_audio / read_audio skip the call then)."""
    from . import _lib
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError('x must be 1-D (got shape %s)' % (x.shape,))
    m = output_length(x.size, sr_orig, sr_new)
    win, num_table = get_filter(filter)
    return _lib.op_resample(x.astype(np.float32, copy=False), int(sr_orig), int(sr_new), win, num_table, 0, m, device=device)
