"""The yardstick of test_frontend_stages_gpu.py checked on the CPU (frontend_ref.py): the staged float64 transform is the DFT, the
reference equals the oracle's front-end before its dB step, the band-packed mel product equals the dense one, the library's framing
geometry and tables are the oracle's, and every control differs from the reference by more than its margin."""
import numpy as np
import pytest

import frontend_ref as R
from l3embedding_amd import _lib
from oracle import l3_oracle as o

F32, F64 = R.F32, R.F64
BANKS = {'stock256': lambda: R.stock_bank(256), 'stock128': lambda: R.stock_bank(128), 'bank70': R.bank70, 'identity': R.identity_bank,
         'edge': R.edge_bank}


def _win32():
    return _lib.frontend_tables()['win']


def test_staged_reference_is_the_dft_of_the_windowed_frames():
    """<= 1e-12 of the largest bin, on noise frames with padding and on the tone sweep; the mis-ordered control is not."""
    case = R.FRAME_CASES[0]
    fr = R.frames_of(R.audio_case(case), *case[2:]).astype(F64).reshape(-1, R.N)
    for xw in (fr * R.window64(R.N), R.tone_sweep().astype(F64) * R.window64(R.N)):
        ref = np.fft.rfft(xw, axis=1)
        st = R.staged_dft(xw)
        assert np.abs(st['X'] - ref).max() <= 1e-12 * np.abs(ref).max()
        assert np.abs(st['nyq'] - ref[:, R.N // 2].real).max() <= 1e-12 * np.abs(ref).max()
        assert np.abs(R.staged_dft(xw, 'k2+32k1')['X'] - ref).max() > 0.1 * np.abs(ref).max()


def test_library_tables_and_geometry_are_the_references():
    """win, b1, b2, tw within 2^-24 of float64; the window is the one kapre's kernels carry; the packed bands of every test bank are
    the first-to-last-nonzero packing bit for bit; frontend_cfg's framing is oracle.tf_same_pad / frame_signal."""
    t, ref = _lib.frontend_tables(), R.tables64()
    for k in ('win', 'b1', 'b2', 'tw'):
        assert t[k].shape == ref[k].shape and np.abs(t[k].astype(F64) - ref[k]).max() <= R.TABLE_BOUND, k
    real = o.stft_kernels(R.N)[0]
    assert R.bits_equal(t['win'], real[:, 0])                   # bin 0 of the real kernels is the window itself
    assert R.bits_equal(_lib.frontend_tables(256)['melw'], R.pack_bands(R.stock_bank(256))[3])        # NULL = the stock bank
    for name, make in BANKS.items():
        fb = make()
        got = _lib.frontend_tables(fb.shape[1], fb)
        st, ln, of, w = R.pack_bands(fb)
        assert np.array_equal(got['mel_start'], st) and np.array_equal(got['mel_len'], ln) and np.array_equal(got['mel_off'], of), name
        assert R.bits_equal(got['melw'], w), name
    assert (R.pack_bands(R.stock_bank(256))[1] == 0).sum() == 2          # the stock bank's two empty filters
    assert tuple(np.flatnonzero(R.pack_bands(R.bank70())[1] == 0)) == R.BANK70_EMPTY
    for tt, n_dft, hop, same in R.CFG_CASES:
        cfg = _lib.frontend_cfg(tt, n_dft, hop, same)
        x = R.rng_of(tt, n_dft, hop).standard_normal((2, tt)).astype(F32)
        want = o.frame_signal(x[:, None, :], n_dft, hop, 'same' if same else 'valid')
        assert cfg['n_frames'] == want.shape[1], (tt, n_dft, hop, same)
        if same:
            assert (cfg['n_frames'], cfg['pad_left']) == o.tf_same_pad(tt, n_dft, hop)[:2]
        else:
            assert cfg['pad_left'] == 0
        assert np.array_equal(R.frames_of(x, n_dft, hop, cfg['pad_left'], cfg['n_frames']), want)
        assert cfg['n_freq'] == n_dft // 2 + 1 and cfg['ncols_pad'] % 32 == 0 and cfg['ncols_pad'] >= 2 * cfg['n_freq']
        assert cfg['ke'] >= n_dft // 2 + 1 and cfg['ko'] >= n_dft // 2 - 1 and cfg['nc'] >= cfg['n_freq'] and cfg['N1'] * cfg['N2'] == n_dft
    # every FRAME_CASES geometry that is a 'same' or 'valid' framing is in CFG_CASES with the same frames and padding
    for b, tt, n_dft, hop, pad, nf in R.FRAME_CASES:
        for same in (True, False):
            if (tt, n_dft, hop, same) in R.CFG_CASES:
                cfg = _lib.frontend_cfg(tt, n_dft, hop, same)
                assert cfg['n_frames'] >= nf and (not same or cfg['pad_left'] >= pad)


@pytest.mark.parametrize('kind,n_mels', [('melspec2', 256), ('melspec1', 128)])
def test_reference_equals_the_oracle_before_its_db_step(kind, n_mels, monkeypatch):
    """oracle.frontend_forward with the dB step (and the square root) switched off is the mel power: the staged reference times the
    stock bank equals it, up to what the oracle's float32-rounded kernels allow -- every kernel entry is within 2^-24 of its value
    relative, so a bin is off by delta <= sqrt(2) 2^-24 sum |x| win and its power by 2 |X| delta + delta^2."""
    monkeypatch.setitem(o.FRONTENDS, kind, dict(o.FRONTENDS[kind], db=False, power=2.0))
    a = o.synthetic_batch(1, seed=9)[1]
    want = o.frontend_forward(kind, a, None, 'sample', F64)[0, :, :, 0].T               # (frames, mels)
    cfg = _lib.frontend_cfg(48000, R.N, 242, True, n_mels)
    fr = R.frames_of(a[:, 0, :], R.N, 242, cfg['pad_left'], cfg['n_frames']).astype(F64).reshape(-1, R.N)
    win = _win32().astype(F64)
    X = R.staged_dft(fr * win)['X']
    fb = R.stock_bank(n_mels).astype(F64)
    got = R.features(X.real ** 2 + X.imag ** 2, fb)
    delta = np.sqrt(2) * R.U24 * (np.abs(fr) * win).sum(1, keepdims=True)
    bound = (2 * np.abs(X) * delta + delta ** 2) @ fb
    assert got.shape == want.shape and R._ratio(np.abs(got - want), bound + 1e-13 * np.abs(want).max()) <= 1.0
    assert np.abs(got - want).max() <= 1e-6 * want.max()


@pytest.mark.parametrize('name', sorted(BANKS))
def test_band_packed_mel_product_equals_the_dense_one(name):
    fb = BANKS[name]().astype(F64)
    re, im = R.spec_input(5, R.N, seed=1)
    pw = R.power_of(re, im)
    dense, banded = pw @ fb, R.banded_product(pw, R.pack_bands(fb))
    assert np.abs(dense - banded).max() <= 1e-13 * dense.max()
    empty = R.pack_bands(fb)[1] == 0
    assert np.all(banded[:, empty] == 0) and np.all(dense[:, empty] == 0)


def test_spec_layouts_hold_the_same_spectrum():
    """spec_layout's three layouts read back as spec_to_features reads them give the power spectrum they were built from."""
    for n_dft in (512, R.N):
        cfg = _lib.frontend_cfg(n_dft, n_dft, 1, False)
        rows, nb = 3, n_dft // 2 + 1
        re, im = R.spec_input(rows, n_dft)
        pw = R.power_of(re, im, F32)
        s, _ = R.spec_layout('unfolded', re, im, cfg)
        assert np.array_equal(s[:, :nb] ** 2 + s[:, nb:2 * nb] ** 2, pw) and not s[:, 2 * nb:].any()
        s, _ = R.spec_layout('folded', re, im, cfg)
        assert all(np.array_equal(s[r, :nb] ** 2 + s[rows + r, :nb] ** 2, pw[r]) for r in range(rows))
    s, nyq = R.spec_layout('factored', re, im, cfg)
    for k in (0, 1, 31, 32, 33, 1023):
        k1, k2 = k % 32, k // 32
        assert np.array_equal(s[:, k1, k2] ** 2 + s[:, k1, 32 + k2] ** 2, pw[:, k])
    assert np.array_equal(nyq * nyq, pw[:, 1024])


def test_every_control_differs_by_more_than_its_margin():
    """The altered references, on the cases named for them, lie more than (CONTROL_MARGIN + 1) bounds from the true one: a GPU
    result within the bound of the true reference is then more than CONTROL_MARGIN bounds from the control."""
    need = (R.CONTROL_MARGIN + 1) * R.LIN_BOUND
    win = _win32()
    x = R.tone_sweep()
    ref = R.fused64(x, 16, 0, 1, win)
    assert np.array_equal(ref.argmax(1), np.arange(R.NB))
    alt = ref.copy()
    alt[:, R.N // 2] = 0
    assert R.row_d(ref[1024:], alt[1024:]) > need
    alt = ref.copy()
    alt[:, 0] = 0
    assert R.row_d(ref[:1], alt[:1]) > need
    assert R.row_d(ref, R.fused64(x, 16, 0, 1, win, order='k2+32k1')) > need
    assert R.row_d(ref, 2 * ref) > need
    for case in R.EDGE_CASES:
        a, geo = R.audio_case(case), case[3:]
        assert R.row_d(R.fused64(a, *geo, win), R.fused64(a, *geo, win, edge=True)) > need, case
    # amin = 1e-12 under the db flag on a quiet input: against the K_D32 rule's bound of that case
    re, im = R.spec_input(4, R.N, quiet_rows=2)
    pw, fb = R.power_of(re, im), R.stock_bank(256)
    ref, alt = R.features(pw, fb, db=True), R.features(pw, fb, db=True, amin=1e-12)
    d32 = R.d_of(R.features(R.power_of(re, im, F32), fb, db=True, dtype=F32), ref)
    assert R.d_of(ref, alt) > (R.CONTROL_MARGIN + 1) * R.K_D32 * max(d32, R.ULP32)
    # the engine-level case: the two edited filters are the loudest outputs, and dropping either edge bin is visible
    a = R.edge_signal()
    cfg = _lib.frontend_cfg(48000, R.N, 242, True, 256)
    p = R.fused64(a[None], 242, cfg['pad_left'], cfg['n_frames'], win)
    out = np.sqrt(p @ R.edge_bank().astype(F64))
    top = set(np.argsort(out.max(0))[-2:])
    assert top == {0, 255}
    for k, q in ((0, 0), (1024, 255)):
        cut = p.copy()
        cut[:, k] = 0
        alt = np.sqrt(cut @ R.edge_bank().astype(F64))
        assert np.abs(alt - out).max() > (R.CONTROL_MARGIN + 1) * R.ENGINE_BOUND * out.max()
