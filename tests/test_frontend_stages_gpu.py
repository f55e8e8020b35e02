"""The audio front-end's nine kernels alone against float64 (frontend_ref.py): frame_audio, frame_audio_folded, dft_pack_frames,
dft_twiddle, dft_fused, spec_to_features, sample_max, batch_max and db_sub_clamp, through the operators that run each on a caller's
input (include/l3hip.h l3_op_frontend_frames ... l3_op_db_normalize: every output NaN before the launch, a guard behind it).

What no other test sees: the DC and Nyquist bins of the 2048-point transform (the stock filterbank has weight 0 on both), empty
filters, the absolute scale of the power spectrum (everything else is compared after the maximum is subtracted), dft_fused's second
trip through its persistent loop, and framing geometries other than 48000 samples at hop 242.

Every call is made twice and must be bit-identical; every output must be finite.  Each criterion is printed as
`FESTAGE <kernel> <case> <criterion> <error / bound>` (<= 1 passes), each control as `FECONTROL <control> <case> <distance /
(CONTROL_MARGIN x bound)>` (> 1 passes); profiles/r30_frontend_stage_bounds.txt keeps the worst of each.

What they found: under amin the kernels returned -100.000015 dB (0xc2c80002) and -5.5262046 (one ulp under float(log(1e-12) / 5))
where the floors are -100 and -5.5262041 -- logf is within one ulp, not correctly rounded, and two more roundings follow.  Both
kernels now take the floor on the result (frontend.hip to_db / to_loglambda); the floor criteria below pass since.
"""
import functools

import numpy as np
import pytest

import frontend_ref as R
from l3embedding_amd import _lib
from oracle import l3_oracle as o

pytestmark = pytest.mark.gpu
F32, F64 = R.F32, R.F64


def _twice(fn, *args, **kw):
    """fn's result (an array or a tuple of arrays and Nones) after a second, bit-identical call; all finite."""
    a, b = fn(*args, **kw), fn(*args, **kw)
    ta, tb = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    for x, y in zip(ta, tb):
        assert (x is None and y is None) or R.bits_equal(x, y), 'two runs differ'
        assert x is None or np.isfinite(x).all(), 'not finite'
    return a


def _report(kernel, case, res):
    for line in R.lines(kernel, case, res):
        print(line)
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, (kernel, case, bad)


def _control(name, case, dist, bound):
    """A control: the altered reference must lie more than CONTROL_MARGIN bounds from what the GPU returned."""
    print('FECONTROL %s %s %.4g' % (name, case, dist / (R.CONTROL_MARGIN * bound)))
    assert dist > R.CONTROL_MARGIN * bound, (name, case, dist, bound)


@functools.lru_cache(maxsize=None)
def _tables():
    return _lib.frontend_tables()


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def test_tables(gpu_required):
    """win, b1, b2, tw within 2^-24 absolute of float64; the packed bands are the first-to-last-nonzero packing bit for bit."""
    t, ref = _twice(lambda: tuple(_tables()[k] for k in ('win', 'b1', 'b2', 'tw'))), R.tables64()
    _report('tables', '2048', {k: float(np.abs(a.astype(F64) - ref[k]).max() / R.TABLE_BOUND) for k, a in zip(('win', 'b1', 'b2', 'tw'), t)})
    for name, fb in (('stock256', R.stock_bank(256)), ('stock128', R.stock_bank(128)), ('bank70', R.bank70()), ('identity', R.identity_bank())):
        for arg in ((fb, None) if name.startswith('stock') else (fb,)):
            got = _lib.frontend_tables(fb.shape[1], arg)
            st, ln, of, w = R.pack_bands(fb)
            assert np.array_equal(got['mel_start'], st) and np.array_equal(got['mel_len'], ln) and np.array_equal(got['mel_off'], of), name
            assert R.bits_equal(got['melw'], w), name


# ---- framing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.FRAME_CASES, ids=[R.tag(c) for c in R.FRAME_CASES])
def test_framing_is_bit_exact(gpu_required, case):
    """frame_audio, frame_audio_folded and (2048) dft_pack_frames against NumPy float32: a copy, one add or subtract, one multiply by
    the returned window; zero padding (the audio carries a 1.0 offset), the padded columns of fe / fo exactly 0."""
    b, t, n_dft, hop, pad, nf = case
    x = R.audio_case(case)
    frames, fe, fo, a1 = _twice(_lib.op_frontend_frames, x, n_dft, hop, pad, nf)
    cfg = _lib.frontend_cfg(max(t, n_dft), n_dft, hop, False)
    want = R.frames_of(x, n_dft, hop, pad, nf)
    assert (want == 0).any() == (pad > 0 or (nf - 1) * hop - pad + n_dft > t)          # the case pads where it says it does
    we, wo = R.folded32(want, cfg['ke'], cfg['ko'])
    res = {'frames': 0.0 if R.bits_equal(frames, want) else np.inf, 'fe': 0.0 if R.bits_equal(fe, we) else np.inf,
           'fo': 0.0 if R.bits_equal(fo, wo) else np.inf,
           'pad_columns': 0.0 if not fe[..., n_dft // 2 + 1:].any() and not fo[..., n_dft // 2 - 1:].any() else np.inf}
    assert (a1 is not None) == (n_dft == 2048)
    if a1 is not None:
        res['a1'] = 0.0 if R.bits_equal(a1, R.packed32(want, _tables()['win'])) else np.inf
    _report('framing', R.tag(case), res)
    # the control: padding by the edge sample is a gross error wherever the case pads
    if (want == 0).any():
        assert np.abs(frames - R.frames_of(x, n_dft, hop, pad, nf, edge=True)).max() > 0.1


def test_framing_operator_refuses_what_the_kernels_cannot_index(gpu_required):
    x = np.zeros((1, 100), F32)
    for args in ((2048, 0, 0, 1), (2048, 16, -1, 1), (2048, 16, 0, 0), (100, 16, 0, 1), (2048, 1 << 30, 0, 4)):
        with pytest.raises(_lib.L3Error):
            _lib.op_frontend_frames(x, *args)
    with pytest.raises(_lib.L3Error):
        _lib.op_dft_fused(x, 16, 0, 1, 0)
    with pytest.raises(_lib.L3Error):
        _lib.op_spec_to_features('factored', np.zeros((1, 32, 64), F32), 1, 1, 2048)            # no Nyquist bins


# ---- dft_twiddle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('frames', R.TWIDDLE_FRAMES)
def test_dft_twiddle(gpu_required, frames):
    y = R.twiddle_input(frames)
    a2, nyq = _twice(_lib.op_dft_twiddle, y)
    _report('dft_twiddle', str(frames), R.twiddle_ratios(y, _tables()['tw'], a2, nyq))


# ---- spec_to_features --------------------------------------------------------------------------------------------------------------
def _spec_run(layout, rows, n_dft, n_mels, fb, re, im, **fl):
    cfg = _lib.frontend_cfg(n_dft, n_dft, 1, False)
    spec, nyq = R.spec_layout(layout, re, im, cfg)
    b = 3 if rows % 3 == 0 else 2 if rows % 2 == 0 else 1          # rows = b n_frames: several samples where rows allows
    out = _twice(_lib.op_spec_to_features, layout, spec, b, rows // b, n_dft, n_mels, fb, nyq, **fl)
    return R.rows_of(out)


_LINEAR = ([(lay, rows, 512, 0, None) for lay in ('unfolded', 'folded') for rows in R.SPEC_ROWS] +
           [(lay, rows, 2048, 128, 'stock128') for lay in ('unfolded', 'folded') for rows in R.SPEC_ROWS] +
           [('factored', 3, 2048, 256, 'stock256'), ('factored', 6, 2048, 70, 'bank70'), ('factored', 1, 2048, 1025, 'identity')])


def _bank(name):
    return None if name is None else {'stock128': lambda: R.stock_bank(128), 'stock256': lambda: R.stock_bank(256), 'bank70': R.bank70,
                                      'identity': R.identity_bank}[name]()


@pytest.mark.parametrize('layout,rows,n_dft,n_mels,bank', _LINEAR, ids=['%s-%d-%d-%s' % (p[0], p[1], p[2], p[4]) for p in _LINEAR])
def test_spec_to_features_linear(gpu_required, layout, rows, n_dft, n_mels, bank):
    """Flags off: (mel_len + 3) 2^-24 relative per element, an empty filter exactly 0; 257 outputs per row at 512 (thread 0 takes a
    second one), the folded im rows at (rows + row) nc, and the 70-filter bank's taps on bins 0 and 1024."""
    fb = _bank(bank)
    re, im = R.spec_input(rows, n_dft)
    got = _spec_run(layout, rows, n_dft, n_mels, None if bank and bank.startswith('stock') and n_mels == 256 else fb, re, im)
    _report('spec_to_features', '%s-%d-%d-%s' % (layout, rows, n_dft, bank), {'linear': R.linear_ratio(got, re, im, fb)})
    if bank == 'bank70':          # the controls: the DC or the Nyquist bin dropped, the bins mis-ordered
        ref = R.power_of(re, im) @ fb.astype(F64)
        for cut, q in ((0, 0), (1024, 1)):
            pw = R.power_of(re, im)
            pw[:, cut] = 0
            alt = pw @ fb.astype(F64)
            _control('bin_%d_zero' % cut, 'spec_to_features-bank70', np.abs(got[:, q] - alt[:, q]).max(), (fb.shape[0] + 3) * R.U24 * ref[:, q].max())


_FLAGGED = [('factored', 2048, 256, 'stock256'), ('unfolded', 512, 0, None)]


@pytest.mark.parametrize('fl', R.FLAG_SETS, ids=[R.flag_tag(f) for f in R.FLAG_SETS])
@pytest.mark.parametrize('layout,n_dft,n_mels,bank', _FLAGGED, ids=['%s-%d' % (p[0], p[1]) for p in _FLAGGED])
def test_spec_to_features_flags(gpu_required, layout, n_dft, n_mels, bank, fl):
    """sqrt_out, db, loglambda, sqrt_out + db: at most K_D32 times further from float64 than the float32 NumPy restatement (floor: one
    fp32 ulp of the result); values under amin give exactly the float32 floor (-100 dB, log(1e-12) / 5); amin = 1e-12 is rejected."""
    fb = _bank(bank)
    re, im = R.spec_input(8, n_dft, quiet_rows=4)
    got = _spec_run(layout, 8, n_dft, n_mels, fb, re, im, **fl)
    res, d, d32 = R.flag_ratios(got, re, im, fb, fl)
    print('FESTAGE spec_to_features %s-%d-%s d %.3g d32 %.3g' % (layout, n_dft, R.flag_tag(fl), d, d32))
    _report('spec_to_features', '%s-%d-%s' % (layout, n_dft, R.flag_tag(fl)), res)
    if fl == dict(db=True):
        alt = R.features(R.power_of(re, im), fb, db=True, amin=1e-12)
        _control('amin_1e-12', '%s-%d-db' % (layout, n_dft), R.d_of(got, alt), R.K_D32 * max(d32, R.ULP32))


# ---- dft_fused ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep():
    """The tone sweep through dft_fused with the identity bank, and its float64 reference: (got, ref), both (1025, 1025)."""
    x = R.tone_sweep()
    got = R.rows_of(_twice(_lib.op_dft_fused, x, 16, 0, 1, R.NB, R.identity_bank()))
    return R._ro(got, R.fused64(x, 16, 0, 1, _tables()['win']))


def test_dft_fused_tone_sweep(gpu_required):
    """One tone per bin, DC and Nyquist included: every row within LIN_BOUND of float64 relative to its peak, the peak in the right
    bin, and the peak power itself within the bound -- which pins the absolute scale.  (The float32 GEMM restatement in NumPy: 1.07e-6.)"""
    got, ref = _sweep()
    d = R.row_d(got, ref)
    k = np.arange(R.NB)
    peak = float((np.abs(got[k, k].astype(F64) - ref[k, k]) / ref[k, k]).max())
    print('FESTAGE dft_fused tone_sweep d %.3g' % d)
    assert np.array_equal(got.argmax(1), k)
    _report('dft_fused', 'tone_sweep', {'lin': d / R.LIN_BOUND, 'peak': peak / R.LIN_BOUND,
                                        'dc': R.row_d(got[:1], ref[:1]) / R.LIN_BOUND, 'nyquist': R.row_d(got[1024:], ref[1024:]) / R.LIN_BOUND})


def test_dft_fused_controls_on_the_tone_sweep(gpu_required):
    """Nyquist bin 0 (row 1024), DC bin 0 (row 0), the bins ordered k2 + 32 k1, the power doubled: each more than CONTROL_MARGIN
    bounds from what the GPU returned."""
    got, ref = _sweep()
    alt = ref.copy()
    alt[:, 1024] = 0
    _control('nyquist_zero', 'tone_sweep-row1024', R.row_d(got[1024:], alt[1024:]), R.LIN_BOUND)
    alt = ref.copy()
    alt[:, 0] = 0
    _control('dc_zero', 'tone_sweep-row0', R.row_d(got[:1], alt[:1]), R.LIN_BOUND)
    _control('bins_k2+32k1', 'tone_sweep', R.row_d(got, R.fused64(R.tone_sweep(), 16, 0, 1, _tables()['win'], order='k2+32k1')), R.LIN_BOUND)
    _control('power_x2', 'tone_sweep', R.row_d(got, 2 * ref), R.LIN_BOUND)


@pytest.mark.parametrize('case', R.EDGE_CASES, ids=[R.tag(c) for c in R.EDGE_CASES])
def test_dft_fused_edges(gpu_required, case):
    """The clamped-index loads: frames with left padding, with both, and of a single sample, on noise plus a 1.0 offset; padding by
    the edge sample is rejected."""
    x, geo = R.audio_case(case), case[3:]
    got = R.rows_of(_twice(_lib.op_dft_fused, x, *geo, R.NB, R.identity_bank()))
    win = _tables()['win']
    _report('dft_fused', 'edges-' + R.tag(case), {'lin': R.row_d(got, R.fused64(x, *geo, win)) / R.LIN_BOUND})
    _control('edge_pad', 'edges-' + R.tag(case), R.row_d(got, R.fused64(x, *geo, win, edge=True)), R.LIN_BOUND)


@pytest.mark.parametrize('rows', (1, 3, 13))
def test_dft_fused_ragged_workgroups(gpu_required, rows):
    """1, 3 and 13 rows: workgroups whose last waves have no frame."""
    x = (R.rng_of(17, rows).standard_normal((1, R.N + 16 * (rows - 1))) * 0.25).astype(F32)
    got = R.rows_of(_twice(_lib.op_dft_fused, x, 16, 0, rows, R.NB, R.identity_bank()))
    _report('dft_fused', 'ragged-%d' % rows, {'lin': R.row_d(got, R.fused64(x, 16, 0, rows, _tables()['win'])) / R.LIN_BOUND})


@pytest.mark.parametrize('bank', ('stock256', 'stock128', 'bank70'))
def test_dft_fused_mel_banks(gpu_required, bank):
    """The stock banks and the 70-filter test bank on noise: LIN_BOUND per row; empty filters exactly 0, exactly -100 under db."""
    case = R.FRAME_CASES[0]
    fb = _bank(bank)
    x, geo = R.audio_case(case), case[3:]
    arg = None if bank.startswith('stock') else fb
    got = R.rows_of(_twice(_lib.op_dft_fused, x, *geo, fb.shape[1], arg))
    ref = R.fused64(x, *geo, _tables()['win']) @ fb.astype(F64)
    empty = R.pack_bands(fb)[1] == 0
    assert empty.sum() == {'stock256': 2, 'stock128': 0, 'bank70': 1}[bank]
    db = R.rows_of(_twice(_lib.op_dft_fused, x, *geo, fb.shape[1], arg, db=True))
    _report('dft_fused', bank, {'lin': R.row_d(got, ref) / R.LIN_BOUND, 'empty': 0.0 if np.all(got[:, empty] == 0) else np.inf,
                                'empty_db': 0.0 if np.all(db[:, empty] == R.DB_FLOOR32) else np.inf})


def test_dft_fused_beyond_one_trip(gpu_required):
    """More rows than the persistent grid has waves (8 per CU): samples 0 and 2 hold the same audio and their rows fall in different
    trips of the loop, which re-uses each wave's LDS region -- bit-identical, and every row within the bound."""
    cus = _cus()
    nf = -(-(2 * 8 * cus + 5) // 3)
    rows = 3 * nf
    assert rows >= 2 * 8 * cus + 5 and 2 * nf > 8 * cus              # all of sample 2 lies beyond the first trip
    t = R.N + 16 * (nf - 1)
    x = (R.rng_of(19, cus).standard_normal((3, t)) * 0.25 + 0.1).astype(F32)
    x[2] = x[0]
    got = _twice(_lib.op_dft_fused, x, 16, 0, nf, R.NB, R.identity_bank())
    assert R.bits_equal(got[0], got[2]) and not R.bits_equal(got[0], got[1])
    ref = R.fused64(x, 16, 0, nf, _tables()['win'])
    _report('dft_fused', 'trips-%dcu-%drows' % (cus, rows), {'lin': R.row_d(R.rows_of(got), ref) / R.LIN_BOUND})


# ---- db_normalize ------------------------------------------------------------------------------------------------------------------
_DB = [(c, 'plain') for c in R.DB_CASES] + [((3, 255), 'floor_row'), ((3, 255), 'last_max'), ((300, 3500), 'last_max')]


@pytest.mark.parametrize('scope', ('sample', 'batch'))
@pytest.mark.parametrize('case,kind', _DB, ids=['%s-%s' % (R.tag(c), k) for c, k in _DB])
def test_db_normalize_is_bit_exact(gpu_required, case, kind, scope):
    """sample_max, batch_max and db_sub_clamp against NumPy float32 maximum(x - max, -80), both scopes."""
    x = R.db_input(*case, kind)
    got = _twice(_lib.op_db_normalize, x, scope)
    want = R.db_normalize32(x, scope)
    _report('db_normalize', '%s-%s-%s' % (R.tag(case), kind, scope), {'exact': 0.0 if R.bits_equal(got, want) else np.inf})
    assert got.max() == 0.0 and got.min() >= -80.0
    if kind == 'floor_row':
        assert np.all(got[min(1, case[0] - 1)] == (0.0 if scope == 'sample' else -80.0))


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
def test_engine_follows_a_filterbank_with_weight_on_dc_and_nyquist(gpu_required, monkeypatch):
    """cnn_L3_melspec2 with freq2mel replaced by a bank whose loudest outputs are a tap on bin 0 and a band ending on bin 1024, on an
    alternating signal with an offset: the fused kernel, the two-GEMM factored chain and the full GEMM all follow the oracle with
    the same constants within test_frontend's tone bound (2e-5 of the peak, linear domain)."""
    mt, kind = 'cnn_L3_melspec2', 'melspec2'
    v = o.synthetic_batch(1, seed=9)[0]
    a = R.edge_signal()[None, None, :]
    consts = o.frontend_constants(kind)
    consts['freq2mel'] = R.edge_bank()
    ref = o.frontend_forward(kind, a, consts, 'sample', F64)
    stock = o.frontend_forward(kind, a, None, 'sample', F64)
    lin = lambda x: 10 ** (np.asarray(x, F64) / 10)
    assert np.abs(lin(ref) - lin(stock)).max() > 0.5                 # the edit is visible at all: the peak moved to the edited filters
    assert {int(q) for q in np.argsort(ref[0, :, :, 0].max(1))[-2:]} == {0, 255}
    res, got = {}, {}
    for mode in ('1', '2', '0'):
        monkeypatch.setenv('L3_DFT_FACTORED', mode)
        eng = _lib.Engine(mt, 1, seed=0)
        name = [n for n, _, _ in eng.param_table() if n.endswith('/freq2mel')][0]
        eng.set_param(name, consts['freq2mel'])
        eng.forward(v, a, training=False)
        got[mode] = eng.activation('audio_model/frontend').reshape(ref.shape)
        eng.close()
        assert np.isfinite(got[mode]).all()
        res['mode%s' % mode] = float(np.abs(lin(got[mode]) - lin(ref)).max() / R.ENGINE_BOUND)
        for q in (0, 255):
            res['mode%s-filter%d' % (mode, q)] = float(np.abs(lin(got[mode][0, q]) - lin(ref[0, q])).max() / R.ENGINE_BOUND)
    res['fused-vs-gemm'] = float(np.abs(lin(got['1']) - lin(got['0'])).max() / R.ENGINE_BOUND)
    _report('engine', 'edge_bank', res)
    assert not np.array_equal(got['1'], got['0'])
