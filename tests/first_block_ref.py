"""The yardstick of the first block's backward (test_first_block_gpu.py, test_first_block_host.py): seeded inputs, the float64
chain and closed form, an fp32 NumPy restatement of the kernels' formulas with named mutants, and the comparators.

The block: x (N, H, W, C), C = 1 or 3  ->  BatchNorm(gamma_in, beta_in)  ->  3x3 'same' convolution w, bias to 64 filters = y  ->
BatchNorm(gamma2, beta2) [-> ReLU]  ->  a, with dA = dL/da given.  The engine never computes the first layer's data gradient nor the
input BatchNorm's backward reduction; from ONE weight gradient over the augmented input [x^, 1] (gaug (9, C + 1, 64): G = the x^ rows,
S = the ones row) it takes dW = gamma G + beta S, dgamma = sum W G, dbeta = sum W S and the bias gradient S[centre tap]
(elementwise.hip first_conv_grads), and in the deferred forms the weight-gradient kernel forms dY = cA mask(dA) + (cB y + cC) itself
from the second BatchNorm's backward coefficients (conv_first.hip, FirstWgFuse).

  * case(): the inputs.  y is an INPUT of the operator: the float64 convolution of the normalised input plus a bias of order one
    (so that cB y + cC really cancels), stored as fp32 or rounded to bfloat16.  dA = 1e-3 N(0,1), and 0 wherever the float64
    pre-activation of the second BatchNorm lies within MASK_MARGIN of 0: the recomputed ReLU mask cannot matter there.
  * chain(): the straightforward float64 backward from the STORED y and dA -- second BatchNorm's backward, the convolution's weight,
    bias AND data gradient, the input BatchNorm's backward -- from oracle.l3_oracle's unfused ops.  closed(): the engine's closed
    form in float64.  forward_loss(): L = sum dA act(BN2(conv(BN_in(x)))), for finite differences.
  * emulate(): the kernels' formulas in NumPy -- fp32 element arithmetic, fp32 partial sums of the weight gradient, float64 column
    sums where the kernels have them (bn_storage_ref's plain_f32 and _bwd_coeffs) -- with the named MUTANTS.
  * stage_ratios() / e2e_ratios(): every criterion as error / bound (<= 1 passes).  Stage by stage each result is held against
    float64 arithmetic on the fp32 tensors the operator returned for the stage before; TOL = 3e-6 of the sum of the terms' magnitudes
    (epilogue_stats_ref.TOL) is the only tolerance besides the roundings counted below.
"""
import functools

import numpy as np

from oracle import l3_oracle as o
import bn_storage_ref as bs
import epilogue_stats_ref as es

TOL = es.TOL
MASK_MARGIN = es.MASK_MARGIN
F32, F64 = np.float32, np.float64
EPS32 = F32(1e-3)
EPS64 = F64(EPS32)
CO = 64
U24 = 2.0 ** -24

# ---- the cases ---------------------------------------------------------------------------------------------------------------------
# (N, H, W), each with C = 1 and C = 3.  Units = N H ceil(W / 4) 4-pixel units; <= 65 536 of them run 16 (or fewer) per wave.
#   (1, 1, 3)    one unit holding 3 of 4 pixels; 4 waves of which 3 are empty
#   (1, 3, 2)    W < 4: one unit per row; one empty wave
#   (2, 9, 7)    2 units per row, the second with 3 pixels; 36 units = 4 waves x 9: ranges start mid-row and cross the image boundary
#   (3, 6, 10)   54 units, 14 per wave (2 dead slots at DEPTH 3 and 4), the last wave 12
#   (1, 5, 199)  the audio width, W mod 4 = 3; 250 units over 16 waves, the last with 10
#   (2, 64, 50)  1 664 units = 104 full waves, 26 workgroup partials for the reduce
SMALL_SHAPES = [(1, 1, 3), (1, 3, 2), (2, 9, 7), (3, 6, 10), (1, 5, 199), (2, 64, 50)]
SMALL_CASES = [(s, c) for s in SMALL_SHAPES for c in (1, 3)]
# beyond the 4096-wave cap (65 536 units): 76 800 / 75 264 units, 19 per wave, 1024 partials, short and empty waves at the end
CAPPED_CASES = [((6, 256, 199), 1), ((6, 224, 224), 3)]
# (form, relu): all five instantiations of conv_first_wgrad_kernel per channel count
SMALL_FORMS = [('explicit', 1), ('deferred', 0), ('deferred', 1), ('deferred_bf16', 0), ('deferred_bf16', 1)]
CAPPED_FORMS = [('deferred', 1), ('deferred_bf16', 1)]
E2E_MIN_PIXELS = 100                 # smaller cases normalise over 3 or 6 rows: stage by stage only
BITE_SHAPES = [(2, 9, 7), (3, 6, 10), (1, 5, 199)]          # where the propagated dgamma_in / dbeta_in bound must stay under BITE
BITE = 0.10
GRADS_SHAPES = [(9, 1, 64), (9, 3, 64), (25, 3, 10), (1, 2, 300)]      # (taps, C, Co) of first_conv_grads alone
# the seed of a case, where 0 would leave dgamma_in / dbeta_in so small by chance that the propagated bound exceeds BITE of the
# tensor's largest entry (test_first_block_host.py checks every BITE_SHAPES case): none needs another -- the worst is 5.1 %
SEEDS = {}


def tag(shape, c):
    return 'x'.join(map(str, shape + (c,)))


def instantiation(c, form, relu):
    return 'wgrad<%d,%d,%d>' % (c + 1, {'explicit': 0, 'deferred': 1, 'deferred_bf16': 2}[form], relu if form != 'explicit' else 0)


# ---- float64 pieces ----------------------------------------------------------------------------------------------------------------
def _cols(xa):
    """im2col of xa (N, H, W, CA) for 3x3 'same', zero padded: (N H W, 9, CA)."""
    n, h, w, ca = xa.shape
    xp = np.pad(xa, ((0, 0), (1, 1), (1, 1), (0, 0)))
    return np.stack([xp[:, i:i + h, j:j + w].reshape(-1, ca) for i in range(3) for j in range(3)], axis=1)


def wgrad64(xa, dy):
    """gaug[tap][ci][co] = sum_p xa[p + tap][ci] dy[p][co] in float64, all taps in one pass: (9, CA, Co)."""
    ca = xa.shape[-1]
    cols = _cols(np.asarray(xa, F64)).reshape(-1, 9 * ca)
    return (cols.T @ np.asarray(dy, F64).reshape(-1, dy.shape[-1])).reshape(9, ca, -1)


def bn2_pre(y64, scale, shift):
    return y64 * np.asarray(scale, F64) + np.asarray(shift, F64)


def closed_from_gaug(gaug, w, gamma, beta):
    """first_conv_grads in float64: gaug (taps, C + 1, Co), w (taps, C, Co) -> dw, dgamma, dbeta, dbias."""
    gaug, w = np.asarray(gaug, F64), np.asarray(w, F64)
    c = w.shape[1]
    g, s = gaug[:, :c], gaug[:, c]
    gm, bt = np.asarray(gamma, F64)[None, :, None], np.asarray(beta, F64)[None, :, None]
    return gm * g + bt * s[:, None], (w * g).sum((0, 2)), (w * s[:, None]).sum((0, 2)), s[gaug.shape[0] // 2]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)          # (a capped case holds 0.3 GB: the cache keeps the few in use)
def case(shape, c, bf16=False):
    """The inputs of one case as a read-only dict: x, gamma_in, beta_in, w, bias, y (stored form: fp32, or bfloat16-valued), y_f32
    (before the bfloat16 rounding), gamma2, beta2, dA, and `zeroed`, the share of dA set to 0 under MASK_MARGIN."""
    n, h, wd = shape
    rng = np.random.default_rng([20240607, n, h, wd, c, SEEDS.get((shape, c), 0)])
    x = rng.standard_normal((n, h, wd, c), dtype=F32) * F32(1.5) + F32(0.3)
    gamma_in = (1 + 0.1 * rng.standard_normal(c)).astype(F32)
    beta_in = (0.1 * rng.standard_normal(c)).astype(F32)
    w = (rng.standard_normal((3, 3, c, CO)) * np.sqrt(2.0 / (9 * c))).astype(F32)
    bias = rng.standard_normal(CO).astype(F32)
    gamma2 = (1 + 0.1 * rng.standard_normal(CO)).astype(F32)
    beta2 = (0.1 * rng.standard_normal(CO)).astype(F32)
    dA = rng.standard_normal((n, h, wd, CO), dtype=F32) * F32(1e-3)
    u = o.bn_fwd(x.astype(F64), gamma_in.astype(F64), beta_in.astype(F64), None, None, True)[0]
    y_f32 = o.conv2d_fwd(u, w.astype(F64), bias.astype(F64), 'same').astype(F32)
    y = o.bf16_round(y_f32) if bf16 else y_f32
    if bf16:
        dA = o.bf16_round(dA)
    pre = o.bn_fwd(y.astype(F64), gamma2.astype(F64), beta2.astype(F64), None, None, True)[0]
    near = np.abs(pre) < MASK_MARGIN
    dA[near] = 0
    zeroed = float(near.mean())
    assert zeroed <= 0.01, (shape, c, zeroed)
    out = dict(x=x, gamma_in=gamma_in, beta_in=beta_in, w=w, bias=bias, y=y, y_f32=y_f32, gamma2=gamma2, beta2=beta2, dA=dA)
    for a in out.values():
        a.setflags(write=False)
    out.update(zeroed=zeroed, shape=shape, c=c, bf16=bf16)
    return out


def op_args(cs):
    return [cs[k] for k in ('x', 'gamma_in', 'beta_in', 'w', 'y', 'gamma2', 'beta2', 'dA')]


# ---- the float64 chain, the closed form, the loss ----------------------------------------------------------------------------------
def _p64(cs, *names):
    return [np.asarray(cs[k], F64) for k in names]


def chain(cs, relu, y=None):
    """The straightforward float64 backward from x, the stored y (or the given one) and dA: dict of dY, dgamma2, dbeta2, T (the
    magnitudes |cA mask(dA)| + |cB y| + |cC| of dY's terms), xhat, dw, dbias, dx_first (the first layer's data gradient), dgamma_in,
    dbeta_in."""
    x, gi, bi, w, g2, b2, dA = _p64(cs, 'x', 'gamma_in', 'beta_in', 'w', 'gamma2', 'beta2', 'dA')
    y = np.asarray(cs['y'] if y is None else y, F64)
    u, cin = o.bn_fwd(x, gi, bi, None, None, True)
    pre, c2 = o.bn_fwd(y, g2, b2, None, None, True)
    dz = np.where(pre > 0, dA, 0.0) if relu else dA
    dY, dg2, db2 = o.bn_bwd(dz, g2, c2, True)
    rows = dz.size // CO
    gr = g2 * c2[1]
    cA, cB, cC = gr, -gr * c2[1] * dg2 / rows, gr * (-db2 / rows + c2[2] * c2[1] * dg2 / rows)
    out = dict(dY=dY, dgamma2=dg2, dbeta2=db2, T=np.abs(cA * dz) + np.abs(cB * y) + np.abs(cC), xhat=cin[0].reshape(x.shape),
               cA=cA, cB=cB, cC=cC)
    dx, dw, db = o.conv2d_bwd(u, w, dY, 'same')
    _, dgi, dbi = o.bn_bwd(dx, gi, cin, True)
    out.update(dw=dw, dbias=db, dx_first=dx, dgamma_in=dgi, dbeta_in=dbi)
    return out


def closed(cs, ch):
    """The engine's closed form in float64 from the chain's x^ and dY: gaug, dw, dbias, dgamma_in, dbeta_in."""
    xa = np.concatenate([ch['xhat'], np.ones(ch['xhat'].shape[:3] + (1,))], axis=-1)
    gaug = wgrad64(xa, ch['dY'])
    c = cs['c']
    dw, dg, db, dbias = closed_from_gaug(gaug, np.asarray(cs['w'], F64).reshape(9, c, CO), cs['gamma_in'], cs['beta_in'])
    return dict(gaug=gaug, dw=dw.reshape(3, 3, c, CO), dbias=dbias, dgamma_in=dg, dbeta_in=db)


def forward_loss(cs, relu, gamma_in=None, beta_in=None, w=None):
    """L = sum dA act(BN2(conv(BN_in(x)) + bias)) in float64, every stage recomputed (batch statistics included)."""
    x, gi, bi, w0, b, g2, b2, dA = _p64(cs, 'x', 'gamma_in', 'beta_in', 'w', 'bias', 'gamma2', 'beta2', 'dA')
    u = o.bn_fwd(x, gi if gamma_in is None else gamma_in, bi if beta_in is None else beta_in, None, None, True)[0]
    y = o.conv2d_fwd(u, w0 if w is None else w, b, 'same')
    a = o.bn_fwd(y, g2, b2, None, None, True)[0]
    return float((dA * (np.maximum(a, 0) if relu else a)).sum()), y


# ---- the kernels' formulas in fp32 NumPy, with mutants -----------------------------------------------------------------------------
MUTANTS = {
    # name: (the criteria of which one must reject it, what it is)
    'taps_transposed': (('gaug',), 'the taps of gaug transposed (kh <-> kw)'),
    's_next_tap': (('dw', 'dbeta_in', 'e2e:dw', 'e2e:dbeta_in'), "S taken from G's neighbouring tap"),
    'gamma_beta_swapped': (('dw', 'e2e:dw'), 'gamma and beta exchanged in dW'),
    'dgamma_next_channel': (('dgamma_in', 'e2e:dgamma_in'), 'dgamma summed with the filter of the next input channel (C = 3)'),
    'bias_tap0': (('dbias', 'e2e:dbias'), 'the bias gradient read from tap 0'),
    'unit_dropped': (('gaug',), 'one 4-pixel unit dropped at a wave boundary'),
    'past_w': (('gaug',), "the pixels past W in a row's last unit let in (they are the next row's first)"),
    'cross_image': (('gaug',), "a tap allowed across an image's top or bottom edge into the neighbouring image"),
    'no_mask': (('gaug', 'dgamma2', 'dbeta2', 'dY'), 'the ReLU mask dropped'),
    'mask_from_dA': (('gaug', 'dgamma2', 'dbeta2', 'dY'), 'the ReLU mask taken from dA > 0'),
    'no_cC': (('gaug',), 'cC omitted'),
    'y_unrounded': (('gaug',), 'y read unrounded where it is bfloat16-stored'),
    'pair_swapped': (('gaug',), 'the two halves of a packed bfloat16 pair exchanged'),
    'xhat_no_eps': (('xaug',), 'x^ without the epsilon'),
}


def launch_shape(shape):
    """conv_first.hip conv_first_wgrad: (segs, units, waves, per_wave)."""
    n, h, wd = shape
    segs = (wd + 3) // 4
    units = n * h * segs
    waves = 4096
    if waves > (units + 15) // 16:
        waves = ((units + 15) // 16 + 3) // 4 * 4
    return segs, units, waves, (units + waves - 1) // waves


def _gaug_f32(xa, dY, shape, mutant):
    """The weight gradient over [x^, 1] with fp32 accumulation: fp32 partial sums of 256 pixels each, summed in fp32."""
    n, h, wd = shape
    ca = xa.shape[-1]
    dY = np.ascontiguousarray(dY, F32)
    if mutant == 'unit_dropped':          # the last unit of wave 0's range
        segs, units, _, per_wave = launch_shape(shape)
        u = min(per_wave, units) - 1
        row, seg = divmod(u, segs)
        dY = dY.copy()
        dY.reshape(n * h, wd, CO)[row, seg * 4:seg * 4 + 4] = 0
    src = xa.reshape(1, n * h, wd, ca) if mutant == 'cross_image' else xa
    cols = _cols(np.ascontiguousarray(src, F32)).reshape(-1, 9 * ca)
    d2 = dY.reshape(-1, CO)
    acc = np.zeros((9 * ca, CO), F32)
    for r0 in range(0, d2.shape[0], 256):
        acc += cols[r0:r0 + 256].T @ d2[r0:r0 + 256]
    if mutant == 'past_w' and wd % 4:
        # the lanes px in [W, 4 segs) of each row's last unit, not masked: pixel row * W + px is the next row's pixel px - W, its
        # taps judged as for column px of this row (so only px = W, dw = -1 passes the column test)
        xf, rows = np.ascontiguousarray(xa, F32).reshape(-1, ca), n * h * wd
        for r in range(n * h):
            for px in range(wd, (wd + 3) // 4 * 4):
                p = r * wd + px
                if p >= rows:
                    continue
                for tap in range(9):
                    dh, dw = tap // 3 - 1, tap % 3 - 1
                    q = p + dh * wd + dw
                    if 0 <= r % h + dh < h and px + dw < wd and 0 <= q < rows:
                        acc[tap * ca:(tap + 1) * ca] += np.outer(xf[q], d2[p])
    g = acc.reshape(3, 3, ca, CO)
    if mutant == 'taps_transposed':
        g = g.transpose(1, 0, 2, 3)
    return np.ascontiguousarray(g).reshape(9, ca, CO)


def emulate(cs, relu, form, mutant=None):
    """What l3_op_first_block_bwd returns, from the kernels' formulas in fp32 NumPy."""
    shape, c = cs['shape'], cs['c']
    bf16 = form == 'deferred_bf16'
    assert bf16 == cs['bf16']
    x, gi, bi, w, g2, b2 = (np.asarray(cs[k], F32) for k in ('x', 'gamma_in', 'beta_in', 'w', 'gamma2', 'beta2'))
    y, dA = np.asarray(cs['y'], F32), np.asarray(cs['dA'], F32)
    out = {}
    with np.errstate(all='ignore'):
        mean, var, _, _ = bs._stats_f32(x, gi, bi)
        rs = F32(1) / np.sqrt(var + (F32(0) if mutant == 'xhat_no_eps' else EPS32)).astype(F32)
        xa = np.concatenate([((x - mean) * rs).astype(F32), np.ones(x.shape[:3] + (1,), F32)], axis=-1)
        out.update(mean_in=mean, var_in=var, xaug=xa)
        m2, v2, sc, sh = bs._stats_f32(y, g2, b2)
        out.update(mean2=m2, var2=v2, scale2=sc, shift2=sh)
        pre = bs._fma(y, sc, sh)
        keep = np.ones(y.shape, bool) if not relu or mutant == 'no_mask' else (dA > 0) if mutant == 'mask_from_dA' else pre > 0
        d = np.where(keep, dA, F32(0))
        rs2 = (F32(1) / np.sqrt(v2 + EPS32)).astype(F32)
        s0, s1 = d.reshape(-1, CO).sum(0, dtype=F64), (d * ((y - m2) * rs2)).reshape(-1, CO).sum(0, dtype=F64)
        dg2, db2, A, B, Cc = bs._bwd_coeffs(s0, s1, g2, m2, v2, y.size // CO)
        out.update(dgamma2=dg2, dbeta2=db2)
        yk, dk = y, d
        if mutant == 'y_unrounded':
            yk = np.asarray(cs['y_f32'], F32)
        if mutant == 'pair_swapped':
            swap = np.arange(CO) ^ 1
            yk, dk = y[..., swap], d[..., swap]
        dY = bs._fma(A, dk, bs._fma(B, yk, F32(0) if mutant == 'no_cC' else Cc))
        if form == 'explicit':
            out['dY'] = dY
        else:
            out.update(cA=A, cB=B, cC=Cc)
        gaug = _gaug_f32(xa, dY, shape, mutant)
        out['gaug'] = gaug
        G, S = gaug[:, :c], gaug[:, c]
        Sd = np.roll(S, -1, axis=0) if mutant == 's_next_tap' else S
        ga, be = (bi, gi) if mutant == 'gamma_beta_swapped' else (gi, bi)
        # (the compiler contracts gamma G + beta S to one multiply and one fused multiply-add: two roundings)
        out['dw'] = bs._fma(ga[None, :, None], G, (be[None, :, None] * Sd[:, None]).astype(F32)).reshape(3, 3, c, CO)
        w9 = w.reshape(9, c, CO).astype(F64)
        wg = np.roll(w9, -1, axis=1) if mutant == 'dgamma_next_channel' else w9
        out['dgamma_in'] = (wg * G.astype(F64)).sum((0, 2)).astype(F32)
        out['dbeta_in'] = (w9 * Sd.astype(F64)[:, None]).sum((0, 2)).astype(F32)
        if form == 'explicit':
            out['dbias'] = dY.reshape(-1, CO).sum(0, dtype=F64).astype(F32)
        else:
            out['dbias'] = S[0 if mutant == 'bias_tap0' else 4].copy()
    return out


def first_conv_grads_f32(gaug, w, gamma, beta):
    """first_conv_grads alone in fp32 (double column sums)."""
    gaug, w, gamma, beta = (np.asarray(a, F32) for a in (gaug, w, gamma, beta))
    c = w.shape[1]
    G, S = gaug[:, :c], gaug[:, c]
    dw = bs._fma(gamma[None, :, None], G, (beta[None, :, None] * S[:, None]).astype(F32))
    return (dw, (w.astype(F64) * G).sum((0, 2)).astype(F32), (w.astype(F64) * S[:, None]).sum((0, 2)).astype(F32),
            S[gaug.shape[0] // 2].copy())


def grads_inputs(taps, c, co):
    rng = np.random.default_rng([5, taps, c, co])
    gaug = rng.standard_normal((taps, c + 1, co), dtype=F32) * F32(0.05)
    w = (rng.standard_normal((taps, c, co)) * np.sqrt(2.0 / (taps * c))).astype(F32)
    return gaug, w, (1 + 0.1 * rng.standard_normal(c)).astype(F32), (0.1 * rng.standard_normal(c)).astype(F32)


# ---- the comparators ---------------------------------------------------------------------------------------------------------------
_ratio = es._ratio


def grads_ratios(gaug, w, gamma, beta, dw, dgamma, dbeta, dbias):
    """first_conv_grads from ITS gaug (taps, C + 1, Co), w (taps, C, Co): dw within 2^-23 (|gamma G| + |beta S|) -- two roundings --;
    dbias (where written) bit-equal to the ones-channel row of the centre tap; dgamma / dbeta within 2^-24 |ref| + 1e-12 sum |W g|
    -- accumulated in double, rounded once."""
    g64, w64 = np.asarray(gaug, F64), np.asarray(w, F64)
    c = w64.shape[1]
    G, S = g64[:, :c], g64[:, c]
    gm, bt = np.asarray(gamma, F64)[None, :, None], np.asarray(beta, F64)[None, :, None]
    dw_r, dg_r, db_r, dbias_r = closed_from_gaug(g64, w64, gamma, beta)
    res = {'dw': _ratio(np.abs(np.asarray(dw, F64).reshape(dw_r.shape) - dw_r), 2 * U24 * (np.abs(gm * G) + np.abs(bt * S[:, None]))),
           'dgamma_in': _ratio(np.abs(np.asarray(dgamma, F64) - dg_r), U24 * np.abs(dg_r) + 1e-12 * np.abs(w64 * G).sum((0, 2))),
           'dbeta_in': _ratio(np.abs(np.asarray(dbeta, F64) - db_r), U24 * np.abs(db_r) + 1e-12 * np.abs(w64 * S[:, None]).sum((0, 2)))}
    if dbias is not None:
        res['dbias'] = 0.0 if np.array_equal(np.asarray(dbias, F32), np.asarray(gaug, F32)[g64.shape[0] // 2, c]) else np.inf
    return res


def implied_dy(cs, relu, out):
    """(dY, T) in float64 as the weight-gradient kernel had them: the returned dY and |dY| (explicit), or what the returned
    coefficients, scale, shift and the stored y, dA imply, and the magnitudes of the terms the kernel adds (deferred)."""
    if 'dY' in out:
        dY = np.asarray(out['dY'], F64)
        return dY, np.abs(dY)
    y, dA = _p64(cs, 'y', 'dA')
    d = np.where(bn2_pre(y, out['scale2'], out['shift2']) > 0, dA, 0.0) if relu else dA
    a, b = np.asarray(out['cA'], F64) * d, np.asarray(out['cB'], F64) * y
    cc = np.asarray(out['cC'], F64)
    return a + (b + cc), np.abs(a) + np.abs(b) + np.abs(cc)


def stage_ratios(cs, relu, form, out):
    """Every stage of one operator call against float64 arithmetic on what the call returned for the stage before."""
    c = cs['c']
    x, y, dA = _p64(cs, 'x', 'y', 'dA')
    res = {}
    # the input BatchNorm's moments: test_batchnorm_fwd_bwd's bounds
    x2 = x.reshape(-1, c)
    res['mean_in'] = bs.relerr(out['mean_in'], x2.mean(0)) / 1e-6
    res['var_in'] = bs.relerr(out['var_in'], x2.var(0)) / 5e-6
    # [x^, 1]: the ones exact; x^ one subtraction, one reciprocal square root, one product from the returned moments
    xa = np.asarray(out['xaug'], F64)
    res['ones'] = 0.0 if np.all(np.asarray(out['xaug'])[..., c] == 1.0) else np.inf
    xh = (x - np.asarray(out['mean_in'], F64)) / np.sqrt(np.asarray(out['var_in'], F64) + EPS64)
    res['xaug'] = _ratio(np.abs(xa[..., :c] - xh), 8 * U24 * np.abs(xh))
    # the second BatchNorm: moments of the stored y; reductions over the stored y and dA, mask from the returned scale and shift
    y2 = y.reshape(-1, CO)
    res['mean2'] = bs.relerr(out['mean2'], y2.mean(0)) / 1e-6
    res['var2'] = bs.relerr(out['var2'], y2.var(0)) / 5e-6
    m2, v2 = np.asarray(out['mean2'], F64), np.asarray(out['var2'], F64)
    t0 = (np.where(bn2_pre(y, out['scale2'], out['shift2']) > 0, dA, 0.0) if relu else dA).reshape(-1, CO)
    t1 = t0 * (y2 - m2) / np.sqrt(v2 + EPS64)
    res['dbeta2'] = es.sum_ratio(out['dbeta2'], t0)
    res['dgamma2'] = es.sum_ratio(out['dgamma2'], t1)
    # dY -- returned, or implied by the returned coefficients -- against the float64 BatchNorm backward of the stored tensors
    # (bn_storage_ref's criterion for dx: TOL of the reference's largest entry; of its largest term where it is identically 0)
    dY, T = implied_dy(cs, relu, out)
    ref = reference(cs['shape'], c, cs['bf16'], relu)
    res['dY'] = bs.relerr(dY, ref['dY'], None if np.any(ref['dY']) else float(np.abs(ref['cA'] * dA).max())) / TOL
    # gaug: per entry against the float64 sum over the returned xaug and that dY, TOL of the sum of the terms' magnitudes
    res['gaug'] = _ratio(np.abs(np.asarray(out['gaug'], F64) - wgrad64(xa, dY)), TOL * wgrad64(np.abs(xa), T))
    # first_conv_grads from the returned gaug
    res.update(grads_ratios(out['gaug'], np.asarray(cs['w']).reshape(9, c, CO), cs['gamma_in'], cs['beta_in'], out['dw'],
                            out['dgamma_in'], out['dbeta_in'], out['dbias'] if form != 'explicit' else None))
    return res


@functools.lru_cache(maxsize=4)
def reference(shape, c, bf16, relu):
    """The float64 chain of a case, computed once and shared (read-only) by every form that runs it."""
    ch = chain(case(shape, c, bf16), relu)
    for a in ch.values():
        a.setflags(write=False)
    return ch


@functools.lru_cache(maxsize=4)
def e2e_reference(shape, c, bf16, relu, explicit):
    """The float64 chain of a case and the bounds that follow from it, computed once: (chain, M, column sums of T) with M
    (9, C + 1, 64) the sums of the magnitudes of gaug's terms -- |x^| (or 1) times T, T = |dY| (explicit) or the magnitudes of dY's
    three terms (deferred)."""
    ch = reference(shape, c, bf16, relu)
    xa = np.concatenate([np.abs(ch['xhat']), np.ones(ch['xhat'].shape[:3] + (1,))], axis=-1)
    T = np.abs(ch['dY']) if explicit else ch['T']
    return ch, wgrad64(xa, T), T.reshape(-1, CO).sum(0)


def e2e_ratios(cs, relu, form, out):
    """The operator's end results against the pure float64 chain (cases of E2E_MIN_PIXELS pixels and more)."""
    shape, c = cs['shape'], cs['c']
    ch, M, tsum = e2e_reference(shape, c, cs['bf16'], relu, form == 'explicit')
    w9 = np.abs(np.asarray(cs['w'], F64)).reshape(9, c, CO)
    gm, bt = np.abs(np.asarray(cs['gamma_in'], F64))[None, :, None], np.abs(np.asarray(cs['beta_in'], F64))[None, :, None]
    MG, MS = M[:, :c], M[:, c][:, None]
    res = {'e2e:dw': _ratio(np.abs(np.asarray(out['dw'], F64) - ch['dw']).reshape(9, c, CO), TOL * (gm * MG + bt * MS))}
    bg, bb = TOL * (w9 * MG).sum((0, 2)), TOL * (w9 * MS).sum((0, 2))
    res['e2e:dgamma_in'] = _ratio(np.abs(np.asarray(out['dgamma_in'], F64) - ch['dgamma_in']), bg)
    res['e2e:dbeta_in'] = _ratio(np.abs(np.asarray(out['dbeta_in'], F64) - ch['dbeta_in']), bb)
    # analytically zero (a BatchNorm follows): the chain's own dbias is rounding noise
    res['e2e:dbias'] = _ratio(np.abs(np.asarray(out['dbias'], F64)), TOL * tsum)
    if shape in BITE_SHAPES:          # the propagated bound is loose where the sums cancel: it must still bite
        res['bite:dgamma_in'] = float(bg.max() / np.abs(ch['dgamma_in']).max()) / BITE
        res['bite:dbeta_in'] = float(bb.max() / np.abs(ch['dbeta_in']).max()) / BITE
    return res


def all_ratios(cs, relu, form, out):
    res = stage_ratios(cs, relu, form, out)
    n, h, wd = cs['shape']
    if n * h * wd >= E2E_MIN_PIXELS:
        res.update(e2e_ratios(cs, relu, form, out))
    return res


def lines(cs, relu, form, res):
    return ['FIRSTBLK %s %s %s %.4g' % (instantiation(cs['c'], form, relu), tag(cs['shape'], cs['c']), k, v) for k, v in sorted(res.items())]
