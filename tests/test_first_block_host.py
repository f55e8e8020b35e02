"""first_block_ref.py on the CPU: the closed form the engine uses equals the straightforward float64 chain (which computes the first
layer's data gradient and the input BatchNorm's backward the engine never does), the chain equals central finite differences of the
loss, the honest fp32 restatement of the kernels stays below HONEST of every criterion test_first_block_gpu.py applies (below 1 of
the three that are exact rounding counts: ROUNDING_BOUNDS), and each named mutant pushes a criterion named for it above 1."""
import numpy as np
import pytest

import first_block_ref as R

# the smallest and the largest small case of each channel count
YARD_SHAPES = [R.SMALL_SHAPES[0], R.SMALL_SHAPES[-1]]
HONEST = 0.5
# first_conv_grads' three bounds are not tolerances but the worst case of the roundings counted: dw = fl(gamma G + fl(beta S)) (or
# three roundings, uncontracted) is within 2^-24 (|beta S| + |dw|) <= 2^-23 (|gamma G| + |beta S|), and a double sum rounded once is
# within 2^-24 of itself.  Honest arithmetic comes arbitrarily close to such a bound (a value just above a power of two) and never
# passes it, whatever the order of the double sum (1e-12 of the terms' magnitudes covers that): held below 1, not below HONEST.
ROUNDING_BOUNDS = ('dw', 'dgamma_in', 'dbeta_in')
F64 = np.float64


@pytest.mark.parametrize('shape,c', R.SMALL_CASES, ids=[R.tag(s, c) for s, c in R.SMALL_CASES])
def test_case_meets_its_margins(shape, c):
    for bf16 in (False, True):
        cs = R.case(shape, c, bf16)          # (asserts that at most 1 % of dA was zeroed)
        assert cs['zeroed'] <= 0.01
        if bf16:
            assert np.array_equal(R.o.bf16_round(cs['y']), cs['y']) and np.array_equal(R.o.bf16_round(cs['dA']), cs['dA'])


@pytest.mark.parametrize('shape,c', R.SMALL_CASES, ids=[R.tag(s, c) for s, c in R.SMALL_CASES])
def test_closed_form_is_the_float64_chain(shape, c):
    cs = R.case(shape, c)
    for relu in (0, 1):
        ch = R.chain(cs, relu)
        cl = R.closed(cs, ch)
        for k in ('dw', 'dbias', 'dgamma_in', 'dbeta_in'):
            scale = max(np.abs(ch[k]).max(), np.abs(ch['dw']).max())
            assert np.abs(cl[k] - ch[k]).max() <= 1e-12 * scale, (relu, k, np.abs(cl[k] - ch[k]).max(), scale)


@pytest.mark.parametrize('shape,c', [((2, 9, 7), 1), ((3, 6, 10), 3)], ids=['2x9x7x1', '3x6x10x3'])
def test_chain_is_the_gradient_of_the_loss(shape, c):
    """Central differences of L = sum dA act(BN2(conv(BN_in(x)))) in gamma_in, beta_in and a handful of filter entries.  dA is 0
    wherever the second BatchNorm's pre-activation is within 1e-3 of 0, so no step of 1e-5 crosses a ReLU kink that counts."""
    cs = R.case(shape, c)
    h = 1e-5
    for relu in (0, 1):
        _, y = R.forward_loss(cs, relu)
        ch = R.chain(cs, relu, y=y)
        gi, bi, w = (np.asarray(cs[k], F64) for k in ('gamma_in', 'beta_in', 'w'))
        checks = []
        for ci in range(c):
            e = np.zeros(c)
            e[ci] = h
            checks.append(('dgamma_in', ch['dgamma_in'][ci],
                           (R.forward_loss(cs, relu, gamma_in=gi + e)[0] - R.forward_loss(cs, relu, gamma_in=gi - e)[0]) / (2 * h)))
            checks.append(('dbeta_in', ch['dbeta_in'][ci],
                           (R.forward_loss(cs, relu, beta_in=bi + e)[0] - R.forward_loss(cs, relu, beta_in=bi - e)[0]) / (2 * h)))
        for idx in [(0, 0, 0, 0), (1, 1, c - 1, 63), (2, 0, 0, 17), (0, 2, c - 1, 40), (1, 2, 0, 5)]:
            e = np.zeros(w.shape)
            e[idx] = h
            checks.append(('dw%r' % (idx,), ch['dw'][idx],
                           (R.forward_loss(cs, relu, w=w + e)[0] - R.forward_loss(cs, relu, w=w - e)[0]) / (2 * h)))
        scale = np.abs(ch['dw']).max()
        for name, got, fd in checks:
            assert abs(got - fd) <= 1e-6 * max(scale, abs(got)), (relu, name, got, fd)


@pytest.mark.parametrize('shape,c', R.SMALL_CASES, ids=[R.tag(s, c) for s, c in R.SMALL_CASES])
def test_honest_fp32_restatement_stays_under_half_of_every_criterion(shape, c):
    """On every small case and form: fp32 arithmetic in the kernels' formulas takes less than HONEST of each bound the GPU test
    applies (ROUNDING_BOUNDS: less than all of it), so the bounds are attainable with room for another summation order; the
    propagated dgamma_in / dbeta_in bounds stay under BITE of the tensor where they are asserted to."""
    worst = {}
    for form, relu in R.SMALL_FORMS:
        cs = R.case(shape, c, form == 'deferred_bf16')
        res = R.all_ratios(cs, relu, form, R.emulate(cs, relu, form))
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
            limit = 1.0 if k.startswith('bite:') or k in ROUNDING_BOUNDS else HONEST
            assert v < limit, (form, relu, k, v)
    print('HONEST %s %s' % (R.tag(shape, c), ' '.join('%s=%.3g' % kv for kv in sorted(worst.items()))))


def _bites(mutant, shape, c, form, relu):
    cs = R.case(shape, c, form == 'deferred_bf16')
    res = R.all_ratios(cs, relu, form, R.emulate(cs, relu, form, mutant))
    return {k: v for k, v in res.items() if k in R.MUTANTS[mutant][0] and v > 1.0}


# where each mutant exists: (form, relu) and, of the yardstick cases, those on which it changes anything
_WHERE = {
    'dgamma_next_channel': dict(c=(3,)),
    'bias_tap0': dict(forms=[('deferred', 1)]),                           # the explicit form's dbias is bn_bwd_fast's
    'unit_dropped': dict(),
    'past_w': dict(shapes=[R.SMALL_SHAPES[-1]]),                          # needs a next row
    'cross_image': dict(shapes=[R.SMALL_SHAPES[-1]]),                     # needs two images
    'no_mask': dict(forms=[('deferred', 1), ('deferred_bf16', 1), ('explicit', 1)], shapes=[R.SMALL_SHAPES[-1]]),
    'mask_from_dA': dict(forms=[('deferred', 1), ('deferred_bf16', 1), ('explicit', 1)], shapes=[R.SMALL_SHAPES[-1]]),
    'no_cC': dict(forms=[('deferred', 0), ('deferred', 1), ('deferred_bf16', 1)]),
    'y_unrounded': dict(forms=[('deferred_bf16', 0), ('deferred_bf16', 1)], shapes=[R.SMALL_SHAPES[-1]]),
    'pair_swapped': dict(forms=[('deferred_bf16', 0), ('deferred_bf16', 1)]),
}


@pytest.mark.parametrize('mutant', sorted(R.MUTANTS))
def test_each_mutant_fails_a_criterion_named_for_it(mutant):
    where = _WHERE.get(mutant, {})
    forms = where.get('forms', [('deferred', 1)])
    for shape in where.get('shapes', YARD_SHAPES):
        for c in where.get('c', (1, 3)):
            for form, relu in forms:
                hit = _bites(mutant, shape, c, form, relu)
                assert hit, '%s (%s) passes every criterion named for it on %s %s relu %d' % (
                    mutant, R.MUTANTS[mutant][1], R.tag(shape, c), form, relu)


@pytest.mark.parametrize('taps,c,co', R.GRADS_SHAPES)
def test_first_conv_grads_yardstick(taps, c, co):
    gaug, w, gamma, beta = R.grads_inputs(taps, c, co)
    res = R.grads_ratios(gaug, w, gamma, beta, *R.first_conv_grads_f32(gaug, w, gamma, beta))
    assert max(res.values()) < 1.0, res          # (ROUNDING_BOUNDS)
    dw, dg, db, dbias = R.first_conv_grads_f32(gaug, w, gamma, beta)
    assert R.grads_ratios(gaug, w, gamma, beta, dw, 2 * dg, db, dbias)['dgamma_in'] > 1          # a factor of two
    assert R.grads_ratios(gaug, w, gamma, beta, dw, dg, 2 * db, dbias)['dbeta_in'] > 1
    if taps > 1:
        assert R.grads_ratios(gaug, w, gamma, beta, dw, dg, db, gaug[0, c])['dbias'] > 1


def test_launch_shapes_are_the_ones_the_cases_name():
    """conv_first_wgrad's launch arithmetic for each case: what the case list says it reaches."""
    assert R.launch_shape((1, 1, 3)) == (1, 1, 4, 1)
    assert R.launch_shape((1, 3, 2)) == (1, 3, 4, 1)
    assert R.launch_shape((2, 9, 7)) == (2, 36, 4, 9)
    assert R.launch_shape((3, 6, 10)) == (3, 54, 4, 14)
    assert R.launch_shape((1, 5, 199)) == (50, 250, 16, 16)
    assert R.launch_shape((2, 64, 50)) == (13, 1664, 104, 16)
    assert R.launch_shape((6, 256, 199)) == (50, 76800, 4096, 19)
    assert R.launch_shape((6, 224, 224)) == (56, 75264, 4096, 19)
