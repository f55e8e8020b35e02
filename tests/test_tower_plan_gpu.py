"""The per-pass rule of the tower plan (engine.hip plan_tower): the kernel path of every tower layer is resolved at the head of
each pass, so a per-call debug knob (L3_WINO4, L3_CONV_FIRST, L3_BF16_HALO -- the kernels read them per launch) set AFTER an engine
was created governs its next pass exactly as if it had been set before: the engine's bookkeeping (which BatchNorm reads how many
epilogue partial blocks) and the kernels cannot disagree.

cnn_L3_melspec2 at batch 2: the smallest engine with epilogue statistics, pooled and unpooled BatchNorm-backward fusion and the
deferred first-layer BatchNorm.  Every comparison is bit for bit.  (L3_CONV_FIRST is not switched on a bf16 engine: the first
conv's bfloat16 output storage is fixed at creation from that knob.)"""
import numpy as np
import pytest

from l3embedding_amd import _lib
from oracle import l3_oracle as o

pytestmark = pytest.mark.gpu

MT, B = 'cnn_L3_melspec2', 2
CASES = [('L3_WINO4', '0', 'f32'), ('L3_CONV_FIRST', '0', 'f32'), ('L3_BF16_HALO', '0', 'bf16')]


@pytest.fixture(scope='module')
def data():
    P = o.init_params(MT, seed=7)
    P['dense_2/kernel'] = (P['dense_2/kernel'] / np.float32(64)).astype(np.float32)      # a live head: every sample has a loss gradient
    return P, [o.synthetic_batch(B, seed=11 + k) for k in range(2)]


def _engine(P, dtype):
    eng = _lib.Engine(MT, B, seed=0, dtype=dtype)
    eng.set_params(P)
    return eng


def _first_bns(eng):
    """Per tower: its input BatchNorm and the first BatchNorm behind a convolution (the consumer of epilogue statistics).
    Relies on param_table() listing a tower's parameters in the order of its ops, so the first two '/gamma' rows are those two."""
    names = []
    for tower in ('vision_model', 'audio_model'):
        bns = [n[:-len('/gamma')] for n, _, _ in eng.param_table() if n.startswith(tower + '/') and n.endswith('/gamma')]
        names += bns[:2]
    assert len(names) == 4, names
    return names


def _pass(eng, batch):
    """One training forward and every backward bucket: loss, the first BatchNorm outputs, every gradient."""
    eng.upload_batch(*batch)
    eng.step_forward(True)
    for b in range(1, eng.bucket_count()):
        eng.step_backward_bucket(b)
    eng.sync()
    loss, _ = eng.step_results()
    out = {'loss': np.float32(loss)}
    for n in _first_bns(eng):
        out['act ' + n] = eng.activation(n)
    for n, g in eng.get_grads().items():
        out['grad ' + n] = g
    return out


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    diff = [k for k in want if not np.array_equal(got[k], want[k])]
    print(what, '%d tensors compared, %d differ' % (len(want), len(diff)))
    assert not diff, (what, diff)
    assert all(np.isfinite(x).all() for x in want.values())
    assert any(np.abs(x).max() > 0 for k, x in want.items() if k.startswith('grad vision_model/')), 'no gradient reached the towers'


@pytest.mark.parametrize('knob,value,dtype', CASES, ids=['%s=%s-%s' % c for c in CASES])
def test_knob_set_after_creation_governs_the_next_pass(gpu_required, data, monkeypatch, knob, value, dtype):
    P, batches = data
    monkeypatch.delenv(knob, raising=False)
    a = _engine(P, dtype)                     # A: created, THEN the knob
    plain = _engine(P, dtype)
    base = _pass(plain, batches[0])
    plain.close()
    monkeypatch.setenv(knob, value)
    got = _pass(a, batches[0])
    a.close()
    b = _engine(P, dtype)                     # B: the knob, then created
    want = _pass(b, batches[0])
    b.close()
    _assert_same(got, want, '%s=%s %s' % (knob, value, dtype))
    # the knob does switch kernels: some tensor differs from the pass without it
    assert any(not np.array_equal(base[k], want[k]) for k in want), 'the knob changed nothing'


def test_knob_changed_between_two_steps_of_one_engine(gpu_required, data, monkeypatch):
    """Step 1 under the product setting, step 2 under L3_WINO4=0 on ONE engine == a fresh engine that ran step 1 under the first
    setting and step 2 under the second (the second step's results and the weights after both updates) == an engine created under
    the second setting that took over the state behind step 1 and ran step 2 alone.  The knob is live: the same second step
    without it differs."""
    P, batches = data

    def step(eng, batch):
        out = _pass(eng, batch)
        eng.step_update(1e-4, 1.0)
        eng.sync()
        for n, p in eng.get_params().items():
            out['param ' + n] = p
        return out

    monkeypatch.delenv('L3_WINO4', raising=False)
    one, fresh, plain = _engine(P, 'f32'), _engine(P, 'f32'), _engine(P, 'f32')
    for e in (one, fresh, plain):
        step(e, batches[0])
    base = step(plain, batches[1])            # step 2 with the knob still unset
    plain.close()
    monkeypatch.setenv('L3_WINO4', '0')
    late = _lib.Engine(MT, B, seed=0, dtype='f32')
    late.copy_state_from(one)
    got, want, want_late = step(one, batches[1]), step(fresh, batches[1]), step(late, batches[1])
    for e in (one, fresh, late):
        e.close()
    _assert_same(got, want, 'L3_WINO4 unset -> 0 between steps, fresh engine')
    _assert_same(got, want_late, 'L3_WINO4 unset -> 0 between steps, engine created under 0')
    assert any(not np.array_equal(base[k], got[k]) for k in got), 'the knob changed nothing in step 2'


def _first_convs(eng):
    """Per tower: (tower, full name) of its first convolution (the first-layer kernel) and of its first wide one.  param_table()
    lists a tower's parameters in the order of its ops, as in _first_bns."""
    out = []
    for tower in ('vision', 'audio'):
        convs = [n[:-len('/kernel')] for n, _, _ in eng.param_table() if n.startswith(tower + '_model/') and n.endswith('/kernel')]
        out += [(tower, c) for c in convs[:2]]
    return out


def _is_bf16(a):
    """every value is a bfloat16: what Engine.activation() returns of a bfloat16-stored tensor"""
    return not (a.view(np.uint32) & 0xffff).any()


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_operator_is_the_engines_convolution(gpu_required, data, dtype):
    """op_conv2d_fwd resolves and runs a convolution through the same code as the engine (csrc/conv_path.h), so on an engine's own
    operands it returns the engine's own activation, bit for bit.  The first two convolutions of each tower -- the first-layer
    kernel, the first wide layer -- in a solo training forward (l3_tower_step: ConvGeom::solo = 1, the operators' setting).

    What a convolution reads is the output tensor of the BatchNorm in front of it: the input BatchNorm for the first one, and
    for the second the BatchNorm behind the first, whose ReLU is folded into it (find_tower_tensor returns an op's output
    tensor, and push_relu gives a ReLU fused into a BatchNorm no tensor of its own), so that name holds the post-ReLU tensor.
    In the bf16 engine both convolutions store bfloat16 (alloc_everything): the first-layer kernel from fp32 input, the wide
    layer from the bfloat16-stored BatchNorm output -- the operator's stored-out form of either."""
    P, batches = data
    eng = _engine(P, dtype)
    eng.upload_batch(*batches[0])
    bns, convs = _first_bns(eng), _first_convs(eng)
    acts = {}
    for tower in ('vision', 'audio'):
        eng.tower_step(tower, backward=False)
        eng.sync()
        for n in bns + [c for _, c in convs]:
            if n.startswith(tower):
                acts[n] = eng.activation(n)
    params = eng.get_params()
    eng.close()
    for i, (tower, name) in enumerate(convs):
        k, b = params[name + '/kernel'], params[name + '/bias']
        want = acts[name]
        x = acts[bns[i]].reshape((B,) + {'vision': (224, 224), 'audio': (256, 199)}[tower] + (k.shape[2],))
        first = i % 2 == 0
        assert (k.shape[2] in (1, 3)) == first and k.shape[3] == 64, (name, k.shape)
        if dtype == 'bf16':
            assert _is_bf16(want) and _is_bf16(x) == (not first), name       # the storage the operator's dtype has to state
        got = _lib.op_conv2d_fwd(x, k, b, True, dtype='f32' if dtype == 'f32' else 'bf16_stored_out')
        same = np.array_equal(got.reshape(-1), want)
        print('%s %s: %d values, max |.| %.3e, bit-identical %s' % (dtype, name, want.size, np.abs(want).max(), same))
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        assert same, (dtype, name, float(np.abs(got.reshape(-1) - want).max()))
