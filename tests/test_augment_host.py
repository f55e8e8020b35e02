"""CPU tests of the augmentation's host side (l3embedding_amd/augment.py, train.train_augmented) and known answers of the
float64 yardstick the GPU tests compare against (tests/augment_ref.py)."""
import inspect
import json
import os
import random

import numpy as np
import pytest

from l3embedding_amd import augment, train as T
from l3embedding_amd.model import L3Model
from l3embedding_amd.training_utils import get_slice_bounds

import augment_ref as R


# ---- draw_params ------------------------------------------------------------------------------------------------------
def _by_hand(seed, n, h, w):
    """The reference's calls, written out: sample.py:156 (uniform's random()), 182, 244, 252, 254-260 / 264-271."""
    rng = random.Random(seed)
    rows = []
    for _ in range(n):
        u = rng.random()
        sx = rng.randrange(h - 224) if h > 224 else 0
        sy = rng.randrange(w - 224) if w > 224 else 0
        flip = rng.random() < 0.5
        if rng.random() < 0.5:
            first = True
            sat = np.float32(rng.random() + 0.5)
            max_delta = 32. / 255.
            bri = np.float32((2 * rng.random() - 1) * max_delta)
        else:
            first = False
            max_delta = 32. / 255.
            bri = np.float32((2 * rng.random() - 1) * max_delta)
            sat = np.float32(rng.random() + 0.5)
        rows.append((u, sx, sy, flip, first, sat, bri))
    return rows


@pytest.mark.parametrize('shape', [(224, 224), (230, 245)])
def test_draw_params_follow_the_reference_call_order(shape):
    n = 64
    p = augment.draw_params(random.Random(20180123), n, shape)
    want = _by_hand(20180123, n, *shape)
    assert p.dtype == augment.PARAMS and p.shape == (n,)
    for row, (u, sx, sy, flip, first, sat, bri) in zip(p, want):
        assert row['u_gain'] == u and row['start_x'] == sx and row['start_y'] == sy
        assert bool(row['flip']) == flip and bool(row['sat_first']) == first
        assert row['saturation'].dtype == np.float32 and row['saturation'] == sat          # float32-exact
        assert row['brightness'].dtype == np.float32 and row['brightness'] == bri
    assert (p['saturation'] >= 0.5).all() and (p['saturation'] < 1.5).all()
    assert (np.abs(p['brightness']) <= np.float32(32. / 255.)).all()
    assert (p['u_gain'] >= 0).all() and (p['u_gain'] < 1).all()
    assert 0 < p['flip'].sum() < n and 0 < p['sat_first'].sum() < n                       # both branches were taken
    if shape == (224, 224):
        assert not p['start_x'].any() and not p['start_y'].any()
    else:
        assert p['start_x'].max() <= 5 and p['start_y'].max() <= 20 and p['start_x'].any() and p['start_y'].any()
    with pytest.raises(ValueError):
        augment.draw_params(random.Random(0), 1, (223, 224))


def test_identity_params():
    p = augment.identity_params(3)
    assert p.dtype == augment.PARAMS and not p['flip'].any() and not p['start_x'].any() and not p['start_y'].any()
    assert (p['saturation'] == 1).all() and (p['brightness'] == 0).all()


# ---- known answers of the yardstick --------------------------------------------------------------------------------------
def _one(frame, **kw):
    p = augment.identity_params(1)
    for k, v in kw.items():
        p[k] = v
    return R.augment_frame(frame, p[0])


def _tile(rgb):
    return np.broadcast_to(np.array(rgb, np.uint8), (224, 224, 3)).copy()


def test_reference_known_answers():
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (224, 224, 3)).astype(np.uint8)
    assert np.array_equal(_one(img), img)                                                  # identity
    assert np.array_equal(_one(img, sat_first=0), img)
    assert np.array_equal(_one(img, flip=1), img[:, ::-1])
    big = rs.randint(0, 256, (230, 245, 3)).astype(np.uint8)
    assert np.array_equal(_one(big, start_x=5, start_y=20), big[5:229, 20:244])
    grey = np.repeat(rs.randint(0, 256, (224, 224, 1)), 3, -1).astype(np.uint8)
    for factor in (0.5, 1.49):
        assert np.array_equal(_one(grey, saturation=factor), grey)                         # greys have no saturation to scale
    # (255, 0, 0) at factor 0.5: 0.5 * 255 = 127.5 exactly, and rint rounds the half to the even 128
    assert _one(_tile((255, 0, 0)), saturation=0.5)[0, 0].tolist() == [255, 128, 128]
    # saturation cannot exceed 1: a fully saturated colour is unchanged by a factor above 1
    assert _one(_tile((0, 200, 0)), saturation=1.49)[0, 0].tolist() == [0, 200, 0]
    d = np.float32(32. / 255.)
    assert _one(_tile((250, 250, 250)), brightness=d)[0, 0].tolist() == [255, 255, 255]    # clipped at the top
    assert _one(_tile((100, 10, 40)), brightness=d)[0, 0].tolist() == [132, 42, 72]
    assert _one(_tile((100, 10, 40)), brightness=-d)[0, 0].tolist() == [68, 0, 8]
    # the order matters once brightness clips: (250, 100, 100), +32/255, factor 0.5
    a = _one(_tile((250, 100, 100)), saturation=0.5, brightness=d, sat_first=1)[0, 0].tolist()
    b = _one(_tile((250, 100, 100)), saturation=0.5, brightness=d, sat_first=0)[0, 0].tolist()
    assert a == [255, 207, 207] and b == [255, 194, 194]


def test_reference_audio_known_answers():
    rows = np.zeros((3, 16), np.int16)
    rows[0, :4] = [100, -50, 7, -7]
    rows[1, 0] = -32768
    out, gains = R.augment_audio(rows, [0.0, 0.5, 0.999])
    assert gains[0] == 1 + (-0.1 + (0.1 - -0.1) * 0.0) == 0.9
    assert out[0, :4].tolist() == [90, -45, 6, -6]                                         # truncation towards zero
    assert gains[1] == 1 + (-0.1 + 0.1 * 0.5) and out[1, 0] == int(-32768 * gains[1])      # peak 32768: max_gain = 0
    assert gains[2] == 1 + (-0.1 + 0.2 * 0.999) and not out[2].any()                       # silence: max_gain = 0.1


# ---- AugmentingFeed ----------------------------------------------------------------------------------------------------------
def _batches(n, b=6):
    rs = np.random.RandomState(1)
    return [([rs.randint(0, 256, (b, 224, 224, 3)).astype(np.uint8), rs.randint(-9, 9, (b, 1, 48)).astype(np.int16)],
             rs.randint(0, 2, (b, 2))) for _ in range(n)]


def test_augmenting_feed_passes_batches_through_and_is_reproducible():
    src = _batches(3)
    a = list(augment.AugmentingFeed(iter(src), 9))
    b = list(augment.AugmentingFeed(iter(src), 9))
    c = list(augment.AugmentingFeed(iter(src), 10))
    rng = random.Random(9)
    for (x, y), (xa, ya), (xb, _), (xc, _) in zip(src, a, b, c):
        assert isinstance(xa, list) and len(xa) == 2 and xa[0] is x[0] and xa[1] is x[1] and ya is y
        assert np.array_equal(xa.augment, augment.draw_params(rng, 6))                    # one stream over the batches
        assert np.array_equal(xa.augment, xb.augment) and not np.array_equal(xa.augment, xc.augment)
        assert not hasattr(xa, 'global_batch')


def test_augmenting_feed_draws_for_the_global_batch_of_a_sharded_feed():
    from l3embedding_amd.blobfeed import ShardedInputs
    (x, y), = _batches(1, b=2)
    (xa, _), = list(augment.AugmentingFeed(iter([(ShardedInputs(x, 7), y)]), 4))
    assert xa.global_batch == 7 and len(xa.augment) == 7
    assert np.array_equal(xa.augment, augment.draw_params(random.Random(4), 7))


class _Dist(object):
    def __init__(self, rank):
        self.rank = rank

    def get_rank(self):
        return self.rank


@pytest.mark.parametrize('world', [2, 3])
def test_data_parallel_slices_params_with_the_rows_bounds(world, monkeypatch):
    (x, y), = _batches(1, b=7)
    params = augment.draw_params(random.Random(2), 7)
    m = L3Model.__new__(L3Model)
    m.replicas = world
    seen = []
    for rank in range(world):
        monkeypatch.setattr(m, '_dist', lambda rank=rank: _Dist(rank), raising=False)
        lo, hi = get_slice_bounds(7, world, rank)
        v, a, l, gb = m._split(augment.AugmentedInputs(x, params), y)
        got = m._split_augment(augment.AugmentedInputs(x, params))
        assert gb == 7 and np.array_equal(v, x[0][lo:hi]) and np.array_equal(got, params[lo:hi]) and len(got) == len(v)
        seen.append(got)
    assert np.array_equal(np.concatenate(seen), params)
    m.replicas = 1
    assert m._split_augment(augment.AugmentedInputs(x, params)) is params and m._split_augment(x) is None


# ---- train_augmented ---------------------------------------------------------------------------------------------------------
class _StubModel(object):
    """Stands in for the engine-backed model: records what fit_generator was handed."""

    def __init__(self):
        self.train_batches = self.validation_batches = None

    def compile(self, *a, **k):
        pass

    def get_config(self):
        return {}

    def to_json(self):
        return '{}'

    def save_weights(self, path, overwrite=True):
        open(path, 'wb').close()

    def fit_generator(self, generator, steps_per_epoch, epochs=1, validation_data=None, **_):
        self.train_batches = [next(generator) for _ in range(2)]
        self.validation_batches = [next(validation_data)]
        from l3embedding_amd.model import History
        return History()


def _blob_dir(path, rows=8):
    from l3embedding_amd import h5lite
    os.makedirs(path)
    rs = np.random.RandomState(0)
    root = h5lite.Group()
    root.create_dataset('audio', rs.randint(-99, 99, (rows, 1, 48)).astype(np.int16))
    root.create_dataset('video', rs.randint(0, 256, (rows, 224, 224, 3)).astype(np.uint8))
    root.create_dataset('label', np.stack([np.arange(rows) % 2, 1 - np.arange(rows) % 2], 1).astype(np.int64))
    h5lite.write_file(os.path.join(path, 'blob.h5'), root)
    return path


def test_train_augmented_config_and_feeds(tmp_path, monkeypatch):
    stub = _StubModel()
    monkeypatch.setitem(T.MODELS, 'tiny_L3', lambda num_gpus=0: (stub, None, None))
    tr, va = _blob_dir(str(tmp_path / 'set_train')), _blob_dir(str(tmp_path / 'set_valid'))
    kw = dict(num_epochs=1, train_epoch_size=2, validation_epoch_size=1, train_batch_size=4, validation_batch_size=4,
              model_type='tiny_L3', disable_logging=True)
    T.train_augmented(tr, va, str(tmp_path / 'out_aug'), augment_random_state=77, **kw)
    rng = random.Random(77)
    for x, y in stub.train_batches:
        assert np.array_equal(x.augment, augment.draw_params(rng, 4)) and x[0].dtype == np.uint8 and len(y) == 4
    assert not hasattr(stub.validation_batches[0][0], 'augment')                           # validation is never augmented
    T.train(tr, va, str(tmp_path / 'out_plain'), **kw)
    assert not hasattr(stub.train_batches[0][0], 'augment')

    def config(out):
        (path,) = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path / out)) for f in fs if f == 'config.json']
        with open(path) as fh:
            return json.load(fh)
    aug, plain = config('out_aug'), config('out_plain')
    assert aug['augment'] is True and aug['augment_random_state'] == 77
    assert 'augment' not in plain and 'augment_random_state' not in plain
    assert set(aug) - set(plain) == {'augment', 'augment_random_state'} and set(plain) <= set(aug)
    assert set(plain) == set(inspect.signature(T.train).parameters) | {'username', 'model_id', 'model_dir', 'git_commit', 'backend'}
    assert plain['train_batch_size'] == aug['train_batch_size'] == 4 and plain['num_epochs'] == 1
    with pytest.raises(TypeError, match='bogus'):
        T.train_augmented(tr, va, str(tmp_path / 'x'), bogus=1)


def test_cli_flags():
    from l3embedding_amd import cli_train
    args = cli_train.parse_arguments(['--augment', '--augment-random-state', '5', 'a_train', 'b', 'c'])
    assert args['augment'] is True and args['augment_random_state'] == 5
    args = cli_train.parse_arguments(['a_train', 'b', 'c'])
    assert args['augment'] is False and args['augment_random_state'] == 20180123
