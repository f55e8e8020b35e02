"""Host-side mirror of l3embedding/model.py (+ the constructors of audio_model.py and
vision_model.py) on top of libl3hip.so.

Same names, argument meaning and error behaviour as the reference so that callers
(train.py:263-267, 05_generate_embedding_samples.py:153-157) can switch imports:

    MODELS[model_type](num_gpus=...) -> (model, [x_i, x_a], y)     model.py:184-195,307-313
    load_model(weights_path, model_type, src_num_gpus, tgt_num_gpus, return_io)   model.py:85-128
    load_embedding(weights_path, model_type, embedding_type, pooling_type, ...)   model.py:131-181
    convert_num_gpus(...)                                                         model.py:38-82

The model object speaks the slice of the Keras protocol those callers use: compile,
fit_generator, train_on_batch, test_on_batch, predict, get_weights/set_weights,
save_weights/load_weights, get_layer, layers, summary, to_json, name.
All arithmetic runs in the HIP library; there is no CPU compute path here.
"""
import json
from collections import OrderedDict

import os

import numpy as np

from . import _lib
from . import kerasfile
from .training_utils import get_slice_bounds

MODEL_TYPES = ('cnn_L3_orig', 'tiny_L3', 'cnn_L3_kapredbinputbn', 'cnn_L3_melspec1', 'cnn_L3_melspec2')

# audio_model.py:461-478
AUDIO_POOLING = {
    'cnn_L3_orig': {'original': (8, 8), 'short': (32, 24)},
    'cnn_L3_kapredbinputbn': {'original': (8, 8), 'short': (32, 24)},
    'cnn_L3_melspec1': {'original': (4, 8), 'short': (16, 24)},
    'cnn_L3_melspec2': {'original': (8, 8), 'short': (32, 24)},
}
VISION_POOLING = (7, 7)   # vision_model.py:212
# (H, W, C) of the audio embedding layer's convolution output, which MaxPooling2D(pool, padding='same') pools: the 'short' pooling
# is the pool over all of it
AUDIO_EMBEDDING_MAP = {mt: pools['short'] + (512,) for mt, pools in AUDIO_POOLING.items()}


class Input(object):
    """Placeholder for keras.layers.Input (audio_model.py:363, vision_model.py:123)."""

    def __init__(self, shape, dtype='float32', name=None):
        self.shape = (None,) + tuple(shape)
        self.dtype = dtype
        self.name = name


class Adam(object):
    """keras.optimizers.Adam as used at train.py:282 (beta_1 .9, beta_2 .999, eps 1e-8)."""

    def __init__(self, lr=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-8, decay=0.0):
        if (beta_1, beta_2, epsilon, decay) != (0.9, 0.999, 1e-8, 0.0):
            raise ValueError('only the keras-default Adam moments used by the reference are implemented')
        self.lr = float(lr)


class History(object):
    def __init__(self):
        self.history = {}
        self.epoch = []


class Layer(object):
    def __init__(self, name, model, tap=None):
        self.name = name
        self._model = model
        self.output = tap      # symbolic handle of the layer's output tensor


class SubModel(object):
    """'vision_model' / 'audio_model' nested models (vision_model.py:193, audio_model.py:440)."""

    def __init__(self, parent, prefix):
        self.name = prefix
        self._parent = parent

    def _names(self):
        return [n for n, _, _ in self._parent.param_table() if n.startswith(self.name + '/')]

    def get_layer(self, name):
        if not any(n.split('/')[1] == name for n in self._names()):
            raise ValueError('No such layer: ' + name)
        return Layer(name, self, tap=(self.name, name))

    def get_weights(self):
        W = self._parent._weights_dict()
        return [W[n] for n in self._names()]

    def set_weights(self, ws):
        names = self._names()
        if len(ws) != len(names):
            raise ValueError('expected %d weight arrays, got %d' % (len(names), len(ws)))
        self._parent._assign(OrderedDict(zip(names, ws)))

    def count_params(self):
        return int(sum(int(np.prod(s)) for n, s, _ in self._parent.param_table() if n.startswith(self.name + '/')))


def _host_param_table(model_type):
    """(name, shape, trainable) in the library's ledger order (layer by layer), without needing a GPU.
    Kept in lock-step with engine.hip:build_ledger (checked against the library on GPU)."""
    tab = []
    cnt = {'conv': 0, 'bn': 0}

    def conv(prefix, name, cin, cout, k):
        tab.append(('%s/%s/kernel' % (prefix, name), (k, k, cin, cout), True))
        tab.append(('%s/%s/bias' % (prefix, name), (cout,), True))

    def bn(prefix, c):
        cnt['bn'] += 1
        b = '%s/batch_normalization_%d' % (prefix, cnt['bn'])
        tab.extend([(b + '/gamma', (c,), True), (b + '/beta', (c,), True),
                    (b + '/moving_mean', (c,), False), (b + '/moving_variance', (c,), False)])

    def vgg(prefix, cin, emb):
        c = cin
        for bi, f in enumerate((64, 128, 256, 512)):
            for ci in range(2):
                if bi == 3 and ci == 1:
                    name = emb
                else:
                    cnt['conv'] += 1
                    name = 'conv2d_%d' % cnt['conv']
                conv(prefix, name, c, f, 3)
                bn(prefix, f)
                c = f

    def tiny(prefix, cin):
        c = cin
        for _ in range(3):
            cnt['conv'] += 1
            conv(prefix, 'conv2d_%d' % cnt['conv'], c, 10, 5)
            bn(prefix, 10)
            c = 10

    fe = {'cnn_L3_orig': ('spectrogram_1', 512, 0), 'tiny_L3': ('spectrogram_1', 512, 0),
          'cnn_L3_kapredbinputbn': ('spectrogram_1', 512, 0), 'cnn_L3_melspec1': ('melspectrogram_1', 2048, 128),
          'cnn_L3_melspec2': ('melspectrogram_1', 2048, 256)}[model_type]
    inputbn = model_type not in ('cnn_L3_orig', 'tiny_L3')
    if model_type == 'tiny_L3':
        tiny('vision_model', 3)
    else:
        if inputbn:
            bn('vision_model', 3)
        vgg('vision_model', 3, 'vision_embedding_layer')
    nb = fe[1] // 2 + 1
    base = 'audio_model/' + fe[0]
    tab.append((base + '/real_kernels', (fe[1], 1, 1, nb), False))
    tab.append((base + '/imag_kernels', (fe[1], 1, 1, nb), False))
    if fe[2]:
        tab.append((base + '/freq2mel', (nb, fe[2]), False))
    if model_type == 'tiny_L3':
        tiny('audio_model', 1)
        feat, head = 360 + 350, 64
    else:
        if inputbn:
            bn('audio_model', 1)
        vgg('audio_model', 1, 'audio_embedding_layer')
        feat, head = 1024, 128
    tab.extend([('dense_1/kernel', (feat, head), True), ('dense_1/bias', (head,), True),
                ('dense_2/kernel', (head, 2), True), ('dense_2/bias', (2,), True)])
    return tab


class L3Model(object):
    """An AVC model bound (lazily) to an l3_engine.  `replicas` > 1 marks the model as
    the data-parallel wrapper of training_utils.multi_gpu_model."""

    def __init__(self, model_type, seed=20180123, device=0, db_max_scope='sample', bn_zero_debias=True, frontend='kapre'):
        if model_type not in MODEL_TYPES:
            raise ValueError('Invalid model type: "{}"'.format(model_type))
        if frontend not in _lib.FRONTENDS:
            raise ValueError('frontend must be one of %s' % sorted(_lib.FRONTENDS))
        # 'kapre': the layer the model was trained with; 'minispec': the deployed pipeline's spectrogram (inference only)
        self.frontend = frontend
        self.model_type = model_type
        self.name = model_type
        self.seed = seed
        self.device = device
        self.db_max_scope = db_max_scope
        # not in the reference (fp32 only): 'bf16' = mixed precision of BASELINE configs[4] -- bf16
        # operands / fp32 accumulate in the 3x3 convolutions (include/l3hip.h, l3_config.dtype)
        self.compute_dtype = os.environ.get('L3_DTYPE', 'f32')
        # fp32 convolution algorithm (include/l3hip.h L3_FP32_CONV_*): 'f4x4' Winograd F(4x4,3x3), the default;
        # 'f2x2' F(2x2,3x3) -- ~7x lower rounding error per layer, the step ~17 % slower
        self.fp32_conv = os.environ.get('L3_FP32_CONV', 'f4x4')
        # BatchNorm moving statistics under data parallelism (include/l3hip.h L3_DP_MOVING_*): 'replicas' = one moving-average update per
        # replica and step on every rank, as multi_gpu_model's per-replica model call produces them (training_utils.py:141-157), the
        # default; 'rank_local' = one update from the rank's own shard
        self.dp_moving = os.environ.get('L3_DP_MOVING', 'replicas')
        self._inflight = None
        self.bn_zero_debias = bn_zero_debias
        self.replicas = 1
        self.optimizer = None
        self.loss = None
        self.metrics_names = ['loss']
        self.stop_training = False
        self._engine = None             # the engine holding the model state (one per fed batch size in _engines)
        self._engines = {}
        self._host_weights = None       # OrderedDict when weights were assigned before an engine exists
        self._table = None
        self.inputs = [Input((224, 224, 3), name='input_1'), Input((1, 48000), name='input_2')]
        self.outputs = [Layer('dense_2', self, tap=('head', 'dense_2'))]

    # -- engine management ---------------------------------------------------------------------
    def param_table(self):
        if self._table is None:
            self._table = _host_param_table(self.model_type)
        return self._table

    serial = False       # replicas > 1: the replicas run one after another on this model's GPU (as_data_parallel(serial=True))
    MAX_ENGINES = 3      # engines kept alive at once (one per fed batch size; ~0.4 GB of HBM per pair of batch)

    def _ensure_engine(self, batch, global_batch=0):
        """The engine for this fed batch size.  Keras keeps one set of variables whatever batch is fed, so
        when the size changes (validation_batch_size != train_batch_size, a ragged last batch) the model
        state -- weights, Adam moments and step, BatchNorm debias accumulators -- moves to the engine of
        the new size device-to-device (`l3_copy_state`) instead of being rebuilt from the weights alone."""
        key = (int(batch), int(global_batch), self.compute_dtype, self.fp32_conv, self.frontend)
        cur = self._engine
        if cur is not None and cur._key == key:
            return cur
        e = self._engines.get(key)
        if e is None:
            stream = None
            if self.replicas > 1 and not self.serial:
                import torch
                if getattr(self, '_tstream', None) is None:
                    self._tstream = torch.cuda.Stream(device=self.device)
                stream = self._tstream.cuda_stream
            e = _lib.Engine(self.model_type, key[0], device=self.device, global_batch=key[1],
                            db_max_scope=self.db_max_scope, bn_zero_debias=self.bn_zero_debias, seed=self.seed,
                            stream=stream, dtype=self.compute_dtype, fp32_conv=self.fp32_conv, dp_moving=self.dp_moving,
                            frontend=self.frontend)
            e._key = key
            e._trainer = None
            lib_tab = [(n, tuple(s), t) for n, s, t in e.param_table()]
            if lib_tab != [(n, tuple(s), t) for n, s, t in self.param_table()]:
                raise RuntimeError('host ledger and libl3hip ledger disagree')
            for old_key in [k for k in self._engines if self._engines[k] is not cur][:max(0, len(self._engines) + 1 - self.MAX_ENGINES)]:
                self._engines.pop(old_key).close()
            self._engines[key] = e
        if cur is not None:
            e.copy_state_from(cur)
        elif self._host_weights is not None:
            e.set_params(self._host_weights)
        self._engine = e
        self._host_weights = None
        return e

    def set_frontend(self, frontend):
        """Switches the front-end form.  The weights stay; the engines, whose geometry depends on the form, are made anew."""
        if frontend not in _lib.FRONTENDS:
            raise ValueError('frontend must be one of %s' % sorted(_lib.FRONTENDS))
        if frontend == self.frontend:
            return
        held = OrderedDict(self._engine.get_params()) if self._engine is not None else self._host_weights
        self._drop_engines()
        self._host_weights = held
        self.frontend = frontend

    def _drop_engines(self):
        for e in self._engines.values():
            e.close()
        self._engines = {}
        self._engine = None

    def _weights_dict(self):
        if self._engine is not None:
            return self._engine.get_params()
        if self._host_weights is None:
            # need the library's initialisation (he_normal + kapre constants): make a batch-1 engine
            self._ensure_engine(1)
            return self._engine.get_params()
        return self._host_weights

    def _assign(self, named):
        if self._engine is not None:
            self._engine.set_params(named)
        else:
            if self._host_weights is None:
                self._host_weights = OrderedDict()
            for k, v in named.items():
                self._host_weights[k] = np.asarray(v, dtype=np.float32)
            # complete dict required before an engine exists
            missing = [n for n, _, _ in self.param_table() if n not in self._host_weights]
            if missing:
                self._ensure_engine(1)
                self._engine.set_params(named)

    # -- keras protocol ---------------------------------------------------------------------------
    @property
    def layers(self):
        vis, aud = SubModel(self, 'vision_model'), SubModel(self, 'audio_model')
        base = [Layer('input_1', self), Layer('input_2', self), vis, aud, Layer('concatenate_1', self),
                Layer('dense_1', self), Layer('dense_2', self)]
        if self.replicas > 1:
            # multi_gpu_model wrapper: [inputs, lambdas..., template model, concat] -- layers[-2] is the
            # template (model.py:77)
            return [Layer('input_1', self), Layer('input_2', self), self._template(), Layer('concatenate_1', self)]
        return base

    def _template(self):
        t = L3Model.__new__(L3Model)
        t.__dict__.update(self.__dict__)
        t.replicas = 1
        return t

    def get_layer(self, name):
        if name in ('vision_model', 'audio_model'):
            return SubModel(self, name)
        if name in ('dense_1', 'dense_2', 'concatenate_1'):
            return Layer(name, self, tap=('head', name))
        raise ValueError('No such layer: ' + name)

    def _weight_order(self):
        """[3P] keras `Model.get_weights()` order: layer by layer over the TOP-LEVEL layers, and a nested
        model's `.weights` lists all its trainable tensors before its non-trainable ones (the same order
        `save_weights` writes, kerasfile.keras_groups).  `get_layer('audio_model').get_weights()` -- a
        call on the sub-model itself -- is layer-interleaved instead (kapre's constants first:
        notebooks/extract_spectrogram_models_from_avc_models.ipynb:446); see SubModel.get_weights."""
        groups = kerasfile.keras_groups(self.param_table(), self.model_type, wrapper=self.replicas > 1)
        return [n for names in groups.values() for n in names]

    def get_weights(self):
        W = self._weights_dict()
        return [W[n] for n in self._weight_order()]

    def set_weights(self, ws):
        order = self._weight_order()
        shapes = {n: tuple(s) for n, s, _ in self.param_table()}
        if len(ws) != len(order):
            raise ValueError('You called `set_weights(weights)` on model "%s" with a weight list of length %d, '
                             'but the model was expecting %d weights.' % (self.name, len(ws), len(order)))
        named = OrderedDict()
        for n, w in zip(order, ws):
            w = np.asarray(w, dtype=np.float32)
            if tuple(w.shape) != shapes[n]:
                raise ValueError('Layer weight shape %s not compatible with provided weight shape %s (%s)' % (shapes[n], w.shape, n))
            named[n] = w
        self._assign(named)

    def count_params(self):
        return int(sum(int(np.prod(s)) for _, s, _ in self.param_table()))

    def save_weights(self, path, overwrite=True):
        """Written next to `path` and renamed onto it: a run killed mid-write leaves the previous
        `model_latest.h5` intact, and that is the file `continue_model_dir` resumes from."""
        if not overwrite and os.path.exists(path):
            raise IOError('"{}" exists and overwrite=False'.format(path))
        stem, ext = os.path.splitext(path)              # the extension picks the format (kerasfile.save_weights): keep it
        tmp = '%s.partial.%d%s' % (stem, os.getpid(), ext)
        try:
            kerasfile.save_weights(tmp, self._weights_dict(), self.param_table(), self.model_type,
                                   wrapper=self.replicas > 1)
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise

    def load_weights(self, path):
        named = kerasfile.load_weights(path, self.param_table(), self.model_type, wrapper=self.replicas > 1)
        self._assign(named)
        if self._engine is not None:
            self._engine.reset_optimizer()

    def to_json(self):
        return json.dumps({'class_name': 'Model', 'config': {'name': self.name, 'model_type': self.model_type,
                                                             'replicas': self.replicas,
                                                             'weights': [[n, list(s), t] for n, s, t in self.param_table()]},
                           'backend': 'libl3hip'})

    def get_config(self):
        return json.loads(self.to_json())['config']

    def summary(self, print_fn=print):
        tot = self.count_params()
        tr = int(sum(int(np.prod(s)) for _, s, t in self.param_table() if t))
        print_fn('Model "%s"' % self.name)
        for sub in ('vision_model', 'audio_model'):
            print_fn('  %-14s (Model)  (None, %d)   %d' % (sub, 512 if self.model_type != 'tiny_L3' else (360 if sub[0] == 'v' else 350),
                                                           SubModel(self, sub).count_params()))
        for d in ('dense_1', 'dense_2'):
            print_fn('  %-14s (Dense)  %d' % (d, sum(int(np.prod(s)) for n, s, _ in self.param_table() if n.startswith(d + '/'))))
        print_fn('Total params: {:,}'.format(tot))
        print_fn('Trainable params: {:,}'.format(tr))
        print_fn('Non-trainable params: {:,}'.format(tot - tr))

    def compile(self, optimizer, loss='categorical_crossentropy', metrics=None):
        if loss != 'categorical_crossentropy':
            raise ValueError('only categorical_crossentropy (train.py:270) is implemented')
        if isinstance(optimizer, str):
            if optimizer.lower() != 'adam':
                raise ValueError('only Adam (train.py:282) is implemented')
            optimizer = Adam()
        self.optimizer = optimizer
        self.loss = loss
        self.metrics_names = ['loss'] + (['acc'] if metrics and ('accuracy' in metrics or 'acc' in metrics) else [])

    def as_data_parallel(self, gpus, serial=False):
        """serial=True: the `gpus` replicas of multi_gpu_model (training_utils.py:121-170) run one after another on this model's
        GPU, in this process (Engine.step_replicas): no torch.distributed, any number of devices.  A fed batch is cut into `gpus`
        equal slices; a batch that does not divide is refused (the reference would give the last replica the remainder)."""
        import os
        self.replicas = int(gpus)
        self.serial = bool(serial)
        if not self.serial:
            self.device = int(os.environ.get('LOCAL_RANK', self.device))     # one process per GPU
        if self._engine is not None:
            self._host_weights = self._engine.get_params()
            self._drop_engines()
        return self

    def _dist(self):
        import torch.distributed as dist
        if not dist.is_available() or not dist.is_initialized():
            raise RuntimeError('a %d-replica model needs torch.distributed initialised with one process per GPU '
                               '(python -m torch.distributed.run --nproc-per-node %d ...)' % (self.replicas, self.replicas))
        if dist.get_world_size() != self.replicas:
            raise ValueError('model has %d replicas but the process group has %d ranks' % (self.replicas, dist.get_world_size()))
        return dist

    def _split(self, x, y=None):
        """[video, audio] (+ labels) -> this rank's shard (training_utils.py:121-133)."""
        v, a = x
        if self.replicas <= 1 or self.serial:       # serial replicas: the whole batch goes to the one engine, which cuts it
            return v, a, y, len(v)
        dist = self._dist()
        if getattr(x, 'global_batch', None):       # blobfeed.ShardedInputs: the feed already read only this rank's rows
            lo, hi = get_slice_bounds(x.global_batch, self.replicas, dist.get_rank())
            if len(v) != hi - lo:
                raise ValueError('rank %d expected %d rows of a %d-row batch, got %d' % (dist.get_rank(), hi - lo,
                                                                                     x.global_batch, len(v)))
            return v, a, y, x.global_batch
        lo, hi = get_slice_bounds(len(v), self.replicas, dist.get_rank())
        return v[lo:hi], a[lo:hi], (None if y is None else y[lo:hi]), len(v)

    def _split_augment(self, x):
        """This rank's rows of the augmentation parameters a training batch carries (augment.AugmentedInputs; None for a plain
        batch).  The rows are those of the global batch, cut with the bounds `_split` cuts the arrays with."""
        params = getattr(x, 'augment', None)
        if params is None or self.replicas <= 1 or self.serial:
            return params
        lo, hi = get_slice_bounds(len(params), self.replicas, self._dist().get_rank())
        return params[lo:hi]

    def _serial_slice(self, n):
        """Rows per replica of an n-row batch fed to a serial-replica model."""
        if n % self.replicas:
            raise ValueError('a batch of %d rows does not divide over %d serial replicas: the reference would give the last '
                             'replica the remainder (training_utils.py:121-133), serial replicas take equal slices only'
                             % (n, self.replicas))
        return n // self.replicas

    @staticmethod
    def _is_raw(v, a):
        """uint8 frames + int16 PCM as stored in the HDF5 blobs (data/avc/sample.py:371-377)."""
        v, a = np.asarray(v), np.asarray(a)
        if v.dtype == np.uint8 and a.dtype == np.int16:
            return True
        if v.dtype == np.uint8 or a.dtype == np.int16:
            raise ValueError('raw batches need uint8 video AND int16 audio')
        return False

    def _feed(self, e, v, a, l, aug=None, stage=False):
        """How a split batch reaches the engine: raw (stored dtypes straight to the GPU; the scaling of train.py:186,189 happens
        there, bit-exact) or float, with the augmentation records of data/avc/sample.py:146-162,241-281 or without, as the global
        batch of serial replicas or as this rank's own, uploaded now or staged behind the running step."""
        raw = self._is_raw(v, a)
        if aug is not None and not raw:
            raise ValueError('only raw batches (uint8 video, int16 audio) can be augmented: the arithmetic of '
                             'data/avc/sample.py is defined on the stored dtypes')
        serial = self.replicas > 1 and self.serial
        if not raw:
            return e.replicas_upload(v, a, l, self.replicas) if serial else e.upload_batch(v, a, l)
        if serial:
            name, tail = 'replicas_stage_raw' if stage else 'replicas_upload_raw', (self.replicas,)
        else:
            name, tail = 'stage_batch_raw' if stage else 'upload_batch_raw', ()
        records = () if aug is None else (aug, aug['u_gain'])
        return getattr(e, name + ('_aug' if records else ''))(v, a, np.asarray(l).astype(np.int32), *(records + tail))

    def _sampled_engine(self, x):
        """The engine for a batch that carries sample records in place of arrays (avsample.SampledInputs; None for any other
        batch): the engine cuts such a batch itself from the bank's clips.  Data-parallel and serial replicas are out of scope."""
        if getattr(x, 'sample_records', None) is None:
            return None
        if self.replicas > 1:
            raise ValueError('a sampled batch (avsample.SampledInputs) cannot be fed to a %d-replica model: the engine builds it '
                             'whole on one GPU' % self.replicas)
        return self._ensure_engine(len(x.sample_records))

    def train_on_batch(self, x, y):
        self._launch_train(x, y, staged=False)
        return self._finish_train()

    def _launch_train(self, x, y, staged):
        """Enqueues one training step (returns without waiting for the device).  staged: the batch was
        already sent with Engine.stage_batch_raw() and is adopted by the step."""
        if self.optimizer is None:
            raise RuntimeError('You must compile a model before training/testing. Use `model.compile(optimizer, loss)`.')
        e = self._sampled_engine(x)
        if e is not None:
            if not staged:
                e.upload_batch_sampled(x.bank, x.sample_records, x.augmented)
            e.step_resident(self.optimizer.lr)
            self._inflight = (e, len(x), len(x))
            return
        v, a, l, gb = self._split(x, y)
        aug = self._split_augment(x)
        if self.replicas > 1 and self.serial:
            e = self._ensure_engine(self._serial_slice(len(v)), global_batch=gb)
            if not staged:
                self._feed(e, v, a, l, aug)
            e.step_replicas(self.optimizer.lr)
            self._inflight = (e, len(v), gb)
            return
        dp = self.replicas > 1
        e = self._ensure_engine(len(v), global_batch=gb if dp else 0)
        if dp and e._trainer is None:
            # L3_DP_COMM=native (default): RCCL inside libl3hip (l3_comm_init / l3_step_dp);
            # L3_DP_COMM=torch: bucketed torch.distributed all-reduce driven from Python (the test double)
            from .training_utils import DataParallelTrainer, NativeDataParallelTrainer
            if os.environ.get('L3_DP_COMM', 'native') == 'native' and self._dist().get_backend() == 'nccl':
                e._trainer = NativeDataParallelTrainer(e, self.replicas, self._dist().get_rank())
            else:
                e._trainer = DataParallelTrainer(e, self.device, self.replicas, self._dist().get_rank(), stream=self._tstream)
        if not staged:
            self._feed(e, v, a, l, aug)
        if dp:
            e._trainer.step(self.optimizer.lr)
        else:
            e.step_resident(self.optimizer.lr)
        self._inflight = (e, len(v), gb)

    def _defer_results(self):
        """The launched step's loss / accuracy go to a pinned slot behind it (Engine.results_enqueue): returns the handle
        `_finish_deferred` takes, or None where results cannot be deferred (engines without the entry point; the torch.distributed
        double of the exchange).  Data parallel over the library's communicator: the sums are added up over the ranks on the device,
        so the values are those of the concatenated batch (training_utils.py:165-170)."""
        e, n_local, gb = self._inflight
        if not hasattr(e, 'results_enqueue'):
            return None
        reduce = self.replicas > 1 and not self.serial      # (serial replicas: the engine has summed its slices itself)
        if reduce and not getattr(e._trainer, 'reduces_results', False):
            return None          # the torch.distributed double: the ranks' values are reduced by _finish_train
        slot = self._res_slot = 1 - getattr(self, '_res_slot', 1)
        e.results_enqueue(slot, reduce=reduce)
        return (e, slot)

    @staticmethod
    def _finish_deferred(handle):
        e, slot = handle
        return list(e.results_wait(slot))

    def _stage_next(self, x, y):
        """Sends the next (raw) batch to the device while the launched step runs.  False if it cannot be staged."""
        if self._inflight is None:
            return False
        e, n_local, _ = self._inflight
        if getattr(x, 'sample_records', None) is not None:
            if len(x) != n_local or self.replicas > 1:
                return False
            e.stage_batch_sampled(x.bank, x.sample_records, x.augmented)
            return True
        v, a, l, _ = self._split(x, y)
        if len(v) != n_local or not self._is_raw(v, a):
            return False
        self._feed(e, v, a, l, self._split_augment(x), stage=True)
        return True

    def _finish_train(self):
        e, n_local, gb = self._inflight
        self._inflight = None
        loss, acc = e.step_results()
        if self.replicas <= 1 or self.serial:
            return [loss, acc]
        import torch
        # logged loss/acc are over the concatenated batch (training_utils.py:165-170)
        t = torch.tensor([loss * n_local, acc * n_local], dtype=torch.float64, device='cuda:%d' % self.device)
        self._dist().all_reduce(t)
        return [float(t[0].item()) / gb, float(t[1].item()) / gb]

    def test_on_batch(self, x, y):
        v, a, l, gb = self._split(x, y)
        if self.replicas > 1 and self.serial:
            e = self._ensure_engine(self._serial_slice(len(v)), global_batch=gb)
            self._feed(e, v, a, l)
            return list(e.eval_replicas())
        e = self._ensure_engine(len(v), global_batch=gb if self.replicas > 1 else 0)
        self._feed(e, v, a, l)
        e.step_forward(training=False)
        loss, acc = e.step_results()
        if self.replicas > 1:
            import torch
            dist = self._dist()
            t = torch.tensor([loss * len(v), acc * len(v)], dtype=torch.float64, device='cuda:%d' % self.device)
            dist.all_reduce(t)
            loss, acc = float(t[0].item()) / gb, float(t[1].item()) / gb
        return [loss, acc]

    def predict(self, x, batch_size=32, verbose=0):
        v, a = x
        n = len(v)
        e = self._ensure_engine(min(batch_size, n) if self._engine is None else self._engine.batch)
        B = e.batch
        out = np.empty((n, 2), np.float32)
        for s in range(0, n, B):
            cnt = min(B, n - s)
            vb = np.zeros((B, 224, 224, 3), np.float32)
            ab = np.zeros((B, 1, 48000), np.float32)
            vb[:cnt], ab[:cnt] = v[s:s + cnt], a[s:s + cnt]
            p, _ = e.forward(vb, ab, training=False)
            out[s:s + cnt] = p[:cnt]
        return out

    def predict_logits(self, x, training=False):
        """Pre-softmax activations of dense_2 (the quantity the 1e-3 parity bar is stated on)."""
        v, a = x
        e = self._ensure_engine(len(v))
        return e.forward(v, a, training=training)[1]

    def predict_towers(self, video=None, audio=None, batch_size=32, to_device=False):
        """The two towers' flattened outputs, each from its tower alone (inference-mode BatchNorm): video (Nv, 224, 224, 3) ->
        V (Nv, nv), audio (Na, 1, 48000) -> A (Na, na), the halves of the concatenate input (model.py:25) that
        crossmodal.PairScorer scores pair by pair.  Either input may be None (its output is None); Nv and Na need not be equal.
        The engine is chosen as predict chooses it.  to_device: usc.DeviceFeatures, which the caller owns and closes."""
        if video is None and audio is None:
            raise ValueError('give video, audio or both')
        ins = [None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (video, audio)]
        for x, name in zip(ins, ('video', 'audio')):
            if x is not None and len(x) == 0:
                raise ValueError('%s has no rows' % name)
        n = max(len(x) for x in ins if x is not None)
        e = self._ensure_engine(max(1, min(batch_size, n)) if self._engine is None else self._engine.batch)
        outs = []
        for tower, x in enumerate(ins):
            if x is None:
                outs.append(None)
            elif to_device:
                from . import usc
                dst = _lib.Features.alloc(len(x), e.tower_dim(tower), device=self.device)
                e.tower_features(tower, x, dst=dst)
                outs.append(usc.DeviceFeatures.from_handle(dst))
            else:
                outs.append(e.tower_features(tower, x))
        return tuple(outs)

    def predict_locations(self, video=None, audio=None, batch_size=32):
        """The two towers' last feature maps before their global max pool, location by location: for each input that
        is given, (usc.DeviceFeatures of n L rows x C channels, (H, W)) with L = H W and item i's locations in rows [i L, (i + 1) L),
        y first -- what crossmodal.PairScorer.set_maps projects; None for an input that is None.  The maximum over an item's rows is
        its row of predict_towers, bit for bit.  The caller owns and closes the DeviceFeatures.  ValueError for a model whose last
        pool does not reduce to 1 x 1 (tiny_L3's vision tower)."""
        if video is None and audio is None:
            raise ValueError('give video, audio or both')
        ins = [None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (video, audio)]
        for x, name in zip(ins, ('video', 'audio')):
            if x is not None and len(x) == 0:
                raise ValueError('%s has no rows' % name)
        n = max(len(x) for x in ins if x is not None)
        e = self._ensure_engine(max(1, min(batch_size, n)) if self._engine is None else self._engine.batch)
        from . import usc
        outs = []
        for tower, x in enumerate(ins):
            if x is None:
                outs.append(None)
                continue
            H, W, _ = e.tower_locations_shape(tower)
            outs.append((usc.DeviceFeatures.from_handle(e.tower_locations(tower, x)), (H, W)))
        return tuple(outs)

    def fit_generator(self, generator, steps_per_epoch, epochs=1, verbose=1, callbacks=None, validation_data=None,
                      validation_steps=None, initial_epoch=0, **_):
        """keras fit_generator loop as driven by train.py:408-414: per step train_on_batch, per
        epoch validation (inference-mode BN) and callbacks with logs {loss, acc, val_loss, val_acc}."""
        callbacks = list(callbacks or [])
        hist = History()
        for cb in callbacks:
            if hasattr(cb, 'set_model'):
                cb.set_model(self)
            else:
                cb.model = self
            if hasattr(cb, 'set_params'):
                cb.set_params({'epochs': epochs, 'steps': steps_per_epoch, 'verbose': verbose,
                               'do_validation': validation_data is not None, 'metrics': ['loss', 'acc', 'val_loss', 'val_acc']})
        for cb in callbacks:
            cb.on_train_begin({})
        self.stop_training = False
        max_queue_size = int(_.get('max_queue_size', 10))
        prefetchers = []
        if max_queue_size > 0:
            generator = _Prefetcher(generator, max_queue_size)
            prefetchers.append(generator)
            if validation_data is not None and hasattr(validation_data, '__next__'):
                validation_data = _Prefetcher(validation_data, max_queue_size)
                prefetchers.append(validation_data)
        try:
            return self._fit_loop(generator, steps_per_epoch, epochs, verbose, callbacks, validation_data,
                                  validation_steps, initial_epoch, hist)
        finally:
            for pf in prefetchers:
                pf.close()

    def _fit_loop(self, generator, steps_per_epoch, epochs, verbose, callbacks, validation_data, validation_steps,
                  initial_epoch, hist):
        for epoch in range(initial_epoch, epochs):
            for cb in callbacks:
                cb.on_epoch_begin(epoch, {})
            sl = sa = 0.0
            seen = 0
            pending = None      # batch fetched (and staged on the device) during the previous step
            late = None         # (step, size, handle): a step whose results are read after the NEXT step has been enqueued

            def batch_end(step, n, loss, acc):
                nonlocal sl, sa, seen
                sl += loss * n
                sa += acc * n
                seen += n
                for cb in callbacks:
                    cb.on_batch_end(step, {'batch': step, 'size': n, 'loss': loss, 'acc': acc})

            # Reading step k's results after step k + 1 has been enqueued moves the batch hooks relative to the computation:
            # begin(k) fires after step k is launched, and end(k) -- with the model already one step further -- after step k + 1 is.
            # That is invisible to hooks that only look at `logs` or the clock (the reference's own: train.py:85-131), and wrong
            # for one that sets the learning rate in on_batch_begin or saves weights in on_batch_end.  So the pipelined order is
            # taken only when every callback either leaves both batch hooks alone or declares them passive
            # (`batch_hooks_are_passive = True`, as callbacks.TimeHistory does); otherwise Keras' order holds against the
            # computation too: begin(k), step k, end(k).
            pipelined = all(_batch_hooks_passive(cb) for cb in callbacks)
            for step in range(steps_per_epoch):
                (bx, by), staged = pending if pending is not None else (next(generator)[:2], False)
                pending = None
                n = len(by)
                if not pipelined:
                    for cb in callbacks:
                        cb.on_batch_begin(step, {'batch': step, 'size': n})
                # launch, then use the device time to pull and send the next batch (never across the
                # epoch boundary: validation uploads its own batches in between)
                self._launch_train(bx, by, staged)
                handle = self._defer_results() if pipelined else None
                # the GPU now holds this step; the step before it is read (and its callbacks run) while this one computes, so the
                # device never waits for the host between steps.  Callback order is Keras': end(k - 1) before begin(k).
                if late is not None:
                    batch_end(late[0], late[1], *self._finish_deferred(late[2]))
                    late = None
                if pipelined:
                    for cb in callbacks:
                        cb.on_batch_begin(step, {'batch': step, 'size': n})
                if step + 1 < steps_per_epoch:
                    nxt = next(generator)[:2]
                    pending = (nxt, self._stage_next(*nxt))
                if handle is None:
                    batch_end(step, n, *self._finish_train())
                else:
                    late = (step, n, handle)
            if late is not None:
                self._inflight = None
                batch_end(late[0], late[1], *self._finish_deferred(late[2]))
            logs = {'loss': sl / max(seen, 1), 'acc': sa / max(seen, 1)}
            if validation_data is not None:
                vl = va = 0.0
                vseen = 0
                for _ in range(validation_steps):
                    bx, by = next(validation_data)[:2]
                    l_, a_ = self.test_on_batch(bx, by)
                    vl += l_ * len(by)
                    va += a_ * len(by)
                    vseen += len(by)
                logs['val_loss'] = vl / max(vseen, 1)
                logs['val_acc'] = va / max(vseen, 1)
            for k, v_ in logs.items():
                hist.history.setdefault(k, []).append(v_)
            hist.epoch.append(epoch)
            if verbose:
                print('Epoch %d/%d - ' % (epoch + 1, epochs) + ' - '.join('%s: %.4f' % kv for kv in sorted(logs.items())))
            for cb in callbacks:
                cb.on_epoch_end(epoch, logs)
            if self.stop_training:
                break
        for cb in callbacks:
            cb.on_train_end({})
        return hist


def _batch_hooks_passive(cb):
    """True if `cb` leaves on_batch_begin / on_batch_end at the base class's no-ops or declares them passive (they only read
    `logs` / the clock: nothing that depends on WHEN they run relative to the step's computation)."""
    if getattr(cb, 'batch_hooks_are_passive', False):
        return True
    from .callbacks import Callback
    for name in ('on_batch_begin', 'on_batch_end'):
        f = getattr(type(cb), name, None)
        if f is not None and f is not getattr(Callback, name):
            return False
    return True


class _Prefetcher(object):
    """[3P] keras.utils.GeneratorEnqueuer as fit_generator uses it (workers=1, max_queue_size=10):
    ONE background thread pulls batches from the Python generator into a bounded queue, so HDF5
    decoding overlaps the device step.  Order is the generator's order; an exception in the
    generator is re-raised in the consumer."""

    _END = object()

    def __init__(self, generator, max_queue_size=10):
        import queue
        import threading
        self._q = queue.Queue(maxsize=max_queue_size)
        self._stop = threading.Event()
        self._gen = generator
        self._thread = threading.Thread(target=self._run, name='l3-prefetch', daemon=True)
        self._thread.start()

    def _put(self, item):
        import queue
        while not self._stop.is_set():
            try:
                self._q.put(item, timeout=0.1)
                return True
            except queue.Full:
                continue
        return False

    def _run(self):
        try:
            for item in self._gen:
                if not self._put(item) or self._stop.is_set():
                    return
            self._put(self._END)
        except BaseException as exc:            # delivered to the consumer
            self._put(exc)

    def __iter__(self):
        return self

    def __next__(self):
        item = self._q.get()
        if item is self._END:
            raise StopIteration
        if isinstance(item, BaseException):
            raise item
        return item

    def close(self):
        """Stops the thread.  The caller's generator stays usable, as with Keras (a second fit_generator on the same
        generator continues where the queue stopped pulling); whoever made the feed closes it (train.train())."""
        import queue
        self._stop.set()
        try:                                    # a producer blocked on the full queue leaves at once instead of at its next poll
            while True:
                self._q.get_nowait()
        except queue.Empty:
            pass
        self._thread.join(timeout=5.0)


class EmbeddingModel(object):
    """Output of load_embedding(): `.predict(x)` -> (N, D) embeddings (data/usc/features.py:304)."""

    def __init__(self, base, embedding_type, pool):
        self.base = base
        self.embedding_type = embedding_type
        self.pool = tuple(pool)
        self.name = 'model_embedding'

    def predict(self, x, batch_size=32, verbose=0):
        x = np.ascontiguousarray(x, dtype=np.float32)
        e = self.base._ensure_engine(self.base._engine.batch if self.base._engine is not None else max(1, min(batch_size, len(x))))
        if self.embedding_type == 'audio':
            return e.embed_audio(x, self.pool)
        return e.embed_vision(x, self.pool)

    # Caps of one l3_embed_audio_frames call of predict_clips (device memory held by a call: the samples, the frame table
    # and the pooled rows): at most CLIP_CALL_FRAMES frames and CLIP_CALL_SAMPLES samples (256 MiB of float32) -- or one
    # engine batch of frames, whatever its span, if that is more.  Larger inputs are split into several calls at engine-batch
    # boundaries of the frame list: between clips or inside one clip's frames.
    CLIP_CALL_FRAMES = 4096
    CLIP_CALL_SAMPLES = 1 << 26

    def predict_clips(self, clips, hop_length, batch_size=32, rates=None, to_device=False):
        """get_l3_frames_uniform's framing + predict for many clips at once (data/usc/features.py:276-306): clips is a
        sequence of 1-D float32 arrays at 48 kHz, hop_length the hop in samples.  Returns one (n_i, D) array per clip, n_i
        from features.frame_table.  The engine is chosen as predict chooses it (the model's current one, else batch
        min(batch_size, frames)).  Each clip is sent to the device once and cut into frames there.  Under
        db_max_scope = 'sample' the frames of consecutive clips share engine batches; under 'batch' (the dB maximum over
        an engine batch, kapre 0.1.3.1) every clip starts a new engine batch, so the batches are those of one predict call
        per clip.

        rates: clip i's sample rate (whole Hz) when the clips are not all at 48 kHz.  Each clip is then resampled to 48 kHz on
        the device as load_audio resamples it (resampy 'kaiser_best', features.py:25-26; a clip at 48 kHz is taken as it is),
        and the 48 kHz lengths are framed and packed exactly as above: the result equals predict_clips on the clips resampled
        by resample.resample.  A clip is uploaded at its own rate, once per call its frames reach.

        to_device: the rows stay on the engine's GPU.  Returns (usc.DeviceFeatures of all clips' rows in clip order, file_idxs),
        file_idxs (n_clips, 2) the row range [s, e) of each clip: the same rows in the same order from the same calls, written by
        the pooling kernel into the matrix (l3_embed_audio_frames_dev), the bits of the host form's np.concatenate.  The caller
        owns the DeviceFeatures and closes it."""
        from .features import frame_table
        if self.embedding_type != 'audio':
            raise TypeError('predict_clips needs an audio embedding model')
        clips = [np.asarray(c, dtype=np.float32) for c in clips]
        for c in clips:
            if c.ndim != 1:
                raise ValueError('every clip must be a 1-D array (got shape %s)' % (c.shape,))
        lengths = np.array([c.size for c in clips], np.int64)
        if rates is not None:
            from .resample import check_rates, get_filter, output_length
            win, num_table = get_filter('kaiser_best')
            rates = [check_rates(r, 48000)[0] for r in np.asarray(rates).reshape(-1).tolist()]
            if len(rates) != len(clips):
                raise ValueError('rates must give one rate per clip (%d rates, %d clips)' % (len(rates), len(clips)))
            native = lengths
            lengths = np.array([n if r == 48000 else output_length(int(n), r, 48000) for n, r in zip(native.tolist(), rates)],
                               np.int64)
        table, counts = frame_table(lengths, hop_length)
        if not clips:
            if to_device:
                raise ValueError('no clips: a device matrix has at least one row')
            return []
        total = int(counts.sum())
        e = self.base._ensure_engine(self.base._engine.batch if self.base._engine is not None else max(1, min(batch_size, total)))
        B = e.batch
        ends = np.cumsum(lengths)
        # rows of the engine's frame list: under 'batch' scope each clip padded to whole engine batches with empty frames
        if self.base.db_max_scope == 'sample':
            rows, row0 = table, np.concatenate([[0], np.cumsum(counts)[:-1]])
        else:
            padded = -(-counts // B) * B
            row0 = np.concatenate([[0], np.cumsum(padded)[:-1]])
            rows = np.empty((int(padded.sum()), 3), np.int64)
            rows[:] = np.repeat(ends, padded)[:, None]                  # empty frames at the clip's end: lo == hi
            first = np.concatenate([[0], np.cumsum(counts)[:-1]])
            for i in range(len(clips)):
                rows[row0[i]:row0[i] + counts[i]] = table[first[i]:first[i] + counts[i]]
        # samples each row reads: [a, b) -- ascending over the rows, so a call's rows read one contiguous stretch
        a = np.maximum(rows[:, 0], rows[:, 1])
        b = np.maximum(np.minimum(rows[:, 0] + 48000, rows[:, 2]), a)
        b = np.maximum.accumulate(b)
        D = int(e.lib.l3_embed_dim(e.h, 0, self.pool[0], self.pool[1]))
        if to_device:
            from . import usc
            out = _lib.Features.alloc(len(rows), D, device=self.base.device)
            where = lambda lo, hi: dict(dst=out, row0=lo)
        else:
            out = np.empty((len(rows), D), np.float32)
            where = lambda lo, hi: dict(out=out[lo:hi])
        max_frames = max(B, self.CLIP_CALL_FRAMES // B * B)
        offs = ends - lengths
        r0, n = 0, len(rows)
        while r0 < n:
            r1 = min(n, r0 + B)
            while r1 < n:
                r2 = min(n, r1 + B)
                if r2 - r0 > max_frames or b[r2 - 1] - a[r0] > self.CLIP_CALL_SAMPLES:
                    break
                r1 = r2
            base, top = int(a[r0]), int(b[r1 - 1])
            t = np.empty((r1 - r0, 3), np.int64)
            t[:, 0] = rows[r0:r1, 0] - base
            t[:, 1] = a[r0:r1] - base
            t[:, 2] = np.maximum(np.minimum(rows[r0:r1, 0] + 48000, rows[r0:r1, 2]), a[r0:r1]) - base
            if rates is None:
                e.embed_audio_frames(_clip_span(clips, offs, base, top), t, self.pool, **where(r0, r1))
            else:
                x, descs = _resample_rows(clips, rates, offs, lengths, base, top)
                e.embed_audio_clips_resampled(x, descs, win, num_table, top - base, t, self.pool, **where(r0, r1))
            r0 = r1
        if to_device:
            if len(rows) != total:          # 'batch' scope: the pad rows of every clip's last engine batch go
                out.gather(np.concatenate([np.arange(row0[i], row0[i] + counts[i]) for i in range(len(clips))]))
            return usc.DeviceFeatures.from_handle(out), usc._row_ranges(counts)
        return [out[row0[i]:row0[i] + counts[i]] for i in range(len(clips))]

    # Caps of one l3_embed_vision_frames call of predict_images (device memory held by a call: the pixels, the tables and the
    # pooled rows): at most IMAGE_CALL_FRAMES frames and IMAGE_CALL_BYTES of pixels -- or one engine batch, whatever its size, if
    # that is more.  Larger inputs are split into several calls at engine-batch boundaries.
    IMAGE_CALL_FRAMES = 4096
    IMAGE_CALL_BYTES = 1 << 28

    def spectrograms(self, clips, hop_length, batch_size=32, rates=None):
        """The front-end's output for every frame predict_clips would embed: (array (n, F, frames, 1) float32, counts), counts[i]
        the number of frames of clip i, framed as predict_clips frames them.  On a 'minispec' model this is the spectrogram the
        deployed pipeline computes per second; on a 'kapre' model the one the tower saw in training."""
        from .features import frame_table
        if self.embedding_type != 'audio':
            raise TypeError('spectrograms needs an audio embedding model')
        if self.base.db_max_scope != 'sample':
            raise ValueError("spectrograms needs db_max_scope = 'sample': under 'batch' a frame's values depend on its batch")
        clips = [np.asarray(c, dtype=np.float32).reshape(-1) for c in clips]
        if rates is not None:
            from .resample import resample
            clips = [c if int(r) == 48000 else np.asarray(resample(c, int(r), 48000), np.float32) for c, r in zip(clips, rates)]
        lengths = np.array([c.size for c in clips], np.int64)
        table, counts = frame_table(lengths, hop_length)
        total = int(counts.sum())
        e = self.base._ensure_engine(self.base._engine.batch if self.base._engine is not None else max(1, min(batch_size, total)))
        samples = np.concatenate(clips) if clips else np.zeros(0, np.float32)
        return e.audio_spectrograms(samples, table)[..., None], counts

    def predict_spectrograms(self, spec, batch_size=32, to_device=False):
        """The spec model's predict: spec (n, F, frames) or (n, F, frames, 1) float32, the front-end's output, -> (n, D); the
        front-end does not run.  to_device: a usc.DeviceFeatures of the same rows, which the caller owns and closes."""
        if self.embedding_type != 'audio':
            raise TypeError('predict_spectrograms needs an audio embedding model')
        spec = np.ascontiguousarray(spec, dtype=np.float32)
        n = spec.shape[0]
        e = self.base._ensure_engine(self.base._engine.batch if self.base._engine is not None else max(1, min(batch_size, n)))
        if not to_device:
            return e.embed_audio_spec(spec, self.pool)
        from . import usc
        if n == 0:
            raise ValueError('no spectrograms: a device matrix has at least one row')
        D = int(e.lib.l3_embed_dim(e.h, 0, self.pool[0], self.pool[1]))
        out = _lib.Features.alloc(n, D, device=self.base.device)
        e.embed_audio_spec(spec, self.pool, dst=out, row0=0)
        return usc.DeviceFeatures.from_handle(out)

    def predict_images(self, images, batch_size=32, resize=256, crop='center', to_device=False):
        """read_video's resize, the 224 x 224 crop, 2 * img_as_float(u8) - 1 and predict for raw frames of any sizes
        (data/avc/sample.py:286-316, :169-193, train.py:186): images is a sequence of (H, W, 3) uint8 arrays or one
        (T, H, W, 3) uint8 array.  resize, crop: features.image_table's (shorter side 256 and the centre crop by default;
        resize=None takes frames as they are).  Each frame goes to the device once, as bytes, and is resized there
        (csrc/frames.hip: antialiased bilinear).  The engine is chosen as predict chooses it.  Returns
        (n, D) float32, or with to_device=True a usc.DeviceFeatures of the same rows, which the caller owns and closes."""
        from .features import image_table
        if self.embedding_type != 'vision':
            raise TypeError('predict_images needs a vision embedding model')
        whole = None          # a C-contiguous (T, H, W, 3) array is the packed buffer already
        if isinstance(images, np.ndarray) and images.ndim == 4:
            frames = [images[i] for i in range(images.shape[0])]
            if images.dtype == np.uint8 and images.flags['C_CONTIGUOUS']:
                whole = images.reshape(-1)
        elif isinstance(images, np.ndarray):
            raise ValueError('images must be a sequence of (H, W, 3) arrays or one (T, H, W, 3) array (got shape %s)' % (images.shape,))
        else:
            frames = [np.asarray(f) for f in images]
        for f in frames:
            if f.dtype != np.uint8:
                raise ValueError('every image must be uint8 (got %s)' % (f.dtype,))
            if f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
                raise ValueError('every image must have shape (H, W, 3) (got %s)' % (f.shape,))
        table, offs = image_table([f.shape[:2] for f in frames], resize=resize, crop=crop)
        n = len(frames)
        if n == 0:
            if to_device:
                raise ValueError('no images: a device matrix has at least one row')
        e = self.base._ensure_engine(self.base._engine.batch if self.base._engine is not None else max(1, min(batch_size, n)))
        B = e.batch
        D = int(e.lib.l3_embed_dim(e.h, 1, self.pool[0], self.pool[1]))
        if to_device:
            from . import usc
            out = _lib.Features.alloc(n, D, device=self.base.device)
            where = lambda lo, hi: dict(dst=out, row0=lo)
        else:
            out = np.empty((n, D), np.float32)
            where = lambda lo, hi: dict(out=out[lo:hi])
        max_frames = max(B, self.IMAGE_CALL_FRAMES // B * B)
        ends = offs + 3 * table[:, 1] * table[:, 2]
        r0 = 0
        while r0 < n:
            r1 = min(n, r0 + B)
            while r1 < n:
                r2 = min(n, r1 + B)
                if r2 - r0 > max_frames or ends[r2 - 1] - offs[r0] > self.IMAGE_CALL_BYTES:
                    break
                r1 = r2
            base = int(offs[r0])
            if whole is not None:
                pixels = whole[base:int(ends[r1 - 1])]
            else:
                pixels = np.empty(int(ends[r1 - 1]) - base, np.uint8)
                for i in range(r0, r1):
                    pixels[offs[i] - base:ends[i] - base] = frames[i].reshape(-1)
            t = table[r0:r1].copy()
            t[:, 0] -= base
            e.embed_vision_frames(pixels, t, self.pool, **where(r0, r1))
            r0 = r1
        if to_device:
            return usc.DeviceFeatures.from_handle(out)
        return out

    def embedding_dim(self):
        """D of an audio embedding model from the model type and the pooling alone: no engine is made (l3_embed_dim's value)"""
        if self.embedding_type != 'audio' or self.base.model_type not in AUDIO_EMBEDDING_MAP:
            raise TypeError('embedding_dim needs an audio embedding model')
        h, w, c = AUDIO_EMBEDDING_MAP[self.base.model_type]
        return -(-h // self.pool[0]) * -(-w // self.pool[1]) * c

    @property
    def output_shape(self):
        e = self.base._ensure_engine(self.base._engine.batch if self.base._engine is not None else 1)
        return (None, int(e.lib.l3_embed_dim(e.h, 1 if self.embedding_type == 'vision' else 0, self.pool[0], self.pool[1])))


def _clip_span(clips, offs, base, top):
    """Samples [base, top) of the clips laid back to back (offs: each clip's first sample): a view when the span lies in one
    clip, else a concatenation of the pieces."""
    i = int(np.searchsorted(offs, base, side='right')) - 1 if len(offs) else 0
    pieces = []
    while base < top:
        while offs[i] + clips[i].size <= base:
            i += 1
        lo = base - int(offs[i])
        hi = min(clips[i].size, top - int(offs[i]))
        pieces.append(clips[i][lo:hi])
        base += hi - lo
    if len(pieces) == 1:
        return pieces[0]
    return np.concatenate(pieces) if pieces else np.zeros(0, np.float32)


def _resample_rows(clips, rates, offs, lengths, base, top):
    """The native samples and clip rows {x_off, L, sr_orig, t0, n_out, y_off} (l3_embed_audio_clips_resampled) that fill samples
    [base, top) of the 48 kHz clips laid back to back (offs, lengths: their first sample and length at 48 kHz).  Every clip the
    span reaches is uploaded whole: the filter reads up to 64 zero crossings beyond the outputs, and a clip is uploaded once per
    call anyway unless it spans calls."""
    i = int(np.searchsorted(offs + lengths, base, side='right'))
    rows, pieces, pos = [], [], 0
    while i < len(clips) and offs[i] < top:
        lo, hi = max(base, int(offs[i])) - int(offs[i]), min(top, int(offs[i] + lengths[i])) - int(offs[i])
        if hi > lo:
            rows.append((pos, clips[i].size, rates[i], lo, hi - lo, int(offs[i]) + lo - base))
            pieces.append(clips[i])
            pos += clips[i].size
        i += 1
    x = np.concatenate(pieces) if len(pieces) > 1 else (pieces[0] if pieces else np.zeros(0, np.float32))
    return x, np.array(rows, np.int64).reshape(-1, 6)


# ---------------------------------------------------------------------------------------------------
# reference entry points
# ---------------------------------------------------------------------------------------------------
def multi_gpu_model(model, gpus, validate=True, serial=False):
    from .training_utils import multi_gpu_model as _m
    return _m(model, gpus, validate, serial)


def gpu_wrapper(model_f):
    """model.py:184-195"""
    def wrapped(num_gpus=0, *args, **kwargs):
        m, inp, out = model_f(*args, **kwargs)
        if num_gpus > 1:
            m = multi_gpu_model(m, gpus=num_gpus)
        return m, inp, out
    wrapped.__name__ = model_f.__name__
    return wrapped


def _construct(model_type):
    m = L3Model(model_type)
    return m, m.inputs, m.outputs[0]


@gpu_wrapper
def construct_cnn_L3_orig():
    """model.py:198-218"""
    return _construct('cnn_L3_orig')


@gpu_wrapper
def construct_cnn_L3_kapredbinputbn():
    """model.py:220-240"""
    return _construct('cnn_L3_kapredbinputbn')


@gpu_wrapper
def construct_cnn_L3_melspec1():
    """model.py:242-262"""
    return _construct('cnn_L3_melspec1')


@gpu_wrapper
def construct_cnn_L3_melspec2():
    """model.py:264-284"""
    return _construct('cnn_L3_melspec2')


@gpu_wrapper
def construct_tiny_L3():
    """model.py:286-304"""
    return _construct('tiny_L3')


MODELS = {
    'cnn_L3_orig': construct_cnn_L3_orig,
    'tiny_L3': construct_tiny_L3,
    'cnn_L3_kapredbinputbn': construct_cnn_L3_kapredbinputbn,
    'cnn_L3_melspec1': construct_cnn_L3_melspec1,
    'cnn_L3_melspec2': construct_cnn_L3_melspec2,
}


# ---------------------------------------------------------------------------------------------------
# tower-level constructors (re-exported by the reference's model.py:1-4 from vision_model.py / audio_model.py)
# ---------------------------------------------------------------------------------------------------
# (vision tower, audio tower) of every registry entry -- model.py:198-304
TOWERS = {
    'cnn_L3_orig': ('cnn_L3_orig_vision', 'cnn_L3_orig_audio'),
    'cnn_L3_kapredbinputbn': ('cnn_L3_orig_inputbn_vision', 'cnn_L3_kapredbinputbn_audio'),
    'cnn_L3_melspec1': ('cnn_L3_orig_inputbn_vision', 'cnn_L3_melspec1_audio'),
    'cnn_L3_melspec2': ('cnn_L3_orig_inputbn_vision', 'cnn_L3_melspec2_audio'),
    'tiny_L3': ('tiny_L3_vision', 'tiny_L3_audio'),
}


class TowerModel(SubModel):
    """A sub-network on its own, as `construct_cnn_L3_melspec2_audio_model()` and its siblings return it
    (audio_model.py:440-442 `Model(inputs=x_a, outputs=y_a)` named 'audio_model'; vision_model.py:193-195).  The engine
    always holds a whole AVC model, so a free-standing tower is the sub-model of a carrier registry entry that contains it;
    `L3_merge_audio_vision_models` puts two towers (and the weights set on them) back into one model."""

    def __init__(self, kind, carrier_type, prefix):
        SubModel.__init__(self, L3Model(carrier_type), prefix)
        self.kind = kind
        full = self._parent.inputs
        self.inputs = [full[0] if prefix == 'vision_model' else full[1]]
        emb = 512 if carrier_type != 'tiny_L3' else (360 if prefix == 'vision_model' else 350)
        self.output_shape = (None, emb)
        self.outputs = [Layer('flatten', self, tap=(prefix, 'output'))]

    def predict(self, x, batch_size=32, verbose=0):
        """(N, 224, 224, 3) frames or (N, 1, 48000) waveforms -> the tower's flattened output (N, 512), inference-mode
        BatchNorm: the tower's half of the concatenate input (model.py:25), read back from the engine."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = len(x)
        par = self._parent
        e = par._ensure_engine(max(1, min(batch_size, n)) if par._engine is None else par._engine.batch)
        B = e.batch
        vis = self.name == 'vision_model'
        nv = 512 if par.model_type != 'tiny_L3' else 360
        out = np.empty((n,) + self.output_shape[1:], np.float32)
        for s0 in range(0, n, B):
            cnt = min(B, n - s0)
            vb = np.zeros((B, 224, 224, 3), np.float32)
            ab = np.zeros((B, 1, 48000), np.float32)
            (vb if vis else ab)[:cnt] = x[s0:s0 + cnt]
            e.forward(vb, ab, training=False)
            h0 = e.activation('h0').reshape(B, -1)
            out[s0:s0 + cnt] = h0[:cnt, :nv] if vis else h0[:cnt, nv:]
        return out


def _tower(kind):
    carrier = [mt for mt in MODEL_TYPES if kind in TOWERS[mt]][-1]
    prefix = 'vision_model' if kind.endswith('_vision') else 'audio_model'
    m = TowerModel(kind, carrier, prefix)
    return m, m.inputs[0], m.outputs[0]


def construct_cnn_L3_orig_vision_model():
    """vision_model.py:7-99"""
    return _tower('cnn_L3_orig_vision')


def construct_cnn_L3_orig_inputbn_vision_model():
    """vision_model.py:102-195"""
    return _tower('cnn_L3_orig_inputbn_vision')


def construct_tiny_L3_vision_model():
    """vision_model.py:221-290"""
    return _tower('tiny_L3_vision')


def construct_cnn_L3_orig_audio_model():
    """audio_model.py:8-115"""
    return _tower('cnn_L3_orig_audio')


def construct_cnn_L3_kapredbinputbn_audio_model():
    """audio_model.py:118-222"""
    return _tower('cnn_L3_kapredbinputbn_audio')


def construct_cnn_L3_melspec1_audio_model():
    """audio_model.py:225-332"""
    return _tower('cnn_L3_melspec1_audio')


def construct_cnn_L3_melspec2_audio_model():
    """audio_model.py:335-442"""
    return _tower('cnn_L3_melspec2_audio')


def construct_tiny_L3_audio_model():
    """audio_model.py:490-560"""
    return _tower('tiny_L3_audio')


def L3_merge_audio_vision_models(vision_model, x_i, audio_model, x_a, model_name, layer_size=128):
    """model.py:7-35: concatenate + Dense(layer_size, relu) + Dense(2, softmax) over two towers.  The pair must be one the
    engine's ledger knows (the five registry entries of model.py:307-313, TOWERS above); weights assigned to the towers
    (`set_weights`) move into the merged model, the head keeps its he_normal initialisation."""
    pair = (getattr(vision_model, 'kind', None), getattr(audio_model, 'kind', None))
    match = [mt for mt in MODEL_TYPES if TOWERS[mt] == pair]
    if not match:
        raise ValueError('no L3 model is made of the towers {}'.format(pair))
    if layer_size != (64 if match[0] == 'tiny_L3' else 128):
        raise ValueError('layer_size={} is not the head of "{}"'.format(layer_size, match[0]))
    m = L3Model(match[0])
    m.name = model_name
    for tower in (vision_model, audio_model):
        src = tower._parent
        if src._engine is not None or src._host_weights is not None:
            W = src._weights_dict()
            m._assign(OrderedDict((n, W[n]) for n in tower._names()))
    return m, m.inputs, m.outputs[0]


def convert_num_gpus(model, inputs, outputs, model_type, src_num_gpus, tgt_num_gpus):
    """model.py:38-82"""
    if src_num_gpus <= 1 and tgt_num_gpus <= 1:
        return model, inputs, outputs
    m_new, inputs_new, output_new = MODELS[model_type]()
    m_new.set_weights(model.layers[-2].get_weights())
    if tgt_num_gpus > 1:
        m_new = multi_gpu_model(m_new, gpus=tgt_num_gpus)
    return m_new, inputs_new, output_new


def load_model(weights_path, model_type, src_num_gpus=0, tgt_num_gpus=None, return_io=False):
    """model.py:85-128"""
    if model_type not in MODELS:
        raise ValueError('Invalid model type: "{}"'.format(model_type))
    m, inputs, output = MODELS[model_type]()
    if src_num_gpus > 1:
        # only the wrapper's weight-file layout is needed here: no device check (a file written by an
        # 8-GPU run loads on any box; the reference needs src_num_gpus real GPUs even to read it)
        m = multi_gpu_model(m, gpus=src_num_gpus, validate=False)
    m.load_weights(weights_path)
    if tgt_num_gpus is not None and src_num_gpus != tgt_num_gpus:
        m, inputs, output = convert_num_gpus(m, inputs, output, model_type, src_num_gpus, tgt_num_gpus)
    if return_io:
        return m, inputs, output
    return m


def convert_audio_model_to_embedding(audio_model, x_a, model_type, pooling_type='original'):
    """audio_model.py:445-487"""
    pool_size = AUDIO_POOLING[model_type][pooling_type]
    audio_model.get_layer('audio_embedding_layer')
    m = EmbeddingModel(audio_model._parent, 'audio', pool_size)
    return m, x_a, Layer('flatten', m)


def construct_cnn_l3_orig_vision_embedding_model(vision_model, x_i):
    """vision_model.py:198-218"""
    vision_model.get_layer('vision_embedding_layer')
    m = EmbeddingModel(vision_model._parent, 'vision', VISION_POOLING)
    return m, x_i, Layer('flatten', m)


def load_embedding(weights_path, model_type, embedding_type, pooling_type, src_num_gpus=0, tgt_num_gpus=None,
                   return_io=False, frontend='kapre'):
    """model.py:131-181.  frontend: 'kapre', or 'minispec' for the deployed pipeline's spectrogram."""
    m, inputs, output = load_model(weights_path, model_type, src_num_gpus=src_num_gpus,
                                   tgt_num_gpus=tgt_num_gpus, return_io=True)
    x_i, x_a = inputs
    if embedding_type == 'vision':
        m_embed_model = m.get_layer('vision_model')
        m_embed, x_embed, y_embed = construct_cnn_l3_orig_vision_embedding_model(m_embed_model, x_i)
    elif embedding_type == 'audio':
        m_embed_model = m.get_layer('audio_model')
        m_embed, x_embed, y_embed = convert_audio_model_to_embedding(m_embed_model, x_a, model_type, pooling_type)
    else:
        raise ValueError('Invalid embedding type: "{}"'.format(embedding_type))
    m_embed.base.set_frontend(frontend)
    if return_io:
        return m_embed, x_embed, y_embed
    return m_embed
