"""Training-set augmentation of `02_generate_samples.py --augment` (data/avc/sample.py:24-69, 117-166, 169-283) on the GPU.

The reference augments offline and bakes ONE draw into the blobs it writes.  Here the draws are made per batch on the host, in
the reference's order of `random` calls, and applied by the kernels of csrc/augment.hip -- as a stand-alone operator
(`augment_batch`), inside the pass that scales a stored batch for the engine (`AugmentingFeed` + `L3Model`), or to write
augmented blobs like the reference's (`rewrite`).  One un-augmented blob set then yields a fresh draw every epoch.

What is NOT here is the file walking of data/avc/sample.py (video decoding needs ffmpeg): the inputs are frames and seconds
that have already been chosen.

    python -m l3embedding_amd.augment rewrite SRC_DIR DST_DIR [--random-state N]
"""
import os
import random

import numpy as np

from . import h5lite

CROP = 224
# one row per sample: the gain's uniform draw and the record of include/l3hip.h l3_augment_params
PARAMS = np.dtype([('u_gain', np.float64), ('start_x', np.int32), ('start_y', np.int32), ('flip', np.int32),
                   ('sat_first', np.int32), ('saturation', np.float32), ('brightness', np.float32)])
# flatten_dict's names for the augmentation parameters of generate_sample(include_metadata=True) (sample.py:384-385)
METADATA_KEYS = ('audio_gain', 'video_bounding_box_start_x', 'video_bounding_box_start_y', 'video_horizontal_flip',
                 'video_saturation_factor', 'video_brightness_delta')


def draw_params(rng, n, frame_shape=(CROP, CROP)):
    """n samples' draws from `rng` (a random.Random), per sample in the reference's call order:
    the gain's random() (random.uniform, sample.py:156), start_x = randrange(H - 224), start_y = randrange(W - 224)
    (sample.py:182; skipped where the extent is already 224, where the reference's randrange(0) would raise),
    flip = random() < 0.5 (sample.py:244), saturation-first = random() < 0.5 (sample.py:252), then the two factors in the
    chosen order (sample.py:254,260 / 266,271), each rounded to float32 as the reference rounds it."""
    h, w = int(frame_shape[0]), int(frame_shape[1])
    if h < CROP or w < CROP:
        raise ValueError('frames of %d x %d are smaller than the %d x %d crop' % (h, w, CROP, CROP))
    p = np.zeros(int(n), PARAMS)
    max_delta = 32. / 255.
    for i in range(int(n)):
        p['u_gain'][i] = rng.random()
        if h > CROP:
            p['start_x'][i] = rng.randrange(h - CROP)
        if w > CROP:
            p['start_y'][i] = rng.randrange(w - CROP)
        p['flip'][i] = rng.random() < 0.5
        sat_first = rng.random() < 0.5
        p['sat_first'][i] = sat_first
        if sat_first:
            p['saturation'][i] = np.float32(rng.random() + 0.5)
            p['brightness'][i] = np.float32((2 * rng.random() - 1) * max_delta)
        else:
            p['brightness'][i] = np.float32((2 * rng.random() - 1) * max_delta)
            p['saturation'][i] = np.float32(rng.random() + 0.5)
    return p


def identity_params(n):
    """Records that change nothing in the frames: no crop offset, no flip, factor 1, delta 0.  (The audio gain has no identity
    draw: u_gain = 0 is the lower end of its range, 0.9.)"""
    p = np.zeros(int(n), PARAMS)
    p['sat_first'] = 1
    p['saturation'] = 1.0
    return p


def metadata(params, gains):
    """The reference's per-sample augmentation metadata under generate_sample's keys (sample.py:162,185-188,275-279,384-385).
    horizontal_flip is stored as 0 / 1 (h5lite has no HDF5 enum, which is how h5py writes a bool)."""
    return {'audio_gain': np.asarray(gains, np.float64),
            'video_bounding_box_start_x': params['start_x'].astype(np.int64),
            'video_bounding_box_start_y': params['start_y'].astype(np.int64),
            'video_horizontal_flip': (params['flip'] != 0).astype(np.uint8),
            'video_saturation_factor': params['saturation'].astype(np.float32),
            'video_brightness_delta': params['brightness'].astype(np.float32)}


def augment_batch(video_u8, audio_i16, params, device=0):
    """Frames (N, H, W, 3) uint8 and seconds (N, T) or (N, 1, T) int16 -> {'video': (N, 224, 224, 3) uint8, 'audio': int16 in the
    input's shape} plus the keys of `metadata` -- what generate_sample(augment=True, include_metadata=True) leaves of them."""
    from . import _lib
    v, a = np.asarray(video_u8), np.asarray(audio_i16)
    if v.dtype != np.uint8 or a.dtype != np.int16:
        raise ValueError('augmentation takes the stored dtypes (uint8 frames, int16 PCM), got %s and %s' % (v.dtype, a.dtype))
    params = np.asarray(params)
    if len(params) != len(v) or len(a) != len(v):
        raise ValueError('%d frames, %d seconds, %d parameter rows' % (len(v), len(a), len(params)))
    out = {'video': _lib.op_augment_video(v, params, out='u8', device=device)}
    rows, gains = _lib.op_augment_audio(a.reshape(len(a), -1), params['u_gain'], out='i16', device=device)
    out['audio'] = rows.reshape(a.shape)
    out.update(metadata(params, gains))
    return out


class AugmentedInputs(list):
    """`[video, audio]` of a raw batch with `.augment`, the parameter rows of the GLOBAL batch (L3Model slices them with the rows'
    own bounds).  `global_batch` is kept from blobfeed.ShardedInputs where the feed had already split the batch."""

    def __init__(self, arrays, augment, global_batch=None):
        super().__init__(arrays)
        self.augment = augment
        if global_batch:
            self.global_batch = int(global_batch)


class AugmentingFeed(object):
    """Wraps a generator of raw `([video, audio], labels, ...)` batches: the arrays and labels pass through untouched, the inputs
    gain `.augment` -- a fresh draw for every batch from a private random.Random(random_state), so a run is reproducible and
    every rank of a data-parallel job draws the same rows for the same global batch."""

    def __init__(self, generator, random_state=20180123):
        self._gen = iter(generator)
        self.rng = random.Random(random_state)

    def __iter__(self):
        return self

    def __next__(self):
        item = next(self._gen)
        x = item[0]
        v = x[0]
        n = getattr(x, 'global_batch', None) or len(v)
        params = draw_params(self.rng, n, np.shape(v)[1:3])
        return (AugmentedInputs(x, params, getattr(x, 'global_batch', None)),) + tuple(item[1:])

    def close(self):
        closer = getattr(self._gen, 'close', None)
        if closer is not None:
            closer()


def rewrite(src_dir, dst_dir, random_state=20180123, device=0):
    """Every un-augmented blob of `src_dir` written to `dst_dir` as 02_generate_samples.py --augment would have left it: 'video'
    and 'audio' augmented with one draw per row, the metadata datasets of `metadata` added, everything else copied (the pattern
    of blobfeed.rewrite_uncompressed).  Blobs are taken in sorted order so that the draws do not depend on the directory
    listing."""
    os.makedirs(dst_dir, exist_ok=True)
    rng = random.Random(random_state)
    done = []
    for name in sorted(os.listdir(src_dir)):
        path = os.path.join(src_dir, name)
        if not os.path.isfile(path):
            continue
        with h5lite.File(path) as f:
            data = {k: node.read() for k, node in f.root.children.items() if isinstance(node, h5lite.Dataset)}
            attrs = dict(f.root.attrs.items())
        if 'video' not in data or 'audio' not in data:
            raise ValueError('%s has no video / audio datasets' % path)
        params = draw_params(rng, len(data['video']), data['video'].shape[1:3])
        data.update(augment_batch(data['video'], data['audio'], params, device=device))
        root = h5lite.Group()
        for k, arr in data.items():
            root.create_dataset(k, arr)
        for k, v in attrs.items():
            root.attrs[k] = v
        tmp = os.path.join(dst_dir, name + '.partial.%d' % os.getpid())
        h5lite.write_file(tmp, root)
        os.replace(tmp, os.path.join(dst_dir, name))
        done.append(name)
    return done


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog='python -m l3embedding_amd.augment', description=__doc__.split('\n')[0])
    sub = p.add_subparsers(dest='command', required=True)
    rw = sub.add_parser('rewrite', help='write every blob of SRC_DIR to DST_DIR augmented, with the metadata datasets')
    rw.add_argument('src_dir')
    rw.add_argument('dst_dir')
    rw.add_argument('--random-state', dest='random_state', type=int, default=20180123)
    rw.add_argument('--device', type=int, default=0)
    args = p.parse_args(argv)
    print('%d blobs rewritten' % len(rewrite(args.src_dir, args.dst_dir, args.random_state, args.device)))


if __name__ == '__main__':
    main()
