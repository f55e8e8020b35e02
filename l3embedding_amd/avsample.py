"""AVC training samples of `02_generate_samples.py` (data/avc/sample.py: `sampler`, `generate_sample`, `sample_one_second`,
`sample_one_frame`, `sample_cropped_frame`) cut on the GPU from decoded clips that are held there.

The reference pairs two videos, picks a second of audio from one of them, a frame inside that second from one of them, crops the
frame and optionally augments both.  Here the clips are uploaded once into a `ClipBank`; the draws are made on the host in the
reference's order of `random` calls (`draw_samples`) and travel as a few dozen bytes per sample (`SAMPLE`); the engine builds the
batch from them with the resize of csrc/frames.hip, the kernels of csrc/avsample.hip and the augmentation of csrc/augment.hip
(`ClipSampler` + `L3Model`, `train.train_sampled`).  The same code writes blobs in the reference's format (`write_blobs`).

What is NOT here, and not reproduced:
  * decoding and file walking (ffmpeg, soundfile): the inputs are decoded clips;
  * ffmpeg's scaler: a bank with `resize=256` resizes with csrc/frames.hip's antialiased bilinear rule;
  * pescador's `Mux`: pescador is not installed here, and the order in which its streamers are opened, sampled and replaced is
    not reproduced.  `ClipSampler` states its own multiplexing rule in full instead.

    python -m l3embedding_amd.avsample generate CLIP.npz CLIP.npz [...] --out-dir DIR --num-batches N

reads each clip from an .npz file holding `frames` (T, H, W, 3) uint8, `audio` (n,) or (n, C) int16 and `rate` -- this project's
own container for a decoded clip, not a format of the reference.
"""
import collections
import os
import random

import numpy as np

from . import _lib, augment, features, h5lite

T = 48000            # one second at the sampler's rate (sample.py:129-136)
FPS = 30             # generate_sample never passes fps to sample_one_frame (sample.py:196,368-369)
CROP = augment.CROP

# One row per sample: where it comes from, its label and the fields of augment.PARAMS.  The layout is l3_sample's (include/l3hip.h).
SAMPLE = _lib.SAMPLE_RECORD
assert all(name in SAMPLE.names for name in augment.PARAMS.names)

# What the draws need to know of a clip: frames as the sampler sees them are out_height x out_width
ClipInfo = collections.namedtuple('ClipInfo', 'frames height width out_height out_width samples name')


def clip_info(n_frames, height, width, n_samples, resize=256, name=None):
    """The ClipInfo of a clip of n_frames frames of height x width and n_samples mono samples in a bank with `resize`:
    features.image_table's sizes (read_video's rule, sample.py:303-305), or the frame's own for resize=None."""
    if resize is None and (height <= CROP or width <= CROP):
        raise ValueError('frames of %d x %d without a resize: both sides must be >= %d (the reference draws randrange(side - %d), '
                         'which raises at 0)' % (height, width, CROP + 1, CROP))
    row = features.image_table([(height, width)], resize=resize)[0][0]
    return ClipInfo(int(n_frames), int(height), int(width), int(row[3]), int(row[4]), int(n_samples), name)


def draw_samples(rng, clip_a, clip_b, n, augment, clips):
    """n samples of the pair (clip_a, clip_b) from `rng` (a random.Random), per sample in the reference's order of calls:
    video_choice = random() < 0.5, audio_choice = random() < 0.5 (sample.py:346-347; True takes clip_a); start =
    randrange(len - 48000) only when len > 48000, else 0 (sample.py:130-133); if augmenting the gain's random() (sample.py:156);
    start_frame = int((start / 48000.0) * 30), duration = min(30, num_frames - start_frame), frame = start_frame +
    randrange(duration) when duration > 0, else min(start_frame, num_frames - 1) without a draw (sample.py:212-230); start_x =
    randrange(Ho - 224), start_y = randrange(Wo - 224) (sample.py:181-182); if augmenting flip, order and the two factors as
    augment.draw_params draws them (sample.py:244-273).  label = int(video_choice != audio_choice) (sample.py:363): the labels row
    is [label, 1 - label] (sample.py:376).  `clips`: ClipInfo by clip id.  Un-augmented rows carry augment.identity_params' values."""
    out = np.zeros(int(n), SAMPLE)
    max_delta = 32. / 255.
    for i in range(int(n)):
        video_choice = rng.random() < 0.5
        audio_choice = rng.random() < 0.5
        vid, aud = (clip_a if video_choice else clip_b), (clip_a if audio_choice else clip_b)
        v, a = clips[vid], clips[aud]
        start = rng.randrange(a.samples - T) if a.samples > T else 0
        if augment:
            out['u_gain'][i] = rng.random()
        start_frame = int((start / float(T)) * FPS)
        duration = min(FPS, v.frames - start_frame)
        if duration > 0:
            frame = start_frame + rng.randrange(duration)
        else:
            frame = min(start_frame, v.frames - 1)
        out['video_clip'][i], out['frame'][i] = vid, frame
        out['audio_clip'][i], out['audio_start'][i] = aud, start
        out['label'][i] = int(video_choice != audio_choice)
        out['start_x'][i] = rng.randrange(v.out_height - CROP)
        out['start_y'][i] = rng.randrange(v.out_width - CROP)
        if not augment:
            out['sat_first'][i], out['saturation'][i] = 1, 1.0
            continue
        out['flip'][i] = rng.random() < 0.5
        sat_first = rng.random() < 0.5
        out['sat_first'][i] = sat_first
        if sat_first:
            out['saturation'][i] = np.float32(rng.random() + 0.5)
            out['brightness'][i] = np.float32((2 * rng.random() - 1) * max_delta)
        else:
            out['brightness'][i] = np.float32((2 * rng.random() - 1) * max_delta)
            out['saturation'][i] = np.float32(rng.random() + 0.5)
    return out


def labels_of(records):
    """(n, 2) int64 rows [label, 1 - label] (sample.py:376)."""
    d = np.asarray(records['label'], np.int64)
    return np.stack([d, 1 - d], axis=1)


class ClipBank(object):
    """Decoded clips resident on the GPU (l3_clipbank): `pixel_bytes` of frames kept as uploaded and `audio_samples` of mono int16
    samples, allocated once; a 10 s clip of 360 x 640 at 30 fps takes 207 MB.  resize=256: frames are resized as
    features.image_table sizes them (read_video's rule) when a sample's window is cut; resize=None: the frames are as the
    caller's decoder resized them."""

    def __init__(self, device=0, pixel_bytes=None, audio_samples=None, resize=256):
        if pixel_bytes is None or audio_samples is None:
            raise ValueError('a ClipBank is allocated once: give pixel_bytes and audio_samples')
        if resize is not None and int(resize) <= CROP:
            raise ValueError('resize must be > %d or None (got %r)' % (CROP, resize))
        self.resize = None if resize is None else int(resize)
        self.device = int(device)
        self.clips = []
        self._handle = _lib.ClipBank(device, pixel_bytes, audio_samples, self.resize or 0)

    @property
    def h(self):
        return self._handle.h

    def add(self, frames, audio, rate, name=None):
        """One clip: (T, H, W, 3) uint8 frames and (n,) or (n, C) int16 PCM at 48 kHz.  Several channels are mixed as
        sample.py:445-448 mixes them, on the GPU.  Returns the clip's id."""
        if int(rate) != T:
            raise ValueError('audio at %r Hz: the sampler cuts seconds of %d samples (the reference would produce rows of the wrong '
                             'length); resample the clip first, e.g. with l3embedding_amd.resample.resample' % (rate, T))
        frames, audio = np.asarray(frames), np.asarray(audio)
        if frames.dtype != np.uint8 or audio.dtype != np.int16:
            raise ValueError('a clip is uint8 frames and int16 PCM, got %s and %s' % (frames.dtype, audio.dtype))
        if frames.ndim != 4 or frames.shape[3] != 3 or audio.ndim not in (1, 2) or len(frames) < 1 or len(audio) < 1:
            raise ValueError('a clip is (T, H, W, 3) frames and (n,) or (n, C) samples, got %r and %r' % (frames.shape, audio.shape))
        info = clip_info(frames.shape[0], frames.shape[1], frames.shape[2], audio.shape[0], self.resize)      # refuses small frames
        cid = self._handle.add(frames, audio.reshape(len(audio), -1))
        got = self._handle.info(cid)
        if got != tuple(info[:6]):
            raise RuntimeError('clip %d: the library sees %r, the host rule %r' % (cid, got, tuple(info[:6])))
        self.clips.append(info._replace(name=name if name is not None else 'clip_%d' % cid))
        return cid

    def audio(self, clip):
        """The clip's mono samples as the bank holds them."""
        return self._handle.audio(clip)

    def usage(self):
        """(pixel bytes used, capacity, samples used, capacity)."""
        return self._handle.info(-1)[1:5]

    def close(self):
        self._handle.close()


class SampledInputs(object):
    """The inputs of a training batch that the engine cuts itself: the bank and the SAMPLE rows in place of arrays."""

    def __init__(self, bank, records, augmented=False):
        self.bank = bank
        self.sample_records = records
        self.augmented = bool(augmented)

    def __len__(self):
        return len(self.sample_records)


def form_pairs(rng, n_clips, num_distractors=1):
    """The (clip, other clip) pairs of data_generator (sample.py:538-553) from `rng`: per clip and distractor, choice() over all
    clips repeated until it names another clip; then the pairs are shuffled."""
    if n_clips < 2:
        raise ValueError('pairs need at least two clips, the bank holds %d' % n_clips)
    ids = list(range(n_clips))
    pairs = []
    for a in ids:
        for _ in range(num_distractors):
            b = a
            while b == a:
                b = rng.choice(ids)
            pairs.append((a, b))
    rng.shuffle(pairs)
    return pairs


class ClipSampler(object):
    """Iterator of `(SampledInputs, labels)` batches over the clips of `bank`.

    Pairs are formed as data_generator forms them (`form_pairs`) from one private random.Random(random_state), which then also
    makes every sample's draws (`draw_samples`), as the reference's module-level generator does.

    The multiplexer is this project's own rule -- pescador is not installed here and its Mux is NOT reproduced.  With
    np.random.RandomState(random_state): the first min(k, len(pairs)) pairs of the list are active, each with a budget of
    max(1, poisson(rate)) samples.  Every sample picks an active slot with randint(len(active)), draws one sample of that slot's
    pair and spends one unit of its budget; a spent slot takes the next pair of the list with a fresh budget.  cycle=True wraps
    around the list; cycle=False drops the slot instead, and the stream ends when no slot is left (a last, partial batch is
    dropped).  `bank` needs only `.clips` (ClipInfo rows) to draw; the batches it yields need a real ClipBank to be built."""

    def __init__(self, bank, batch_size=64, random_state=20171021, k=32, rate=32, num_distractors=1, augment=False, cycle=True):
        self.bank = bank
        self.batch_size, self.k, self.rate, self.augment, self.cycle = int(batch_size), int(k), rate, bool(augment), bool(cycle)
        self.rng = random.Random(random_state)
        self.pairs = form_pairs(self.rng, len(bank.clips), int(num_distractors))
        self.mux = np.random.RandomState(random_state)
        self.args = dict(batch_size=self.batch_size, random_state=random_state, k=self.k, rate=rate,
                         num_distractors=int(num_distractors), augment=self.augment, cycle=self.cycle)
        self.trace = None           # set to a list: one (pair, budget left after the draw, active pairs before it) per sample
        self._next_pair = 0
        self.active = []
        for _ in range(min(self.k, len(self.pairs))):
            self.active.append(self._open())

    def _open(self):
        if self._next_pair >= len(self.pairs):
            if not self.cycle:
                return None
            self._next_pair = 0
        slot = [self.pairs[self._next_pair], max(1, int(self.mux.poisson(self.rate)))]
        self._next_pair += 1
        return slot

    def _one(self):
        if not self.active:
            raise StopIteration
        i = int(self.mux.randint(len(self.active)))
        slot = self.active[i]
        before = [s[0] for s in self.active] if self.trace is not None else None
        rec = draw_samples(self.rng, slot[0][0], slot[0][1], 1, self.augment, self.bank.clips)[0]
        slot[1] -= 1
        if self.trace is not None:
            self.trace.append((slot[0], slot[1], before))
        if slot[1] == 0:
            fresh = self._open()
            if fresh is None:
                del self.active[i]
            else:
                self.active[i] = fresh
        return rec

    def __iter__(self):
        return self

    def __next__(self):
        records = np.zeros(self.batch_size, SAMPLE)
        for i in range(self.batch_size):
            records[i] = self._one()
        return SampledInputs(self.bank, records, self.augment), labels_of(records)


def sample_batch(bank, records, augment_rows=False):
    """The batch of `records` in the stored dtypes under generate_sample(include_metadata=True)'s keys (sample.py:373-385):
    video (n, 224, 224, 3) uint8, audio (n, 1, 48000) int16, label (n, 2), audio_file, video_file, audio_start_sample_idx --
    which despite its name is start / 48000.0 (sample.py:166,382) --, video_start_frame_idx and, when augmenting, the keys of
    augment.metadata with the crop offsets of the records."""
    records = np.asarray(records)
    v, a, gains = _lib.op_sample_batch(bank, records, augment_rows)
    names = [str(c.name).encode('utf-8') for c in bank.clips]
    out = {'video': v, 'audio': a.reshape(len(a), 1, T), 'label': labels_of(records),
           'audio_file': np.array([names[i] for i in records['audio_clip']]),
           'video_file': np.array([names[i] for i in records['video_clip']]),
           'audio_start_sample_idx': records['audio_start'].astype(np.float64) / float(T),
           'video_start_frame_idx': records['frame'].astype(np.int64)}
    if augment_rows:
        out.update(augment.metadata(records, gains))
    return out


def write_blobs(sampler, num_batches, out_dir):
    """`num_batches` batches of `sampler` as the blobs sample_and_save writes (sample.py:565-595): one gzip-compressed dataset per
    key, named {random_state}_0_{i}.h5.  train.data_generator reads them.  Returns the paths."""
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for i in range(int(num_batches)):
        x, _ = next(sampler)
        batch = sample_batch(x.bank, x.sample_records, x.augmented)
        root = h5lite.Group()
        for key, arr in batch.items():
            root.create_dataset(key, arr, compression='gzip')
        path = os.path.join(out_dir, '%s_0_%d.h5' % (sampler.args['random_state'], i))
        tmp = path + '.partial.%d' % os.getpid()
        h5lite.write_file(tmp, root)
        os.replace(tmp, path)
        paths.append(path)
    return paths


def load_clips(bank, paths):
    """Adds the clip of every .npz of `paths` (frames, audio, rate) to `bank`, named after its file."""
    for path in paths:
        with np.load(path) as z:
            bank.add(z['frames'], z['audio'], int(z['rate']), name=os.path.basename(path))
    return bank


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog='python -m l3embedding_amd.avsample', description=__doc__.split('\n')[0])
    sub = p.add_subparsers(dest='command', required=True)
    g = sub.add_parser('generate', help='write blobs sampled from decoded clips (.npz files holding frames, audio and rate)')
    g.add_argument('clips', nargs='+')
    g.add_argument('--out-dir', required=True)
    g.add_argument('--num-batches', type=int, required=True)
    g.add_argument('--batch-size', type=int, default=64)
    g.add_argument('--random-state', type=int, default=20171021)
    g.add_argument('--num-streamers', type=int, default=32)
    g.add_argument('--rate', type=int, default=32)
    g.add_argument('--num-distractors', type=int, default=1)
    g.add_argument('--augment', action='store_true')
    g.add_argument('--resize', type=int, default=256, help='0: the frames are already resized')
    g.add_argument('--device', type=int, default=0)
    args = p.parse_args(argv)
    pixels = samples = 0
    for path in args.clips:
        with np.load(path) as z:
            pixels += z['frames'].size
            samples += len(z['audio']) + 8
    bank = load_clips(ClipBank(args.device, pixels, samples, args.resize or None), args.clips)
    sampler = ClipSampler(bank, args.batch_size, args.random_state, args.num_streamers, args.rate, args.num_distractors,
                          args.augment)
    print('%d blobs written' % len(write_blobs(sampler, args.num_batches, args.out_dir)))
    bank.close()


if __name__ == '__main__':
    main()
