"""ref_avsample.npz: samples computed by the REFERENCE's own generate_sample (data/avc/sample.py:319-387, with
sample_one_second :117-166, sample_one_frame :196-283 and sample_cropped_frame :169-193), imported by path and executed unmodified
through make_ref_fixtures.import_reference (same interpreter, same placeholder modules; see that file's header).

Per sample: random.seed(s), then generate_sample(name_1, audio_1, name_2, audio_2, name_1, frames_1, name_2, frames_2, 48000,
augment, include_metadata=True) on two of the synthetic clips of tests/avsample_ref.py (FIXTURE_CLIPS), regenerated there from
seeds.  Stored: the seed, the pair, the outputs and the metadata -- never the clips.

  plain_*   un-augmented samples with their frames and audio rows: a yardstick in full
  aug_*     augmented samples with audio rows and metadata only: that interpreter's skimage (0.18.3) gives float images the
            limits (-1, 1) in the colour operations, so its augmented frame BYTES are not the reference's of its own era and are
            not stored; draws, gains, audio rows and labels are

The seeds are found by a scan, in order, so that every case of the rule is met: a clip shorter than a second (padding, no
start draw, a frame draw over 7 frames), a clip of exactly one second, a start late enough that duration < 30, and one for
which duration <= 0.

    python tests/golden/make_avsample_fixture.py        (the interpreter make_ref_fixtures.py names)
"""
import os
import random
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import avsample_ref as A                            # noqa: E402
from make_ref_fixtures import import_reference      # noqa: E402

N_PLAIN, N_AUG = 12, 24
META = ('audio_start_sample_idx', 'video_start_frame_idx', 'video_bounding_box_start_x', 'video_bounding_box_start_y')
META_AUG = ('audio_gain', 'video_horizontal_flip', 'video_saturation_factor', 'video_brightness_delta')


def cases_of(sample, pair):
    """which cases of the rule a sample exercises"""
    clip_of = dict(zip([os.path.basename(n).encode() for n in A.FIXTURE_NAMES], range(3)))
    ac, vc = clip_of[sample['audio_file']], clip_of[sample['video_file']]
    n_samples, n_frames = A.FIXTURE_CLIPS[ac][4], A.FIXTURE_CLIPS[vc][1]
    start = int(round(sample['audio_start_sample_idx'] * A.T))
    start_frame = int((start / float(A.T)) * A.FPS)
    duration = min(A.FPS, n_frames - start_frame)
    out = set()
    if n_samples < A.T:
        out.add('padded')
    if n_samples == A.T:
        out.add('exact')
    if n_frames < A.FPS and duration > 0:
        out.add('short_video')
    if 0 < duration < A.FPS and n_frames >= A.FPS:
        out.add('late')
    if duration <= 0:
        out.add('past_end')
    if duration == A.FPS:
        out.add('full')
    out.add('label_%d' % sample['label'][0])
    return out


def collect(ref_sample, clips, augment, count):
    want = {'padded', 'exact', 'short_video', 'late', 'past_end', 'full', 'label_0', 'label_1'}
    kept, seen, fill = [], set(), []
    for seed in range(2000):
        pair = A.FIXTURE_PAIRS[seed % len(A.FIXTURE_PAIRS)]
        (f1, a1), (f2, a2) = clips[pair[0]], clips[pair[1]]
        n1, n2 = A.FIXTURE_NAMES[pair[0]], A.FIXTURE_NAMES[pair[1]]
        random.seed(seed)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            s = ref_sample.generate_sample(n1, a1, n2, a2, n1, f1, n2, f2, A.T, augment, include_metadata=True)
        new = cases_of(s, pair) - seen
        if new:
            seen |= new
            kept.append((seed, pair, s))
        elif len(fill) < count:
            fill.append((seed, pair, s))
        if seen == want and len(kept) + len(fill) >= count:
            break
    assert seen == want, want - seen
    kept = sorted(kept + fill[:max(0, count - len(kept))], key=lambda t: t[0])
    return kept, seen


def pack(prefix, kept, augment, with_video, out):
    out[prefix + '_seed'] = np.array([k[0] for k in kept])
    out[prefix + '_pair'] = np.array([k[1] for k in kept])
    samples = [k[2] for k in kept]
    out[prefix + '_audio'] = np.stack([s['audio'] for s in samples])
    out[prefix + '_label'] = np.stack([s['label'] for s in samples])
    out[prefix + '_audio_file'] = np.array([s['audio_file'] for s in samples])
    out[prefix + '_video_file'] = np.array([s['video_file'] for s in samples])
    for key in META + (META_AUG if augment else ()):
        out[prefix + '_' + key] = np.array([s[key] for s in samples])
    if with_video:
        out[prefix + '_video'] = np.stack([s['video'] for s in samples])


if __name__ == '__main__':
    _, _, _, ref_sample = import_reference()
    clips = A.fixture_clips()
    out = {}
    plain, seen = collect(ref_sample, clips, False, N_PLAIN)
    pack('plain', plain, False, True, out)
    print('plain: %d samples, cases %s' % (len(plain), sorted(seen)))
    aug, seen = collect(ref_sample, clips, True, N_AUG)
    pack('aug', aug, True, False, out)
    print('aug: %d samples, cases %s' % (len(aug), sorted(seen)))
    # the arithmetic of the augmented rows, checked where it is computed: trunc(slice * gain)
    for seed, pair, s in aug:
        names = [os.path.basename(n).encode() for n in A.FIXTURE_NAMES]
        mono = clips[names.index(s['audio_file'])][1]
        start = int(round(s['audio_start_sample_idx'] * A.T))
        row = A.one_second(mono, start).astype(float)
        row *= s['audio_gain']
        assert np.array_equal(row.astype(np.int16), s['audio'][0]), seed
    path = os.path.join(HERE, 'ref_avsample.npz')
    np.savez_compressed(path, **out)
    print('ref_avsample.npz: %d bytes' % os.path.getsize(path))
