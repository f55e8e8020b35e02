"""NumPy oracle of the sampled-batch tests, in the project's own words: what data/avc/sample.py leaves of a pair of decoded
clips once the draws are made -- the mono mix, the second with its zero padding, the frame and its crop.  The resize comes
through tests/image_ref.py and the augmentation through tests/augment_ref.py.  Also the synthetic clips that the fixture
tests/golden/ref_avsample.npz was computed on (regenerated from seeds here and in tests/golden/make_avsample_fixture.py; the
fixture stores only seeds, outputs and metadata).

Shared by tests/test_avsample_host.py and tests/test_avsample_gpu.py; not a test module itself.  NumPy only."""
import functools

import numpy as np

T = 48000
FPS = 30
CROP = 224

# (seed, frames, H, W, samples, amplitude): 40 frames with 1.5 s of audio; 7 frames with less than a second (padding, start = 0
# without a draw, a frame draw over 7 frames); a clip of exactly one second whose samples reach full scale
FIXTURE_CLIPS = [(11, 40, 232, 240, 72000, 30000), (12, 7, 256, 300, 30000, 12000), (13, 30, 230, 226, 48000, 32767)]
FIXTURE_NAMES = ['/data/clips/a.mp4', '/data/clips/b.mp4', '/data/clips/c.mp4']
# the (clip_1, clip_2) orders the fixture's seeds cycle through
FIXTURE_PAIRS = [(0, 1), (1, 0), (0, 2), (2, 1), (1, 2), (2, 0)]


def synth_clip(seed, n_frames, H, W, n_samples, amplitude):
    """(frames (n_frames, H, W, 3) uint8, audio (n_samples,) int16) of low entropy, so that rows cut from them compress, yet
    every second and every crop is unlike any other: a short random pattern repeated, with a counter written over it every
    1000 samples / at every 8th pixel of every 8th row."""
    rs = np.random.RandomState(seed)
    pat = rs.randint(-amplitude, amplitude + 1, 499)
    pat[0] = amplitude
    audio = np.resize(pat, n_samples).astype(np.int16)
    audio[::1000] = np.arange(len(audio[::1000])) * 7 - 200
    tile = rs.randint(0, 256, (61, 3))
    f, y, x = np.meshgrid(np.arange(n_frames), np.arange(H), np.arange(W), indexing='ij')
    frames = tile[(x + 5 * y + 17 * f) % 61].astype(np.uint8)
    mark = np.stack([2 * f + (x >> 8), y & 255, x & 255], -1).astype(np.uint8)
    frames[:, ::8, ::8] = mark[:, ::8, ::8]
    return frames, audio


@functools.lru_cache(maxsize=None)
def fixture_clips():
    """[(frames, audio)] of FIXTURE_CLIPS, computed once per process; callers must not write to them"""
    out = [synth_clip(*spec) for spec in FIXTURE_CLIPS]
    for fr, au in out:
        fr.setflags(write=False)
        au.setflags(write=False)
    return out


def downmix(audio):
    """sample.py:445-448: the mean over the channels in float64, truncated toward zero by astype('int16')"""
    a = np.asarray(audio)
    if a.ndim == 1:
        return a.astype(np.int16)
    return a.mean(axis=-1).astype('int16')


def one_second(mono, start):
    """sample.py:136-144: mono[start : start + T], zeros past the clip's end"""
    row = np.asarray(mono)[start:start + T]
    if len(row) < T:
        row = np.concatenate([row, np.zeros(T - len(row), row.dtype)])
    return row


def frame_of(start, n_frames, draw):
    """sample.py:212-230 for start in samples: (frame, whether randrange(duration) was drawn); draw(duration) makes that draw"""
    start_frame = int((start / float(T)) * FPS)
    duration = min(FPS, n_frames - start_frame)
    if duration > 0:
        return start_frame + draw(duration), True
    return min(start_frame, n_frames - 1), False


def cut(clips, records, resized=None):
    """(video (n, 224, 224, 3) uint8, audio (n, T) int16) of un-augmented records over clips [(frames, mono audio)].
    resized(frame, clip id) -> the frame as the sampler sees it (None: as it is)."""
    video, audio = [], []
    for r in records:
        fr = clips[int(r['video_clip'])][0][int(r['frame'])]
        if resized is not None:
            fr = resized(fr, int(r['video_clip']))
        x0, y0 = int(r['start_x']), int(r['start_y'])
        video.append(fr[x0:x0 + CROP, y0:y0 + CROP])
        audio.append(one_second(clips[int(r['audio_clip'])][1], int(r['audio_start'])))
    return np.stack(video), np.stack(audio)
