"""Audio embeddings of whole clips -- data/usc/features.py:18-28,224-240,256-323 (load_audio, get_vggish_frames_uniform,
get_l3_frames_uniform, compute_file_features).

The framing rule lives here and only here: `frame_table` turns clip lengths into one (start, lo, hi) row per 1-second
frame, and the C side (l3_embed_audio_frames, csrc/clips.hip) only follows the table on the GPU.  load_audio keeps its
PCM16-at-48-kHz contract; read_wav / read_audio are the reference's load_audio in full: any PCM or IEEE-float WAV file, resampled
on the GPU (resample.py, csrc/resample.hip) when its rate is not the one asked for.
"""
import os
import struct
import wave

import numpy as np

FRAME_LENGTH = 48000        # sr * 1 at the model's rate (features.py:279)


def frame_table(lengths, hop_length):
    """Frames of clips stored back to back, as get_l3_frames_uniform cuts them (features.py:276-300):

    - a clip of L < 48000 samples (L = 0 included) is one frame, padded with (48000 - L) // 2 zeros in front and the rest
      behind;
    - a clip of L >= 48000 samples gives 1 + (L - 48000) // hop_length frames, frame k = samples [k * hop, k * hop + 48000)
      and the tail dropped.  The reference's pad length `int(np.ceil(L - F) / hop) * hop - (L - F)` is never positive (the
      ceil acts on an integer before the division), so it never pads; reproduced as is.

    Returns (table, counts): table (n_frames, 3) int64 rows (start, lo, hi) in the coordinates of the concatenated clips --
    output sample j of a frame is samples[start + j] if lo <= start + j < hi, else 0 --, and counts (n_clips,) int64.
    """
    hop = int(hop_length)
    if hop < 1:
        raise ValueError('hop_length must be >= 1 sample (got %r)' % (hop_length,))
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if (L < 0).any():
        raise ValueError('clip lengths must be >= 0')
    off = np.zeros_like(L)
    if L.size > 1:
        off[1:] = np.cumsum(L)[:-1]
    short = L < FRAME_LENGTH
    counts = np.where(short, 1, 1 + (np.maximum(L, FRAME_LENGTH) - FRAME_LENGTH) // hop).astype(np.int64)
    n = int(counts.sum())
    clip = np.repeat(np.arange(L.size), counts)
    first = np.zeros_like(counts)
    if counts.size > 1:
        first[1:] = np.cumsum(counts)[:-1]
    k = np.arange(n, dtype=np.int64) - np.repeat(first, counts)
    table = np.empty((n, 3), np.int64)
    table[:, 0] = np.where(short[clip], off[clip] - (FRAME_LENGTH - L[clip]) // 2, off[clip] + k * hop)
    table[:, 1] = off[clip]
    table[:, 2] = off[clip] + L[clip]
    return table, counts


IMAGE_SIDE = 224            # the vision tower's input (data/avc/sample.py:182-183)


def image_table(shapes, resize=256, crop='center'):
    """Where raw frames stored back to back are resized to and cropped: one row {offset, H, W, Ho, Wo, y0, x0} per frame for
    l3_embed_vision_frames (csrc/frames.hip), which only follows the table on the GPU.

    shapes: (n, 2) frame sizes (H, W); frame i holds 3 * H * W bytes (HWC uint8) at the returned offset.
    resize: the shorter side after the resize, read_video's rule (data/avc/sample.py:303-305): scaling = resize / min(W, H),
    Wo = ceil(scaling * W), Ho = ceil(scaling * H).  None takes every frame as it is (Ho = H, Wo = W, the source bytes), and each
    side must then be at least 224.
    crop: 'center' (y0 = (Ho - 224) // 2, x0 = (Wo - 224) // 2) or an (n, 2) array of (y0, x0) in the resized frame.

    Returns (table, offsets): table (n, 7) int64 and offsets (n,) int64, the byte offset of each frame."""
    import math
    hw = np.asarray(shapes, dtype=np.int64).reshape(-1, 2)
    if (hw < 1).any():
        raise ValueError('frame sides must be >= 1')
    if resize is not None and int(resize) < IMAGE_SIDE:
        raise ValueError('resize must be >= %d or None (got %r)' % (IMAGE_SIDE, resize))
    n = hw.shape[0]
    table = np.empty((n, 7), np.int64)
    sizes = 3 * hw[:, 0] * hw[:, 1]
    table[:, 0] = np.cumsum(sizes) - sizes
    table[:, 1:3] = hw
    if resize is None:
        if (hw < IMAGE_SIDE).any():
            i = int(np.nonzero((hw < IMAGE_SIDE).any(axis=1))[0][0])
            raise ValueError('frame %d is %d x %d: without a resize every side must be >= %d'
                             % (i, hw[i, 0], hw[i, 1], IMAGE_SIDE))
        table[:, 3:5] = hw
    else:
        for i, (h, w) in enumerate(hw.tolist()):
            scaling = float(resize) / min(w, h)
            table[i, 3] = math.ceil(scaling * h)
            table[i, 4] = math.ceil(scaling * w)
    if isinstance(crop, str):
        if crop != 'center':
            raise ValueError("crop must be 'center' or an (n, 2) array of (y0, x0) (got %r)" % (crop,))
        table[:, 5:7] = (table[:, 3:5] - IMAGE_SIDE) // 2
    else:
        yx = np.asarray(crop, dtype=np.int64)
        if yx.shape != (n, 2):
            raise ValueError('crop must give one (y0, x0) per frame: shape %s, not %s' % ((n, 2), yx.shape))
        if (yx < 0).any() or (yx > table[:, 3:5] - IMAGE_SIDE).any():
            i = int(np.nonzero(((yx < 0) | (yx > table[:, 3:5] - IMAGE_SIDE)).any(axis=1))[0][0])
            raise ValueError('frame %d: the crop at (%d, %d) is outside the %d x %d resized frame'
                             % (i, yx[i, 0], yx[i, 1], table[i, 3], table[i, 4]))
        table[:, 5:7] = yx
    return table, table[:, 0].copy()


def load_audio(path, sr):
    """features.py:18-28 for PCM16 WAV files: int16 / 32768 (soundfile's float32 read), then the float32 mean over the
    channels.  The reference resamples other rates with resampy and reads any format soundfile knows; neither is a
    dependency here, so any other sample width or rate raises ValueError."""
    try:
        with wave.open(str(path), 'rb') as w:
            nch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            raw = w.readframes(n)
    except wave.Error as exc:
        raise ValueError('%s: not a PCM WAV file (%s); decode the audio and pass the array instead' % (path, exc))
    if width != 2:
        raise ValueError('%s: %d-bit samples; only 16-bit PCM WAV files are read here -- decode the audio and pass a float32 '
                         'array instead' % (path, 8 * width))
    if rate != sr:
        raise ValueError('%s: sample rate %d Hz, expected %d Hz; resample the audio and pass the array instead'
                         % (path, rate, sr))
    pcm = np.frombuffer(raw, dtype='<i2').reshape(-1, nch)
    return (pcm.astype(np.float32) / np.float32(32768)).mean(axis=-1)


# WAVE format tags (mmreg.h) that read_wav names when it refuses them
_WAVE_FORMATS = {0x0001: 'PCM', 0x0002: 'MS ADPCM', 0x0003: 'IEEE float', 0x0006: 'A-law', 0x0007: 'mu-law',
                 0x0011: 'IMA ADPCM', 0x0031: 'GSM 6.10', 0x0050: 'MPEG', 0x0055: 'MPEG Layer 3', 0xFFFE: 'extensible'}


def _wave_format_name(tag):
    return '%s (format tag 0x%04x)' % (_WAVE_FORMATS.get(tag, 'unknown'), tag)


def read_wav(path):
    """(samples, rate): a WAV file as sf.read(path, dtype='float32', always_2d=True) reads it, then the float32 mean over the
    channels (data/usc/features.py:22-23), without soundfile.  The RIFF chunks are parsed here, with libsndfile's conversions
    to float32 [3P]: 8-bit unsigned PCM (u - 128) / 128; 16-, 24- and 32-bit PCM float32(v) * 2^-(bits - 1); IEEE float 32 as
    stored, 64 cast to float32; WAVE_FORMAT_EXTENSIBLE with a PCM or float sub-format the same.  Any other encoding (ADPCM,
    A-law, mu-law, MPEG, ...) or a malformed file raises ValueError naming it."""
    with open(str(path), 'rb') as fh:
        raw = fh.read()
    if len(raw) < 12 or raw[0:4] != b'RIFF' or raw[8:12] != b'WAVE':
        raise ValueError('%s: not a RIFF WAVE file' % (path,))
    fmt, data, pos = None, None, 12
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack('<I', raw[pos + 4:pos + 8])[0]
        body = raw[pos + 8:pos + 8 + size]          # a data chunk whose size runs past the end of the file is cut there
        if cid == b'fmt ' and fmt is None:
            fmt = body
        elif cid == b'data' and data is None:
            data = body
        pos += 8 + size + (size & 1)
    if fmt is None or len(fmt) < 16:
        raise ValueError('%s: WAV file without a valid fmt chunk' % (path,))
    if data is None:
        raise ValueError('%s: WAV file without a data chunk' % (path,))
    tag, nch, rate, _, block, bits = struct.unpack('<HHIIHH', fmt[:16])
    if tag == 0xFFFE:
        if len(fmt) < 40:
            raise ValueError('%s: WAVE_FORMAT_EXTENSIBLE fmt chunk of %d bytes' % (path, len(fmt)))
        sub = struct.unpack('<H', fmt[24:26])[0]
        if sub not in (1, 3):
            raise ValueError('%s: unsupported WAV encoding: extensible with sub-format %s' % (path, _wave_format_name(sub)))
        tag = sub
    if tag not in (1, 3):
        raise ValueError('%s: unsupported WAV encoding: %s' % (path, _wave_format_name(tag)))
    if nch < 1 or rate < 1:
        raise ValueError('%s: %d channels at %d Hz' % (path, nch, rate))
    width = (bits + 7) // 8
    if (tag == 1 and width not in (1, 2, 3, 4)) or (tag == 3 and width not in (4, 8)) or block != width * nch:
        raise ValueError('%s: unsupported WAV encoding: %s with %d bits per sample, block of %d bytes'
                         % (path, _wave_format_name(tag), bits, block))
    n = len(data) // block
    b = np.frombuffer(data, dtype=np.uint8, count=n * block)
    if tag == 3:
        x = b.view('<f4' if width == 4 else '<f8').astype(np.float32)
    elif width == 1:
        x = (b.astype(np.float32) - np.float32(128)) / np.float32(128)
    elif width == 2:
        x = b.view('<i2').astype(np.float32) * np.float32(2.0 ** -15)
    elif width == 3:
        v = b.reshape(-1, 3).astype(np.int32)
        v = (v[:, 0] | (v[:, 1] << 8) | (v[:, 2] << 16)) << 8 >> 8          # sign-extend the 24-bit little-endian value
        x = v.astype(np.float32) * np.float32(2.0 ** -23)
    else:
        x = b.view('<i4').astype(np.float32) * np.float32(2.0 ** -31)
    return x.reshape(n, nch).mean(axis=-1), int(rate)


def read_audio(path, sr, device=0):
    """data/usc/features.py:18-28 (load_audio) in full: read_wav, then, when the file's rate is not `sr`, resampy.resample(data,
    sr_orig, sr) on the GPU (resample.resample, filter 'kaiser_best').  Returns float32 samples at `sr`."""
    from .resample import resample
    data, sr_orig = read_wav(path)
    if sr_orig != sr:
        data = resample(data, sr_orig, sr, device=device)
    return data


def get_l3_frames_uniform(audio, l3embedding_model, hop_size=0.1, sr=48000):
    """features.py:256-306: one embedding per 1-second frame of `audio` (a path to a PCM16 WAV file or a 1-D array at
    `sr`), frames every int(hop_size * sr) samples.  `l3embedding_model` is the audio EmbeddingModel load_embedding
    returns.  Returns (n_frames, D) float32."""
    from .model import EmbeddingModel
    if not isinstance(l3embedding_model, EmbeddingModel) or l3embedding_model.embedding_type != 'audio':
        raise TypeError('l3embedding_model must be the audio embedding model load_embedding(..., "audio", ...) returns')
    if sr != FRAME_LENGTH:
        raise ValueError('the audio embedding takes 1 s frames of %d samples: sr must be %d (got %r)'
                         % (FRAME_LENGTH, FRAME_LENGTH, sr))
    if isinstance(audio, (str, os.PathLike)):
        audio = load_audio(audio, sr)
    audio = np.asarray(audio, dtype=np.float32)
    if audio.ndim != 1:
        raise ValueError('audio must be 1-D (got shape %s)' % (audio.shape,))
    return l3embedding_model.predict_clips([audio], int(hop_size * sr))[0]


def get_vggish_frames_uniform(audio_path, hop_size=0.1, vggish_model=None):
    """features.py:224-240: the VGGish features of an audio file, one 128-vector per 0.96-second example every hop_size seconds
    (vggish.extract_vggish_embedding with frame_hop_sec=hop_size).  vggish_model: a vggish.VGGishModel to use instead of the one
    read from the default resources directory."""
    from .vggish import extract_vggish_embedding
    return extract_vggish_embedding(audio_path, frame_hop_sec=hop_size, vggish_model=vggish_model)


def compute_file_features(path, feature_type, l3embedding_model=None, **feature_args):
    """features.py:309-323: the features of one file, 'l3' or 'vggish' (feature_args: hop_size; vggish_model for 'vggish')"""
    if feature_type == 'l3':
        if not l3embedding_model:
            raise ValueError('Must provide L3 embedding model to use {} features'.format(feature_type))
        hop_size = feature_args.get('hop_size', 0.1)
        file_features = get_l3_frames_uniform(read_audio(path, FRAME_LENGTH), l3embedding_model, hop_size=hop_size)
    elif feature_type == 'vggish':
        hop_size = feature_args.get('hop_size', 0.1)
        file_features = get_vggish_frames_uniform(path, hop_size=hop_size, vggish_model=feature_args.get('vggish_model'))
    else:
        raise ValueError('Invalid feature type: {}'.format(feature_type))
    return file_features
