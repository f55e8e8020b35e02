"""Audio embeddings of whole clips -- data/usc/features.py:18-28,256-306 (load_audio, get_l3_frames_uniform).

The framing rule lives here and only here: `frame_table` turns clip lengths into one (start, lo, hi) row per 1-second
frame, and the C side (l3_embed_audio_frames, csrc/clips.hip) only follows the table on the GPU.  Resampling and
non-PCM16 files are out of scope: decode / resample with any library and pass the array.
"""
import os
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
