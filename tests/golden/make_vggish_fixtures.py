"""VGGish fixtures computed by the REFERENCE's own NumPy code, not by this repository's restatement.

Run on the build machine only (the reference tree is not on the GPU machine):

    python tests/golden/make_vggish_fixtures.py [path of the reference tree]

Imported from the reference by path and executed unmodified:

  data/usc/vggish/vggish_input.py:25-75        waveform_to_examples (log-mel + framing) at hops 0.96, 0.1, 0.37 -> vggish_examples.npz
  data/usc/vggish/mel_features.py:187-218      log_mel_spectrogram of the same audio                           -> vggish_logmel.npz
  data/usc/vggish/mel_features.py:114-184      spectrogram_to_mel_matrix(64, 257, 16000, 125, 7500)            -> vggish_logmel.npz
  data/usc/vggish/vggish_postprocess.py:21-94  Postprocessor.postprocess, quantize True / False               -> vggish_postprocess.npz

vggish_input.py imports resampy and the package's __init__ chain may import tensorflow; neither is installed nor used by the
functions above (the audio is already at 16 kHz), so both are satisfied by inert placeholder modules.  Only the .npz data written
here travels; no reference source is copied.
"""
import importlib
import importlib.abc
import importlib.machinery
import os
import sys
import tempfile
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PLACEHOLDERS = ('resampy', 'tensorflow')


class _Placeholder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split('.')[0] in PLACEHOLDERS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        m = mock.MagicMock(name=spec.name)
        m.__path__, m.__spec__, m.__name__, m.__loader__ = [], spec, spec.name, self
        return m

    def exec_module(self, module):
        pass


def seeded_audio(seed=20171021, seconds=2.0):
    """a few seconds at 16 kHz: noise under a slow envelope, two tones and a click"""
    rng = np.random.RandomState(seed)
    n = int(seconds * 16000)
    t = np.arange(n) / 16000.0
    x = 0.2 * rng.standard_normal(n) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.7 * t)) + 0.3 * np.sin(2 * np.pi * 440 * t) \
        + 0.1 * np.sin(2 * np.pi * 3100 * t)
    x[n // 3] += 0.9
    return x.astype(np.float32)


def main(ref):
    sys.meta_path.insert(0, _Placeholder())
    sys.path.insert(0, os.path.join(ref, 'data', 'usc'))
    vggish_input = importlib.import_module('vggish.vggish_input')
    mel_features = importlib.import_module('vggish.mel_features')
    vggish_postprocess = importlib.import_module('vggish.vggish_postprocess')

    audio = seeded_audio()
    out = dict(audio=audio, mel_matrix=mel_features.spectrogram_to_mel_matrix(
        num_mel_bins=64, num_spectrogram_bins=257, audio_sample_rate=16000, lower_edge_hertz=125, upper_edge_hertz=7500))
    out['log_mel'] = mel_features.log_mel_spectrogram(audio, audio_sample_rate=16000, log_offset=0.01, window_length_secs=0.025,
                                                      hop_length_secs=0.010, num_mel_bins=64, lower_edge_hertz=125,
                                                      upper_edge_hertz=7500)
    np.savez_compressed(os.path.join(HERE, 'vggish_logmel.npz'), **out)
    # (two files: each stays below the repository's limit for a committed file)
    ex = {'examples_hop_%s' % hop: np.ascontiguousarray(vggish_input.waveform_to_examples(audio, 16000, frame_hop_sec=hop))
          for hop in (0.96, 0.1, 0.37)}
    np.savez_compressed(os.path.join(HERE, 'vggish_examples.npz'), **ex)

    rng = np.random.RandomState(7)
    emb = np.maximum(rng.standard_normal((40, 128)), 0).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((128, 128)))
    pca = q * 1.6                                      # float64, like the arithmetic of np.dot on them
    means = 0.4 + 0.1 * rng.standard_normal(128)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'vggish_pca_params.npz')
        np.savez(path, pca_eigen_vectors=pca, pca_means=means)
        pp = vggish_postprocess.Postprocessor(path)
        np.savez_compressed(os.path.join(HERE, 'vggish_postprocess.npz'), embeddings=emb, pca_eigen_vectors=pca, pca_means=means,
                            quantized=pp.postprocess(emb), clipped=pp.postprocess(emb, quantize=False))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
