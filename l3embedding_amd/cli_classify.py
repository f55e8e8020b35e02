"""Label audio files with a trained L3 embedding and a trained downstream classifier, on the GPU (the inference step of the
reference's notebooks/pimodel.ipynb) driving l3embedding_amd.sound.SoundClassifier.

    python -m l3embedding_amd.cli_classify --model-dir <run dir> --weights <l3 weights .h5> --model-type cnn_L3_melspec2 \\
        --pooling-type original [--hop-size 0.1] a.wav b.wav ...

One JSON line per file on standard output: {"path": ..., "class": <class index>, "proba": [...]}.
"""
import argparse
import json
import logging
import sys

# (long flag, dest, argparse settings, help)
_OPTIONS = [
    ('--model-dir', 'model_dir', dict(type=str, required=True),
     "a fold's run directory of the classifier: config.json, min_max_scaler.pkl, stdizer.pkl and model.h5 or model.pkl"),
    ('--weights', 'weights', dict(type=str, required=True), 'weight file of the trained L3 model'),
    ('--model-type', 'model_type', dict(type=str, required=True), 'L3 model type, e.g. cnn_L3_melspec2'),
    ('--pooling-type', 'pooling_type', dict(type=str, default='original'), "pooling of the audio embedding: 'original' or 'short'"),
    ('--hop-size', 'hop_size', dict(type=float, default=0.1), 'seconds between the 1 s frames of a file'),
    ('--frontend', 'frontend', dict(type=str, default='kapre', choices=('kapre', 'minispec')),
     "the audio front-end: 'kapre', the layer the model was trained with, or 'minispec', the spectrogram of pimodel.ipynb cell 12 "
     '(with --hop-size 1.0 the run is then that notebook from the file to the label)'),
]


def build_parser():
    p = argparse.ArgumentParser(description='Classify WAV files with an L3 audio embedding and a trained sound classifier on the GPU.')
    for flag, dest, settings, text in _OPTIONS:
        p.add_argument(flag, dest=dest, help=text, **settings)
    p.add_argument('files', nargs='+', help='WAV files of any sample rate')
    return p


def main(argv=None, out=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, stream=sys.stderr)
    from .model import load_embedding
    from .sound import SoundClassifier
    embedding = load_embedding(args.weights, args.model_type, 'audio', args.pooling_type, frontend=args.frontend)
    got = SoundClassifier.from_run(embedding, args.model_dir, hop_size=args.hop_size).predict_files(args.files)
    out = out or sys.stdout
    for path, cls, proba in zip(args.files, got['file_predict'], got['file_proba']):
        out.write(json.dumps({'path': path, 'class': int(cls), 'proba': [float(v) for v in proba]}) + '\n')


if __name__ == '__main__':
    main()
