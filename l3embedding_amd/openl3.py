"""The per-tower OpenL3 model files and the deployed pipeline's framing.

Replaces (reference notebooks, relative to the reference tree):
  notebooks/extract_embedding_models_from_avc_models.ipynb     a trained AVC model cut into openl3_audio_<repr>_<subset>.h5 and
                                                               openl3_image_<repr>_<subset>.h5, each tower up to its embedding layer
  notebooks/extract_spectrogram_models_from_avc_models.ipynb   openl3_audio_<repr>_<subset>_spec.h5, the audio tower without its
                                                               front-end layer: the "spec model", input (F, 199, 1)
  notebooks/pimodel.ipynb cell 12                              whole seconds of a clip, one spectrogram each, the spec model

The files are Keras `save_weights` files of a FLAT model: one top-level group per layer that has weights, in layer order, each
with its `weight_names`; in the audio file the (Mel)spectrogram layer's constants come first (three for the mel models -- the
two DFT kernels and the filterbank --, two for the linear model), and the spec file is the same list without them.  Unverified
against Keras, as the nested layout of kerasfile.py is: no Keras is at hand to read them back.  Reading places
every tensor by layer and weight name, also below a `model_weights/` group as `Model.save` writes it.

    python -m l3embedding_amd.openl3 extract WEIGHTS MODEL_TYPE SUBSET OUTDIR [--compress gzip bz2]
"""
import argparse
import bz2
import gzip
import os
from collections import OrderedDict

import numpy as np

from . import h5lite
from . import kerasfile

# input representation -> the AVC model type whose audio tower it names
INPUT_REPRS = OrderedDict([('linear', 'cnn_L3_kapredbinputbn'), ('mel128', 'cnn_L3_melspec1'), ('mel256', 'cnn_L3_melspec2')])
# embedding size -> MaxPooling2D pool of the embedding layer's output
AUDIO_POOLINGS = {
    'linear': {6144: (8, 8), 512: (32, 24)},
    'mel128': {6144: (4, 8), 512: (16, 24)},
    'mel256': {6144: (8, 8), 512: (32, 24)},
}
IMAGE_POOLINGS = {8192: (7, 7), 512: (28, 28)}
FRAME = 48000
COMPRESSORS = {'gzip': ('.gz', gzip.open), 'bz2': ('.bz2', bz2.BZ2File)}


def model_type_of(input_repr):
    if input_repr not in INPUT_REPRS:
        raise ValueError('input_repr must be one of %s (got %r)' % (list(INPUT_REPRS), input_repr))
    return INPUT_REPRS[input_repr]


def repr_of(model_type):
    for r, mt in INPUT_REPRS.items():
        if mt == model_type:
            return r
    raise ValueError('no OpenL3 input representation for model type %r (one of %s)' % (model_type, list(INPUT_REPRS.values())))


def frame_table(lengths):
    """The deployed pipeline's framing of clips stored back to back: every whole second, hop 48000, the tail dropped.  A clip
    shorter than one second has no frame: ValueError.  Returns (table (n_frames, 3) int64 rows {start, lo, hi}, counts) in
    features.frame_table's form."""
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if (L < FRAME).any():
        bad = int(np.flatnonzero(L < FRAME)[0])
        raise ValueError('clip %d has %d samples: less than one second at 48 kHz' % (bad, int(L[bad])))
    counts = L // FRAME
    off = np.concatenate([[0], np.cumsum(L)[:-1]]).astype(np.int64) if L.size else np.zeros(0, np.int64)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64) if L.size else np.zeros(0, np.int64)
    clip = np.repeat(np.arange(L.size), counts)
    k = np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(first, counts)
    table = np.empty((k.size, 3), np.int64)
    table[:, 0] = off[clip] + k * FRAME
    table[:, 1] = off[clip]
    table[:, 2] = off[clip] + L[clip]
    return table, counts


# ---- the flat layout ------------------------------------------------------------------------------------------------------------
def tower_layers(table, model_type, tower):
    """OrderedDict layer -> [parameter names] of one tower ('audio_model' / 'vision_model') in layer order, each layer's weights
    in the order Keras lists them (kerasfile.keras_groups' names; trainable before non-trainable inside a layer)."""
    names = kerasfile.keras_groups(table, model_type)[tower]
    order = [n for n, _, _ in table if n.startswith(tower + '/')]          # get_weights order: layer by layer
    layers = OrderedDict()
    for n in order:
        layers.setdefault(n.split('/')[1], [])
    for n in names:                                                         # trainable first inside each layer
        layers[n.split('/')[1]].append(n)
    return layers


def frontend_layer(layers):
    """name of the (Mel)spectrogram layer: the tower's first, the one that holds the DFT kernels"""
    first = next(iter(layers))
    if not any(n.endswith('/real_kernels') for n in layers[first]):
        raise ValueError('the first audio layer "%s" holds no DFT kernels' % first)
    return first


def _write_flat(path, layers, named):
    root = h5lite.Group()
    root.attrs['layer_names'] = np.array([ln.encode('utf8') for ln in layers])
    root.attrs['backend'] = b'tensorflow'
    root.attrs['keras_version'] = b'2.0.9'
    for ln, pnames in layers.items():
        g = root.create_group(ln)
        wnames = [kerasfile._tf_name(p) for p in pnames]
        g.attrs['weight_names'] = np.array([w.encode('utf8') for w in wnames])
        for p, w in zip(pnames, wnames):
            g.create_dataset(w, np.asarray(named[p], dtype=np.float32))
    h5lite.write_file(path, root)


def _compressed_copies(path, compress):
    out = []
    for kind in compress:
        if kind not in COMPRESSORS:
            raise ValueError('compress entries must be among %s (got %r)' % (sorted(COMPRESSORS), kind))
        suffix, opener = COMPRESSORS[kind]
        with open(path, 'rb') as src, opener(path + suffix, 'wb') as dst:
            dst.write(src.read())
        out.append(path + suffix)
    return out


def extract_models(model_or_weights_path, model_type, subset, output_dir, compress=()):
    """Cuts an AVC model -- an L3Model, or the path of its weight file -- into the three OpenL3 files of its input representation
    in output_dir, with gzip / bz2 copies beside them for every entry of `compress`.  Returns {'audio', 'image', 'spec'} -> path."""
    from . import model as l3model
    input_repr = repr_of(model_type)
    compress = tuple(compress)
    for kind in compress:
        if kind not in COMPRESSORS:
            raise ValueError('compress entries must be among %s (got %r)' % (sorted(COMPRESSORS), kind))
    m = model_or_weights_path
    if not isinstance(m, l3model.L3Model):
        m = l3model.load_model(m, model_type)
    if m.model_type != model_type:
        raise ValueError('the model is a %s, not a %s' % (m.model_type, model_type))
    table, named = m.param_table(), m._weights_dict()
    audio = tower_layers(table, model_type, 'audio_model')
    image = tower_layers(table, model_type, 'vision_model')
    fe = frontend_layer(audio)
    spec = OrderedDict((ln, p) for ln, p in audio.items() if ln != fe)
    os.makedirs(output_dir, exist_ok=True)
    stem = os.path.join(output_dir, 'openl3_%%s_%s_%s%%s.h5' % (input_repr, subset))
    paths = {'audio': stem % ('audio', ''), 'image': stem % ('image', ''), 'spec': stem % ('audio', '_spec')}
    _write_flat(paths['audio'], audio, named)
    _write_flat(paths['image'], image, named)
    _write_flat(paths['spec'], spec, named)
    for p in paths.values():
        _compressed_copies(p, compress)
    return paths


def _open_tree(path):
    """The file's group tree; a .gz / .bz2 copy is inflated first; `model_weights/` (Model.save) is stepped into."""
    opener = gzip.open if path.endswith('.gz') else bz2.BZ2File if path.endswith('.bz2') else None
    if opener is not None:
        import tempfile
        with opener(path, 'rb') as src, tempfile.NamedTemporaryFile(suffix='.h5') as tmp:
            tmp.write(src.read())
            tmp.flush()
            root = h5lite.read_file(tmp.name)
    else:
        root = h5lite.read_file(path)
    if 'layer_names' not in root.attrs and isinstance(root.children.get('model_weights'), h5lite.Group):
        root = root.children['model_weights']
    if 'layer_names' not in root.attrs:
        raise ValueError('%s is not a keras weight file (no layer_names attribute)' % path)
    return root


def read_flat(path):
    """-> OrderedDict layer -> OrderedDict weight name -> float32 array, of every layer group that has weights, in file order"""
    root = _open_tree(path)
    out = OrderedDict()
    for ln in np.atleast_1d(root.attrs['layer_names']):
        ln = ln.decode('utf8') if isinstance(ln, bytes) else str(ln)
        g = root.children.get(ln)
        if g is None:
            raise ValueError('layer group "%s" missing in %s' % (ln, path))
        wn = g.attrs.get('weight_names')
        if wn is None or np.asarray(wn).dtype.kind != 'S':
            continue
        out[ln] = OrderedDict((n.decode('utf8'), np.asarray(g[n.decode('utf8')], dtype=np.float32)) for n in np.atleast_1d(wn))
    return out


def _tower_weights(path, table, model_type, tower, optional=()):
    """{parameter name: array} of one tower from a flat file, placed by layer and weight name (kerasfile._match_group's rules inside
    a layer).  Layers named in `optional` may be absent (the spec file has no front-end layer)."""
    shapes = {n: tuple(s) for n, s, _ in table}
    layers = tower_layers(table, model_type, tower)
    have = read_flat(path)
    named = OrderedDict()
    for ln, pnames in layers.items():
        if ln not in have:
            if ln in optional:
                continue
            raise ValueError('layer "%s" of the %s missing in %s' % (ln, tower, path))
        picked, _ = kerasfile._match_group(ln, pnames, list(have[ln]))
        for w, p in zip(picked, pnames):
            arr = have[ln][w]
            if tuple(arr.shape) != shapes[p]:
                raise ValueError('shape mismatch for %s: file %s has %s, model expects %s' % (p, w, arr.shape, shapes[p]))
            named[p] = arr
    extra = [ln for ln in have if ln not in layers]
    if extra:
        raise ValueError('%s holds layers the %s of %s does not have: %s' % (path, tower, model_type, extra))
    return named


def _embedding(path, input_repr, tower, pool, frontend, seed, device):
    from . import model as l3model
    model_type = model_type_of(input_repr)
    m = l3model.L3Model(model_type, seed=seed, device=device, frontend=frontend)
    table = m.param_table()
    optional = ()
    if tower == 'audio_model':
        optional = (frontend_layer(tower_layers(table, model_type, tower)),)
    named = _tower_weights(path, table, model_type, tower, optional)
    # everything the file does not hold -- the other tower, the head and, for a spec file, the DFT and mel constants -- keeps the
    # values the engine generates
    full = OrderedDict(m._weights_dict())
    full.update(named)
    m._assign(full)
    return l3model.EmbeddingModel(m, 'audio' if tower == 'audio_model' else 'vision', pool)


def load_audio_embedding(path, input_repr, embedding_size, frontend='kapre', seed=20180123, device=0):
    """An EmbeddingModel from openl3_audio_<repr>_<subset>.h5 or its _spec form (also .gz / .bz2, and below model_weights/).
    frontend: 'kapre' or 'minispec' (the deployed pipeline's spectrogram); a spec file carries no DFT or mel constants, which then
    keep the stock values."""
    pools = AUDIO_POOLINGS[input_repr] if input_repr in AUDIO_POOLINGS else {}
    model_type_of(input_repr)
    if embedding_size not in pools:
        raise ValueError('embedding_size must be one of %s for %s (got %r)' % (sorted(pools), input_repr, embedding_size))
    return _embedding(path, input_repr, 'audio_model', pools[embedding_size], frontend, seed, device)


def load_image_embedding(path, input_repr, embedding_size, seed=20180123, device=0):
    """An EmbeddingModel from openl3_image_<repr>_<subset>.h5 (also .gz / .bz2, and below model_weights/)."""
    model_type_of(input_repr)
    if embedding_size not in IMAGE_POOLINGS:
        raise ValueError('embedding_size must be one of %s (got %r)' % (sorted(IMAGE_POOLINGS), embedding_size))
    return _embedding(path, input_repr, 'vision_model', IMAGE_POOLINGS[embedding_size], 'kapre', seed, device)


def main(argv=None):
    p = argparse.ArgumentParser(description='Cut a trained AVC model into the OpenL3 audio, image and spectrogram-input model files.')
    sub = p.add_subparsers(dest='command')
    sub.required = True
    ex = sub.add_parser('extract', help='write openl3_{audio,image}_<repr>_<subset>.h5 and openl3_audio_<repr>_<subset>_spec.h5')
    ex.add_argument('weights', help='weight file of the trained AVC model')
    ex.add_argument('model_type', help='one of %s' % ', '.join(INPUT_REPRS.values()))
    ex.add_argument('subset', help="the subset the model was trained on, e.g. 'music' or 'env'")
    ex.add_argument('outdir')
    ex.add_argument('--compress', nargs='*', default=(), choices=sorted(COMPRESSORS), help='also write compressed copies')
    args = p.parse_args(argv)
    for kind, path in sorted(extract_models(args.weights, args.model_type, args.subset, args.outdir, args.compress).items()):
        print('%s %s' % (kind, path))


if __name__ == '__main__':
    main()
