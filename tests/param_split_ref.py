"""What the tests of the parameter search without a validation fold share (test_param_split_host.py, test_param_split_gpu.py): a
small written feature tree whose training rows can be cut by class, and readers of a fold's files."""
import json
import os
import pickle

import numpy as np

from l3embedding_amd import usc

GRID_POINTS = 9          # the MLP's grid: three learning rates by three weight decays


def write_tree(root, dataset='esc50', D=24, files=6, seed=0):
    """<root>/features/<dataset>/l3/x/fold1 .. foldN: `files` files of 3 to 8 frames of D floats per fold, one label per file, three
    classes that every fold holds twice -- so every class has members enough for usc.stratified_shuffle_split in both feature
    modes (24 files in four training folds: 20 / 4 at 0.15)."""
    feats = os.path.join(str(root), 'features', dataset, 'l3', 'x')
    r = np.random.RandomState(seed)
    for fold in range(1, usc.DATASET_NUM_FOLDS[dataset] + 1):
        d = os.path.join(feats, 'fold%d' % fold)
        os.makedirs(d)
        for i in range(files):
            label = (fold + i) % 3
            X = (r.randn(r.randint(3, 9), D) + 0.5 * label).astype(np.float32)
            np.savez(os.path.join(d, 'clip%d.npz' % i), X=X, y=np.array(label))
    return feats


def load_pickle(path):
    with open(path, 'rb') as fh:
        return pickle.load(fh)


def load_config(fold_dir):
    with open(os.path.join(fold_dir, 'config.json')) as fh:
        return json.load(fh)
