"""What the FoldBank tests share (test_foldbank_host.py, test_foldbank_gpu.py): small written feature trees and the comparison of a
split with the one usc.get_split reads."""
import os

import numpy as np

from l3embedding_amd import usc


def write_tree(root, dataset, D=6, seed=0, per_frame_labels=False):
    """<root>/features/<dataset>/l3/x/fold1 .. foldN.  us8k: augmented copies ('_' in the name) in every fold, fold 5 holding
    nothing else; everywhere one file of a single vector (1-d X) and files of 1 to 8 frames."""
    feats = os.path.join(str(root), 'features', dataset, 'l3', 'x')
    r = np.random.RandomState(seed)
    for fold in range(1, usc.DATASET_NUM_FOLDS[dataset] + 1):
        d = os.path.join(feats, 'fold%d' % fold)
        os.makedirs(d)
        names = ['clip%d.npz' % i for i in range(4)]
        if dataset == 'us8k':
            names = ['clip0_bg1.npz', 'clip1_ps2.npz'] if fold == 5 else names + ['clip0_bg1.npz', 'clip2_ps-1.npz']
        for i, name in enumerate(names):
            n = r.randint(1, 9)
            label = (fold + i) % 3
            if i == 1 and not per_frame_labels:
                X = r.randn(D).astype(np.float32)          # a single vector
            else:
                X = r.randn(n, D).astype(np.float32)
            y = np.full(X.shape[0], label) if per_frame_labels else np.array(label)
            np.savez(os.path.join(d, name), X=X, y=y)
    return feats


def assert_same_split(got, want):
    assert (got is None) == (want is None)
    if want is None:
        return
    assert sorted(got) == sorted(want)
    assert got['filenames'] == want['filenames']
    for k in ('labels', 'file_idxs'):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        np.testing.assert_array_equal(a, b, err_msg=k)
    a = got['features'].to_host() if isinstance(got['features'], usc.DeviceFeatures) else got['features']
    b = want['features']
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
