"""The NumPy oracle of scoring a forest at nested sizes (l3_forest_score in csrc/forest.hip): the forest of
the first n trees, its probabilities with the sums in tree order, a file's mean with its rows added in row order, and the
_lib.Forest interface on the oracle (tests/forest_ref.py's forest plus this scoring) for the host tests.  It shares no code with
l3embedding_amd."""
import numpy as np

import forest_ref as R

SCORE_OUTPUTS = ('pred', 'correct', 'file_mean', 'file_pred', 'proba')


def prefix_forest(forest, n):
    """the first n trees of a forest in forest_ref's flat arrays"""
    nodes = int(forest['tree_off'][n])
    return {k: (v[:n + 1] if k == 'tree_off' else v[:nodes]).copy() for k, v in forest.items()}


def prefix_proba(forest, X, prefixes):
    """(G, n, C) float64: forest_ref.predict_proba of each prefix (its sums run in tree order, so a prefix's is a prefix of them)"""
    return np.stack([R.predict_proba(prefix_forest(forest, int(p)), X) for p in prefixes])


def file_mean(proba, files):
    """(F, C): each file's rows added one after the other in row order, / their number"""
    out = np.zeros((len(files), proba.shape[1]), np.float64)
    for i, (s, e) in enumerate(files):
        acc = np.zeros(proba.shape[1], np.float64)
        for r in range(int(s), int(e)):
            acc = acc + proba[r]
        out[i] = acc / np.float64(int(e) - int(s))
    return out


def score(forest, X, prefixes, labels=None, files=None, outputs=('pred',)):
    """l3_forest_score's outputs on the host -> dict, each with the leading axis G"""
    proba = prefix_proba(forest, X, prefixes)
    pred = proba.argmax(axis=2).astype(np.int32)
    out = dict(proba=proba, pred=pred)
    if labels is not None:
        out['correct'] = (pred == np.asarray(labels)[None, :]).sum(axis=1).astype(np.int64)
    if files is not None:
        out['file_mean'] = np.stack([file_mean(p, files) for p in proba])
        out['file_pred'] = out['file_mean'].argmax(axis=2).astype(np.int32)
    return {k: out[k] for k in outputs}


def make_oracle_handle(base):
    """`base` (tests/test_forest_host.py's OracleForest, the _lib.Forest interface on forest_ref) with l3_forest_score's method"""
    class ScoringOracleForest(base):
        scored = []          # (source, prefixes) of every call, for the tests

        def score(self, X=None, feat=None, lo=0, hi=None, resident=False, prefixes=None, labels=None, files=None, outputs=('pred',),
                  chunk_rows=0, stage_bytes=0):
            assert feat is None and (X is None) == bool(resident)
            rows = self.X if resident else np.ascontiguousarray(X, np.float32)
            T = self.forest['tree_off'].size - 1
            prefixes = [T] if prefixes is None else [int(p) for p in prefixes]
            assert prefixes and all(1 <= p <= T for p in prefixes) and all(a < b for a, b in zip(prefixes, prefixes[1:]))
            type(self).scored.append(('resident' if resident else 'host', tuple(prefixes)))
            return score(self.forest, rows, prefixes, labels=labels, files=files, outputs=outputs)

    return ScoringOracleForest
