"""The NumPy oracle of out-of-bag scoring at nested forest sizes (l3_forest_oob in csrc/forest.hip): for the
trees in order, the rows a tree's bootstrap sample missed get the class fractions of the leaf they reach added to their sums, in
float64, and snapshots of the sums and of the number of such trees are taken at the prefixes.  The walk is forest_ref.predict_proba's.
The aggregation (aggregate) is separate from the walk so that it can be fed sklearn's own trees.  It shares no code with
l3embedding_amd."""
import numpy as np

import forest_ref as R


def tree_fractions(forest, X, t):
    """(n, C) float64: counts / their sum of the leaf every row reaches in tree t (forest_ref.predict_proba of that tree alone)"""
    nodes = slice(int(forest['tree_off'][t]), int(forest['tree_off'][t + 1]))
    one = {k: v[nodes] for k, v in forest.items() if k != 'tree_off'}
    one['tree_off'] = np.array([0, nodes.stop - nodes.start], np.int64)
    return R.predict_proba(one, X)          # / 1.0 at its end changes no bit


def aggregate(fractions, masks, prefixes):
    """fractions: per tree, in tree order, the (n, C) class fractions of its leaves; masks: per tree the (n) bool of the rows it left
    out -> (sums (G, n, C) float64, n_oob (G, n) int32): the snapshots after tree prefixes[g] - 1"""
    sums = n_oob = None
    out_sums, out_n = [], []
    for t, (frac, mask) in enumerate(zip(fractions, masks)):
        if sums is None:
            sums, n_oob = np.zeros(frac.shape, np.float64), np.zeros(frac.shape[0], np.int32)
        sums[mask] += frac[mask]
        n_oob[mask] += 1
        if t + 1 in prefixes:
            out_sums.append(sums.copy()), out_n.append(n_oob.copy())
    assert len(out_sums) == len(prefixes)
    return np.stack(out_sums), np.stack(out_n)


def oob(forest, X, boot, prefixes):
    """l3_forest_oob's sums and n_oob of the rows X under the multiplicities boot (n_trees, n), at the ascending prefixes"""
    T = int(max(prefixes))
    return aggregate((tree_fractions(forest, X, t) for t in range(T)), (np.asarray(boot[t]) == 0 for t in range(T)), list(prefixes))


def oob_of_fit(forest, X, random_state, prefixes):
    """oob() with the multiplicities a fit draws: bootstrap(seed_t, n) of the seeds of random_state"""
    n = len(X)
    seeds = R.tree_seeds(random_state, int(max(prefixes)))
    return oob(forest, X, [R.bootstrap(s, n) for s in seeds], prefixes)


def make_oracle_handle(base):
    """`base` (the _lib.Forest interface on the oracles: forest_search_ref.make_oracle_handle's class) with l3_forest_oob's method"""
    class OobOracleForest(base):
        def oob(self, boot, prefixes=None, labels=None, outputs=('correct',), chunk_rows=0, stage_bytes=0):
            T = self.forest['tree_off'].size - 1
            prefixes = [T] if prefixes is None else [int(p) for p in prefixes]
            assert np.asarray(boot).shape == (T, self.n) and all(1 <= p <= T for p in prefixes)
            assert all(a < b for a, b in zip(prefixes, prefixes[1:]))
            sums, n_oob = oob(self.forest, self.X, boot, prefixes)
            out = dict(sums=sums, n_oob=n_oob, pred=sums.argmax(axis=2).astype(np.int32))
            if labels is not None:
                out['correct'] = (out['pred'] == np.asarray(labels)[None, :]).sum(axis=1).astype(np.int64)
            return {k: out[k] for k in outputs}

    return OobOracleForest


def decision(sums):
    """sklearn 0.19's normalisation of one forest's sums (n, C): NaN for a row that no tree left out"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return sums / sums.sum(axis=1)[:, None]

