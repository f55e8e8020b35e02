"""Writes tests/golden/fold_driver_record.json: what classifier.train, train_svm_fold and cross_validate do on a small feature tree
with the native classifiers replaced by deterministic stand-ins (tests/fold_driver_ref.py) -- per case config.json and its key
order, the files of every fold directory, results.pkl, the ordered log of the stand-ins' calls (row counts, SHA-256 of the features
and labels they received, keyword arguments) and a SHA-256 of NumPy's global state afterwards.  tests/test_fold_driver_record.py
replays the cases and compares for equality, so the file is the behaviour of the commit it was generated on: it was written on the
parent of the commit that introduced the single fold driver and the single search body, from a separate work tree of that parent,

    PYTHONPATH=<work tree of the recorded commit>:tests python tests/golden/make_fold_driver_record.py

and is regenerated only when the drivers' behaviour is meant to change.  No GPU is needed.  The results and the call log are
committed as SHA-256 digests (fold_driver_ref.condensed); when a replay differs in one of them,

    python tests/golden/make_fold_driver_record.py --full PATH

writes the whole record of the commit it runs on to PATH instead, and two such files (of the recorded commit and of the one that
differs) show the difference.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(1, os.path.dirname(HERE))

import fold_driver_ref as ref  # noqa: E402


def main():
    full = sys.argv[2] if sys.argv[1:2] == ['--full'] else None
    ref.install()
    record = {}
    with tempfile.TemporaryDirectory() as root:
        tree = ref.write_tree(os.path.join(root, 'tree'))
        for k, (name, case) in enumerate(ref.cases().items()):
            whole = ref.run_case(case, tree, os.path.join(root, 'out%d' % k))
            print('%-40s %4d calls, folds %s' % (name, len(whole['calls']), whole['fold_dirs']))
            record[name] = whole if full else ref.condensed(whole)
    path = full or os.path.join(HERE, 'fold_driver_record.json')
    with open(path, 'w') as fh:          # one case per line
        fh.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(name), json.dumps(record[name], sort_keys=True, separators=(',', ':')))
                                   for name in sorted(record)) + '\n}\n')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
