"""The fold drivers and both parameter searches against a record of what they did before they were put together from one fold body
and one search body (tests/golden/fold_driver_record.json, written by tests/golden/make_fold_driver_record.py on that parent commit):
with deterministic stand-ins for the native classifiers, every case must write the same config.json (keys in the same order), the
same files and the same results, hand the stand-ins the same rows with the same arguments in the same order, and leave NumPy's
global stream where it was left then.  Equality throughout (results and the call log through SHA-256 digests of their canonical
JSON: fold_driver_ref.condensed); no GPU."""
import json
import os

import pytest

import fold_driver_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, 'golden', 'fold_driver_record.json')) as _fh:
    RECORD = json.load(_fh)


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return ref.write_tree(tmp_path_factory.mktemp('fold_driver') / 'tree')


def test_the_record_holds_the_cases():
    assert sorted(RECORD) == sorted(ref.cases()) and len(RECORD) == 14


@pytest.mark.parametrize('name', sorted(ref.cases()))
def test_case_equals_the_record(tree, tmp_path, monkeypatch, name):
    ref.install(monkeypatch.setattr)
    got = ref.condensed(ref.run_case(ref.cases()[name], tree, tmp_path))
    want = RECORD[name]
    hint = ': make_fold_driver_record.py --full on both commits shows the difference'
    assert sorted(got) == sorted(want)
    for part in ('fold_dirs', 'files', 'numpy_state'):
        assert got.get(part) == want.get(part), part
    assert len(got['folds']) == len(want['folds'])
    for g, w in zip(got['folds'], want['folds']):
        assert g['config_keys'] == w['config_keys']
        assert g['config'] == w['config']
        assert g['files'] == w['files']
        assert g['results'] == w['results'], 'results.pkl' + hint
    assert got.get('results') == want.get('results'), 'the top-level results.pkl' + hint
    assert got['calls']['order'] == want['calls']['order']
    assert got['calls'] == want['calls'], 'what the stand-ins received' + hint
