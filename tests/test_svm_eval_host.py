"""SVC.evaluate and train_svm(evaluate_on_device=...) without a GPU (l3embedding_amd/svm.py, classifier.py): the ValueErrors that
evaluate raises before any device work, and the signatures."""
import inspect

import numpy as np
import pytest

from l3embedding_amd import _build, _lib, classifier, svm


class _NoDevice(svm.SVC):
    """a fitted model whose device handle must never be asked for"""

    def _handle(self):
        raise AssertionError('evaluate reached the device before checking its arguments')


def _fitted(probability=True, classes=(3, 5, 9), D=7):
    m = _NoDevice(probability=probability)
    nc = len(classes)
    m.classes_ = np.array(classes)
    m.shape_fit_ = (20, D)
    m._gamma = 1.0 / D
    m.support_ = np.arange(nc, dtype=np.int32)
    m.support_vectors_ = np.zeros((nc, D), np.float32)
    m._sv_start = np.arange(nc + 1, dtype=np.int64)
    m._dual_coef_ = np.zeros((nc - 1, nc))
    m._intercept_ = np.zeros(nc * (nc - 1) // 2)
    m.probA_ = m.probB_ = np.zeros(nc * (nc - 1) // 2) if probability else np.empty(0)
    return m


X = np.zeros((6, 7), np.float32)


def test_hinge_loss_needs_labels():
    with pytest.raises(ValueError, match='hinge_loss'):
        _fitted().evaluate(X, outputs=('predict', 'hinge_loss'))


def test_file_outputs_need_file_idxs():
    for out in ('file_proba', 'file_predict'):
        with pytest.raises(ValueError, match='file_idxs'):
            _fitted().evaluate(X, outputs=(out,))


def test_probability_outputs_need_probability():
    for out in ('predict_proba', 'file_proba', 'file_predict'):
        with pytest.raises(ValueError, match='probability=False'):
            _fitted(probability=False).evaluate(X, file_idxs=[(0, 6)], outputs=(out,))


def test_wrong_width():
    with pytest.raises(ValueError, match='expecting 7'):
        _fitted().evaluate(np.zeros((6, 8), np.float32))


def test_label_outside_classes():
    with pytest.raises(ValueError, match='not in classes_'):
        _fitted().evaluate(X, y=[3, 5, 9, 4, 3, 3], outputs=('hinge_loss',))
    with pytest.raises(ValueError, match='not in classes_'):
        _fitted().evaluate(X, y=[3, 5, 9, 10, 3, 3], outputs=('hinge_loss',))
    with pytest.raises(ValueError, match='one label per row'):
        _fitted().evaluate(X, y=[3, 5], outputs=('hinge_loss',))


def test_bad_file_ranges_and_unknown_outputs():
    for bad in ([(0, 7)], [(2, 2)], [(-1, 3)], []):
        with pytest.raises(ValueError, match='file_idxs'):
            _fitted().evaluate(X, file_idxs=bad, outputs=('file_predict',))
    with pytest.raises(ValueError, match='unknown outputs'):
        _fitted().evaluate(X, outputs=('votes',))
    with pytest.raises(ValueError, match='not fitted'):
        svm.SVC().evaluate(X)


def test_unpickled_state_sets_the_model_again():
    m = _fitted()
    m._model_set, m._resident = True, True
    state = m.__getstate__()
    assert state['_h'] is None and state['_model_set'] is False and state['_resident'] is False
    assert m._model_set and m._resident           # the live object keeps its own


def test_signatures():
    sig = inspect.signature(classifier.train_svm)
    assert sig.parameters['evaluate_on_device'].default is False
    sig = inspect.signature(svm.SVC.evaluate)
    assert list(sig.parameters)[1:] == ['X', 'y', 'file_idxs', 'outputs']
    assert sig.parameters['y'].default is None and sig.parameters['file_idxs'].default is None
    assert set(svm.EVALUATE_OUTPUTS) == {'predict', 'decision_function', 'hinge_loss', 'predict_proba', 'file_proba', 'file_predict'}
    for name in ('set_data_dev', 'get_rows', 'set_model', 'score'):
        assert callable(getattr(_lib.SVM, name))
    assert callable(_lib.op_svm_tail)


def test_scoring_source_is_built_without_contraction():
    assert 'svm_eval.hip' in _build.SOURCES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['svm_eval.hip']
