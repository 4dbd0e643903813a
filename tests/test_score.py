"""CPU-side checks of the prediction-scoring entry points (no device needed):
NULL handles and outputs fail with a status and a message before any device
call, and the Python faces refuse a theta of the wrong shape before any native
call.  The GPU behaviour is in test_score_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm


@pytest.fixture(scope="module")
def libs():
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(tm.TM_LIB_PATH)):
        from ldagibbssampling_amd.build import build_library
        build_library()
    return capi.load(), tm.load_tm()


@pytest.fixture()
def handle(libs):
    _, T = libs
    h = C.c_void_p()
    assert T.ldatm_create(C.byref(h), 4, 1.0, 0.01) == 0
    yield h
    T.ldatm_destroy(h)


def test_lda_score_docs_null_ctx(libs):
    L, _ = libs
    theta = np.full((1, 4), 0.25)
    out = np.zeros((1, 1))
    for metric in (capi.SCORE_METRICS["cosine"], capi.SCORE_METRICS["mse"]):
        assert L.lda_score_docs(None, metric, 1, theta.ctypes.data, 0, 1, None, out.ctypes.data) == -1
        assert L.lda_last_error()


def test_ldatm_score_theta_null_arguments(libs, handle):
    _, T = libs
    theta = np.full((1, 4), 0.25)
    out = np.zeros((1, 1))
    assert T.ldatm_score_theta(None, 0, 1, theta.ctypes.data, 1, None, out.ctypes.data) == -1
    assert b"null" in T.ldatm_last_error()
    assert T.ldatm_score_theta(handle, 0, 1, theta.ctypes.data, 1, None, None) == -1
    assert b"null scores" in T.ldatm_last_error()


def test_ldatm_score_null_arguments(libs, handle):
    _, T = libs
    off = np.array([0, 1], np.int64)
    w = np.array([0], np.int32)
    out = np.zeros((1, 1))
    args = (1, off.ctypes.data, w.ctypes.data, 10, 2, 2, 0, 1, None)
    assert T.ldatm_score(None, 0, *args, out.ctypes.data, None) == -1
    assert b"null" in T.ldatm_last_error()
    assert T.ldatm_score(handle, 0, *args, None, None) == -1
    assert b"null scores" in T.ldatm_last_error()


def test_ldatm_score_top_null_arguments(libs, handle):
    _, T = libs
    theta = np.full((1, 4), 0.25)
    ids = np.zeros((1, 2), np.int64)
    sc = np.zeros((1, 2))
    assert T.ldatm_score_top(None, 0, 1, theta.ctypes.data, 2, ids.ctypes.data, sc.ctypes.data) == -1
    assert b"null" in T.ldatm_last_error()
    assert T.ldatm_score_top(handle, 0, 1, theta.ctypes.data, 2, None, sc.ctypes.data) == -1
    assert b"null output" in T.ldatm_last_error()
    assert T.ldatm_score_top(handle, 0, 1, theta.ctypes.data, 2, ids.ctypes.data, None) == -1
    assert b"null output" in T.ldatm_last_error()


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the shape check")


def test_python_faces_reject_wrong_theta_shape(libs):
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        inf = m.getInferencer()
        for bad in (np.zeros((2, 5)), np.zeros(3), np.zeros((2, 2, 4))):
            with pytest.raises(ValueError, match="theta must have shape"):
                m.scoreDistributions(bad)
            with pytest.raises(ValueError, match="theta must have shape"):
                m.topDocuments(bad, 3)
        with pytest.raises(ValueError, match="metric"):
            m.scoreDistributions(np.full((1, 4), 0.25), metric="euclid")
        with pytest.raises(ValueError, match="metric"):
            inf.scoreInstances([tm.Instance([0])], metric="euclid")
    finally:
        m._L = real
        m.close()

    from ldagibbssampling_amd.sampler import GibbsSampler
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    with pytest.raises(ValueError, match="theta must have shape"):
        g.score_docs(np.zeros((2, 5)))
    with pytest.raises(ValueError, match="metric"):
        g.score_docs(np.full((1, 4), 0.25), metric="euclid")


def test_metric_names_match_the_header():
    text = open(capi.HEADER_PATH).read()
    assert "#define LDA_SCORE_COSINE 0" in text and "#define LDA_SCORE_MSE 1" in text
    assert capi.SCORE_METRICS == {"cosine": 0, "mse": 1}
    assert "#define LDA_ABI_VERSION 8" in text
