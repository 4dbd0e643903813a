"""CPU-side checks of held-out evaluation (no device needed): the new symbols
are declared and bound, NULL handles fail with a status and a message before
any device call, the Python faces refuse wrong shapes before any native call,
the result object's perplexity, and the model-level completion split.  The GPU
behaviour is in test_heldout_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm
from ldagibbssampling_amd.corpus import Corpus, document_completion_split

TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")
SAMPLER_SYMBOLS = ("lda_heldout_loglik", "lda_doc_completion")
MODEL_SYMBOLS = ("ldatm_heldout_loglik", "ldatm_evaluate", "ldatm_completion_split", "ldatm_set_held_out",
                 "ldatm_get_held_out_trace")


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


def test_new_symbols_in_headers_bindings_and_libraries(libs):
    L, T = libs
    text = open(capi.HEADER_PATH).read()
    for name in SAMPLER_SYMBOLS:
        assert re.search(r"\blda_status\s+%s\s*\(" % name, text), name
        assert name in capi.SIGNATURES and getattr(L, name) is not None
    text_tm = open(TM_HEADER).read()
    for name in MODEL_SYMBOLS:
        assert re.search(r"\blda_status\s+%s\s*\(" % name, text_tm), name
        assert name in tm.TM_SIGNATURES and getattr(T, name) is not None
    # the change only adds symbols: the ABI version stays, and the history says so
    assert "#define LDA_ABI_VERSION 8" in text and L.lda_abi_version() == 8
    assert re.search(r"lda_heldout_loglik and lda_doc_completion[^/]*version stays 8", text)


def test_token_batch_matches_the_kernel_header():
    h = open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "lda_kernels.h")).read()
    assert "constexpr int doc_completion_batch(int C) { return C <= 8 ? 64 : 16; }" in h
    assert [capi.doc_completion_batch(c) for c in (1, 2, 4, 8, 16, 32, 64)] == [64, 64, 64, 64, 16, 16, 16]


def test_null_arguments(libs, handle):
    L, T = libs
    theta = np.full((1, 4), 0.25)
    off = np.array([0, 1], np.int64)
    w = np.array([0], np.int32)
    out = np.zeros(1)
    p = lambda a: a.ctypes.data
    assert L.lda_heldout_loglik(None, 1, p(theta), p(off), p(w), p(out), None) == -1
    assert b"null" in L.lda_last_error()
    assert L.lda_doc_completion(None, 1, p(off), p(w), p(off), p(w), 10, 2, 2, 0, p(out), None, None) == -1
    assert b"null" in L.lda_last_error()
    assert T.ldatm_heldout_loglik(None, 1, p(theta), p(off), p(w), p(out), None) == -1
    assert b"null" in T.ldatm_last_error()
    assert T.ldatm_heldout_loglik(handle, 1, p(theta), p(off), p(w), None, None) == -1
    assert b"null doc_ll" in T.ldatm_last_error()
    assert T.ldatm_evaluate(None, 1, p(off), p(w), 10, 2, 2, 0, p(out), None, None, None) == -1
    assert b"null" in T.ldatm_last_error()
    assert T.ldatm_evaluate(handle, 1, p(off), p(w), 10, 2, 2, 0, None, None, None, None) == -1
    assert b"null doc_ll" in T.ldatm_last_error()
    assert T.ldatm_set_held_out(None, 1, p(off), p(w), 10, 10, 2, 2, 0) == -1
    assert T.ldatm_get_held_out_trace(None, None, None, 0, None) == -1
    assert T.ldatm_completion_split(4, 1, None, p(w), p(off), None, p(off), None) == -1
    assert b"null" in T.ldatm_last_error()


def test_set_held_out_on_the_host(libs, handle):
    """Setting and clearing a held-out set needs no device; bad settings are
    refused; the trace is empty before estimate()."""
    _, T = libs
    off = np.array([0, 2, 5], np.int64)
    w = np.array([0, 1, 2, 3, 99], np.int32)
    p = lambda a: a.ctypes.data
    assert T.ldatm_set_held_out(handle, 2, p(off), p(w), 10, 100, 10, 10, 0) == 0
    assert T.ldatm_set_held_out(handle, 2, p(off), p(w), 0, 100, 10, 10, 0) == 0
    assert T.ldatm_set_held_out(handle, 2, p(off), p(w), -1, 100, 10, 10, 0) == -1
    assert T.ldatm_set_held_out(handle, 2, p(off), p(w), 10, 100, 0, 10, 0) == -1      # thinning < 1
    bad = np.array([0, 3, 2], np.int64)
    assert T.ldatm_set_held_out(handle, 2, p(bad), p(w), 10, 100, 10, 10, 0) == -1
    assert b"monotone" in T.ldatm_last_error()
    n = C.c_int32(-1)
    assert T.ldatm_get_held_out_trace(handle, None, None, 0, C.byref(n)) == 0 and n.value == 0


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the shape check")


def test_python_faces_reject_wrong_shapes(libs):
    off, words = np.array([0, 2, 3], np.int64), np.array([0, 1, 2], np.int32)
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        for bad in (np.zeros((2, 5)), np.zeros(3), np.zeros((2, 2, 4))):
            with pytest.raises(ValueError, match="theta must have shape"):
                m.heldOutLogLikelihood(bad, off, words)
        with pytest.raises(ValueError, match="must have 3 entries"):
            m.heldOutLogLikelihood(np.full((2, 4), 0.25), off[:2], words[:2])
        with pytest.raises(ValueError, match="spans 3 tokens but words holds 2"):
            m.heldOutLogLikelihood(np.full((2, 4), 0.25), off, words[:2])
        with pytest.raises(ValueError, match="interval"):
            m.setHeldOut([tm.Instance([0])], -1)
    finally:
        m._L = real
        m.close()

    from ldagibbssampling_amd.sampler import GibbsSampler
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    for bad in (np.zeros((2, 5)), np.zeros(3), np.zeros((2, 2, 4))):
        with pytest.raises(ValueError, match="theta must have shape"):
            g.heldout_loglik(bad, off, words)
    with pytest.raises(ValueError, match="must have 4 entries"):
        g.heldout_loglik(np.full((3, 4), 0.25), off, words)
    with pytest.raises(ValueError, match="spans 3 tokens but words holds 4"):
        g.heldout_loglik(np.full((2, 4), 0.25), off, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="at least one offset"):
        g.heldout_loglik(np.zeros((0, 4)), [], [])
    with pytest.raises(ValueError, match="obs_off spans 3 tokens but words holds 1"):
        g.doc_completion(off, [0], off, words)
    with pytest.raises(ValueError, match="sc_off spans 3 tokens but words holds 1"):
        g.doc_completion(off, words, off, [0])
    with pytest.raises(ValueError, match="sc_off must have 3 entries"):
        g.doc_completion(off, words, [0, 3], words)


def test_result_perplexity():
    r = tm.HeldOutResult(-690.5, 100, np.array([-300.0, -390.5]), np.full((2, 4), 0.25))
    assert r.perplexity == float(np.exp(690.5 / 100))
    assert (r.logLikelihood, r.tokens) == (-690.5, 100)
    assert r.perDocument.shape == (2,) and r.theta.shape == (2, 4)
    assert np.isnan(tm.HeldOutResult(0.0, 0, np.zeros(0), np.zeros((0, 4))).perplexity)


def test_completion_split_equals_the_corpus_split(libs):
    """Out-of-vocabulary ids are dropped first (as ParallelTopicModel's
    inference drops them) and are not counted; what is left splits as
    corpus.document_completion_split does."""
    V = 30
    rng = np.random.default_rng(3)
    docs = []
    for L in (0, 1, 2, 3, 7, 8, 41, 5):
        w = rng.integers(0, V, L).astype(np.int32)
        if L >= 3:
            w[0], w[L // 2] = V, -2              # out of vocabulary, at a place that moves the middle
        if L == 5:
            w[:] = V + 3                         # nothing left of this one
        docs.append(w)
    kept = [w[(w >= 0) & (w < V)] for w in docs]
    off = np.zeros(len(kept) + 1, np.int64)
    np.cumsum([len(w) for w in kept], out=off[1:])
    obs_c, sc_c = document_completion_split(Corpus(off, np.concatenate(kept).astype(np.int32), V))
    obs_off, obs, sc_off, sc = tm.completion_split([tm.Instance(w) for w in docs], V)
    np.testing.assert_array_equal(obs_off, obs_c.doc_off)
    np.testing.assert_array_equal(sc_off, sc_c.doc_off)
    np.testing.assert_array_equal(obs, obs_c.words)
    np.testing.assert_array_equal(sc, sc_c.words)
    assert obs.dtype == np.int32 and sc.dtype == np.int32
    assert len(obs) + len(sc) == sum(len(w) for w in kept) < sum(len(w) for w in docs)
    assert sc_off[-1] - sc_off[-2] == 0          # the all-unknown document scores nothing
