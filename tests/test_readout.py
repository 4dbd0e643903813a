"""CPU-side checks of the device readouts (no device needed): lda_top_words,
lda_doc_top_topics, lda_doc_counts and their ldatm_ mirrors are declared,
bound and exported; bad arguments fail with a status and a message before any
device work; the Python faces check their arguments before any native call and
fail loudly without a GPU.  The GPU behaviour is in test_readout_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

SAMPLER_CALLS = ["lda_top_words", "lda_doc_top_topics", "lda_doc_counts"]
MODEL_CALLS = ["ldatm_top_words", "ldatm_doc_top_topics", "ldatm_doc_counts"]
TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")


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


def _declared(path, prefix):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, text))


def _exported(path, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\bT (%s\w+)" % prefix, out))


def test_symbols_in_header_binding_and_exports(libs):
    assert set(SAMPLER_CALLS) <= _declared(capi.HEADER_PATH, "lda_")
    assert set(SAMPLER_CALLS) <= set(capi.SIGNATURES)
    assert set(SAMPLER_CALLS) <= _exported(capi.LIB_PATH, "lda_")
    assert set(MODEL_CALLS) <= _declared(TM_HEADER, "ldatm_")
    assert set(MODEL_CALLS) <= set(tm.TM_SIGNATURES)
    assert set(MODEL_CALLS) <= _exported(tm.TM_LIB_PATH, "ldatm_")


def test_caps_match_the_header_and_the_abi_stays_8(libs):
    L, _ = libs
    text = open(capi.HEADER_PATH).read()
    assert "#define LDA_TOP_WORDS_MAX %d\n" % capi.TOP_WORDS_MAX in text
    assert "#define LDA_TOP_TOPICS_MAX %d\n" % capi.TOP_TOPICS_MAX in text
    assert capi.TOP_WORDS_MAX == 64 and capi.TOP_TOPICS_MAX == 64
    assert L.lda_abi_version() == 8


def test_sampler_calls_reject_a_null_context(libs):
    L, _ = libs
    out = np.zeros(8, np.int32)
    assert L.lda_top_words(None, 1, out.ctypes.data, out.ctypes.data) == -1
    assert L.lda_last_error()
    assert L.lda_doc_top_topics(None, 1, 0, 1, None, out.ctypes.data, out.ctypes.data) == -1
    assert L.lda_last_error()
    assert L.lda_doc_counts(None, 0, 1, None, out.ctypes.data) == -1
    assert L.lda_last_error()


def test_model_calls_reject_bad_arguments_before_any_device_work(libs, handle):
    """A model without documents and without a GPU: the argument checks come
    first, so each call names its own argument, not the missing device."""
    _, T = libs
    out = np.zeros(4 * 65, np.int32)
    p = out.ctypes.data
    assert T.ldatm_top_words(None, 1, p, p) == -1 and b"null" in T.ldatm_last_error()
    assert T.ldatm_doc_top_topics(None, 1, 0, None, p, p) == -1 and b"null" in T.ldatm_last_error()
    assert T.ldatm_doc_counts(None, 0, None, p) == -1 and b"null" in T.ldatm_last_error()
    for n in (0, -1, capi.TOP_WORDS_MAX + 1):
        assert T.ldatm_top_words(handle, n, p, p) == -1
        assert b"LDA_TOP_WORDS_MAX" in T.ldatm_last_error()
    assert T.ldatm_top_words(handle, 1, None, p) == -1 and b"null output" in T.ldatm_last_error()
    assert T.ldatm_top_words(handle, 1, p, None) == -1 and b"null output" in T.ldatm_last_error()
    for m in (0, -3, capi.TOP_TOPICS_MAX + 1):
        assert T.ldatm_doc_top_topics(handle, m, 0, None, p, p) == -1
        assert b"LDA_TOP_TOPICS_MAX" in T.ldatm_last_error()
    # the model holds no documents: any id is out of range, M must be D = 0
    ids = np.array([0], np.int64)
    assert T.ldatm_doc_counts(handle, 1, ids.ctypes.data, p) == -1 and b"out of range" in T.ldatm_last_error()
    assert T.ldatm_doc_top_topics(handle, 2, 1, ids.ctypes.data, p, p) == -1
    assert b"out of range" in T.ldatm_last_error()
    assert T.ldatm_doc_counts(handle, 3, None, p) == -1 and b"M must be" in T.ldatm_last_error()
    assert T.ldatm_doc_counts(handle, -1, None, p) == -1
    # M = 0 succeeds and touches nothing, without a device
    assert T.ldatm_doc_counts(handle, 0, None, None) == 0
    assert T.ldatm_doc_top_topics(handle, 2, 0, None, None, None) == 0


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    for name in ("top_words", "doc_top_topics", "doc_counts"):
        assert callable(getattr(GibbsSampler, name))
    for name in ("getTopWords", "topTopics", "topWords", "docTopTopics", "docCounts"):
        assert callable(getattr(tm.ParallelTopicModel, name))
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    for bad in (0, -1, capi.TOP_WORDS_MAX + 1):
        with pytest.raises(ValueError, match="n must be in"):
            g.top_words(bad)
    for bad in (0, capi.TOP_TOPICS_MAX + 1):
        with pytest.raises(ValueError, match="m must be in"):
            g.doc_top_topics(bad)
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        for bad in (0, capi.TOP_WORDS_MAX + 1):
            with pytest.raises(ValueError, match="numWords must be in"):
                m.getTopWords(bad)
        for bad in (0, capi.TOP_TOPICS_MAX + 1):
            with pytest.raises(ValueError, match="n must be in"):
                m.topTopics(n=bad)
    finally:
        m._L = real
        m.close()


def test_python_faces_fail_loudly_without_a_gpu(libs):
    """The first use of the GPU fails with LdaError when there is none (no
    host fall-back); with one, the same calls answer."""
    import torch
    from ldagibbssampling_amd.sampler import GibbsSampler
    off = np.array([0, 2, 3], np.int64)
    words = np.array([0, 1, 2], np.int32)
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    try:
        il = tm.InstanceList(tm.Alphabet(range(3)))
        il.add(tm.Instance([0, 1]))
        il.add(tm.Instance([2]))
        m.addInstances(il)
        calls = (lambda: m.getTopWords(2), lambda: m.topTopics(n=2), lambda: m.docCounts([1]),
                 lambda: m.getTopicProbabilities(0), lambda: m.displayTopWords(3),
                 lambda: m.documentTopics(0.0, 2))
        if not torch.cuda.is_available():
            with pytest.raises(capi.LdaError):
                GibbsSampler(4, 3, off, words, np.full(4, 0.25), 0.01, seed=1)
            for call in calls:
                with pytest.raises(capi.LdaError):
                    call()
        else:
            assert len(m.getTopWords(2)) == 4 and m.docCounts([1]).sum() == 1
    finally:
        m.close()
