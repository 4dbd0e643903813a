"""CPU-side checks of the top documents per topic (no device needed):
lda_topic_top_docs, its test hook and the ldatm_ mirrors are declared, bound
and exported and the ABI stays 8; bad arguments fail with a status and a
message before any device work; the numpy restatement every GPU expectation
comes from (topic_docs_numpy) is checked against an example worked by hand;
printTopicDocuments' text is checked from given arrays.  The GPU behaviour is
in test_topic_docs_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

import topic_docs_numpy as N

SAMPLER_CALLS = ["lda_topic_top_docs", "lda_debug_topic_docs_chunk_docs"]
MODEL_CALLS = ["ldatm_topic_top_docs", "ldatm_print_topic_documents", "ldatm_topic_documents_text",
               "ldatm_topic_documents_format"]
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
    L, _ = libs
    assert set(SAMPLER_CALLS) <= _declared(capi.HEADER_PATH, "lda_")
    assert set(SAMPLER_CALLS) <= set(capi.SIGNATURES)
    assert set(SAMPLER_CALLS) <= _exported(capi.LIB_PATH, "lda_")
    assert set(MODEL_CALLS) <= _declared(TM_HEADER, "ldatm_")
    assert set(MODEL_CALLS) <= set(tm.TM_SIGNATURES)
    assert set(MODEL_CALLS) <= _exported(tm.TM_LIB_PATH, "ldatm_")
    text = open(capi.HEADER_PATH).read()
    assert "#define LDA_TOPIC_DOCS_MAX %d\n" % capi.TOPIC_DOCS_MAX in text and capi.TOPIC_DOCS_MAX == 128
    assert "#define LDA_ABI_VERSION 8" in text and L.lda_abi_version() == 8


def test_sampler_call_rejects_a_null_context_and_the_hook_needs_none(libs):
    L, _ = libs
    ids = np.zeros(8, np.int64)
    out = np.zeros(8, np.int32)
    assert L.lda_topic_top_docs(None, 1, 0.0, 1, ids.ctypes.data, out.ctypes.data, out.ctypes.data) == -1
    assert b"null ctx" in L.lda_last_error()
    L.lda_debug_topic_docs_chunk_docs(5)
    L.lda_debug_topic_docs_chunk_docs(0)


def test_model_call_rejects_bad_arguments_before_any_device_work(libs, handle):
    """A model without documents and without a GPU: the argument checks come
    first, so each call names its own argument, not the missing device."""
    _, T = libs
    ids = np.zeros(4 * 129, np.int64)
    out = np.zeros(4 * 129, np.int32)
    i, p = ids.ctypes.data, out.ctypes.data
    assert T.ldatm_topic_top_docs(None, 1, 0.0, 1, i, p, p) == -1 and b"null" in T.ldatm_last_error()
    for n in (0, -1, capi.TOPIC_DOCS_MAX + 1):
        assert T.ldatm_topic_top_docs(handle, n, 0.0, 1, i, p, p) == -1
        assert b"LDA_TOPIC_DOCS_MAX" in T.ldatm_last_error()
    for s in (-1e-9, -1.0, math.nan, math.inf, -math.inf):
        assert T.ldatm_topic_top_docs(handle, 2, s, 1, i, p, p) == -1
        assert b"smoothing" in T.ldatm_last_error()
    for mt in (0, -4):
        assert T.ldatm_topic_top_docs(handle, 2, 1.0, mt, i, p, p) == -1
        assert b"min_tokens" in T.ldatm_last_error()
    for args in ((None, p, p), (i, None, p), (i, p, None)):
        assert T.ldatm_topic_top_docs(handle, 2, 1.0, 1, *args) == -1
        assert b"null output" in T.ldatm_last_error()
    # the text calls check the same arguments
    size = C.c_size_t()
    assert T.ldatm_topic_documents_text(None, 5, 1.0, 1, None, 0, C.byref(size)) == -1
    assert T.ldatm_topic_documents_text(handle, 0, 1.0, 1, None, 0, C.byref(size)) == -1
    assert b"LDA_TOPIC_DOCS_MAX" in T.ldatm_last_error()
    assert T.ldatm_print_topic_documents(handle, b"/nonexistent/x", 5, -1.0, 1) == -1
    assert b"smoothing" in T.ldatm_last_error()
    assert T.ldatm_print_topic_documents(None, b"/nonexistent/x", 5, 1.0, 1) == -1


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_n_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    assert callable(GibbsSampler.topic_top_docs)
    for name in ("topicDocuments", "getTopicDocuments", "printTopicDocuments", "topicDocumentsText"):
        assert callable(getattr(tm.ParallelTopicModel, name))
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    for bad in (0, -1, capi.TOPIC_DOCS_MAX + 1):
        with pytest.raises(ValueError, match="n must be in"):
            g.topic_top_docs(bad)
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        for bad in (0, capi.TOPIC_DOCS_MAX + 1):
            with pytest.raises(ValueError, match="n must be in"):
                m.topicDocuments(bad)
    finally:
        m._L = real
        m.close()


# ------------------------------------------------- the restatement, by hand
# six documents, K = 3 (topic 2 never appears):
#   d0 [0 0]  d1 [0 0]  d2 [0]  d3 [0 1 1 1]  d4 [1 0 0]  d5 []
DOC_OFF = np.array([0, 2, 4, 5, 9, 12, 12], np.int64)
Z = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0], np.int32)


def test_restatement_counts():
    nd = N.doc_topic_counts(Z, DOC_OFF, 3)
    assert nd.tolist() == [[2, 0, 0], [2, 0, 0], [1, 0, 0], [1, 3, 0], [2, 1, 0], [0, 0, 0]]


def test_restatement_smoothing_zero_min_tokens_two():
    """Topic 0: d0 and d1 tie at 1.0 (the smaller id first), d2 (1.0, one
    token) is under min_tokens, then d4 (2/3); d3 (1/4) is cut at n = 3.
    Topic 1: d3 (3/4), d4 (1/3): fewer than n.  Topic 2: none."""
    docs, cnt, lens = N.expected_topic_docs(Z, DOC_OFF, 3, 3, smoothing=0.0, min_tokens=2)
    assert docs.tolist() == [[0, 1, 4], [3, 4, -1], [-1, -1, -1]]
    assert cnt.tolist() == [[2, 2, 2], [3, 1, 0], [0, 0, 0]]
    assert lens.tolist() == [[2, 2, 3], [4, 3, 0], [0, 0, 0]]
    assert docs.dtype == np.int64 and cnt.dtype == np.int32 and lens.dtype == np.int32
    assert N.has_tie(3, 0.0, docs, cnt, lens)


def test_restatement_smoothing_zero_keeps_the_one_token_document():
    docs, cnt, lens = N.expected_topic_docs(Z, DOC_OFF, 3, 4, smoothing=0.0, min_tokens=1)
    assert docs[0].tolist() == [0, 1, 2, 4] and cnt[0].tolist() == [2, 2, 1, 2] and lens[0].tolist() == [2, 2, 1, 3]


def test_restatement_with_smoothing():
    """smoothing 1, K smoothing = 3.  Topic 0: d0 and d1 3/5, d2 2/4 and d4
    3/6 tie at 0.5 (d2 first), d3 2/7.  Topic 1: d3 4/7, d4 2/6."""
    docs, cnt, lens = N.expected_topic_docs(Z, DOC_OFF, 3, 5, smoothing=1.0, min_tokens=1)
    assert docs.tolist() == [[0, 1, 2, 4, 3], [3, 4, -1, -1, -1], [-1] * 5]
    w = N.weights(3, 1.0, cnt, lens)
    assert w[0].tolist() == [3 / 5, 3 / 5, 2 / 4, 3 / 6, 2 / 7] and w[1, :2].tolist() == [4 / 7, 2 / 6]
    assert docs[0, :1].tolist() == N.expected_topic_docs(Z, DOC_OFF, 3, 1, 1.0, 1)[0][0].tolist()
    got = tm.topic_document_weights(3, 1.0, docs, cnt, lens)
    assert np.array_equal(got[docs >= 0], w[docs >= 0]) and np.all(np.isnan(got[docs < 0]))


# ------------------------------------------------------------ the text
def test_topic_documents_text_from_given_arrays(libs):
    docs = np.array([[2, 1, -1], [5, -1, -1]], np.int64)
    cnt = np.array([[1, 3, 0], [7, 0, 0]], np.int32)
    lens = np.array([[1, 9, 0], [40, 0, 0]], np.int32)
    text = tm.format_topic_documents(docs, cnt, lens, smoothing=0.5, names=["n0", None, "file two"])
    w = N.weights(2, 0.5, cnt, lens)
    assert w[0, 0] == 0.75
    assert text == ("#topic doc name proportion ...\n"
                    "0 2 file two 0.75\n"
                    f"0 1 null-source {tm.format_double(w[0, 1])}\n"
                    f"1 5 null-source {tm.format_double(w[1, 0])}\n")
    assert tm.format_double(w[0, 1]) == "0.35" and float(tm.format_double(w[1, 0])) == 7.5 / 41.0
    # without names every document is null-source (K = 1: (1 + 0.5) / (1 + 0.5));
    # an all-padding table is the header alone
    assert tm.format_topic_documents(docs[:1, :1], cnt[:1, :1], lens[:1, :1], 0.5) == \
        "#topic doc name proportion ...\n0 2 null-source 1.0\n"
    empty = np.full((3, 2), -1, np.int64)
    zero = np.zeros((3, 2), np.int32)
    assert tm.format_topic_documents(empty, zero, zero) == "#topic doc name proportion ...\n"
    with pytest.raises(ValueError, match="one shape"):
        tm.format_topic_documents(docs, cnt[:, :2], lens)
