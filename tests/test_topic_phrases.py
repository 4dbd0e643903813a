"""CPU-side checks of the topic phrases (no device needed): lda_topic_phrases,
lda_phrase_counts, lda_phrase_lookup, their test hook and the ldatm_ mirrors
are declared, bound and exported and the ABI stays 8; bad arguments fail with
a status and a message before any device work; the brute-force restatement
every GPU expectation comes from (topic_phrases_numpy) is checked against an
example worked by hand; the text and the multi-shard bound are checked from
typed-in arrays.  The GPU behaviour is in test_topic_phrases_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

import topic_phrases_numpy as N

SAMPLER_CALLS = ["lda_topic_phrases", "lda_phrase_counts", "lda_phrase_lookup", "lda_debug_phrase_table_slots"]
MODEL_CALLS = ["ldatm_topic_phrases", "ldatm_topic_phrases_text", "ldatm_print_topic_phrases",
               "ldatm_topic_phrases_format", "ldatm_topic_phrases_bound"]
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
    assert "#define LDA_PHRASE_LEN_MAX %d\n" % capi.PHRASE_LEN_MAX in text and capi.PHRASE_LEN_MAX == 32
    assert "#define LDA_PHRASES_MAX %d\n" % capi.PHRASES_MAX in text and capi.PHRASES_MAX == 128
    assert "#define LDA_ABI_VERSION 8" in text and L.lda_abi_version() == 8


def test_sampler_calls_reject_a_null_context_and_the_hook_needs_none(libs):
    L, _ = libs
    w = np.zeros(64, np.int32)
    o = np.zeros(8, np.int64)
    p, q = w.ctypes.data, o.ctypes.data
    assert L.lda_topic_phrases(None, 1, 2, 32, 1, p, p, q, q, q, q, q) == -1
    assert b"null ctx" in L.lda_last_error()
    assert L.lda_phrase_counts(None, 2, 32, 1, p, q, p, q) == -1
    assert b"null ctx" in L.lda_last_error()
    assert L.lda_phrase_lookup(None, 2, 32, 1, p, q, p, q, q) == -1
    assert b"null ctx" in L.lda_last_error()
    for slots in (64, 63, -1, 0):
        L.lda_debug_phrase_table_slots(slots)


def test_model_call_rejects_bad_arguments_before_any_device_work(libs, handle):
    """A model without documents and without a GPU: the argument checks come
    first, so each call names its own argument, not the missing device."""
    _, T = libs
    w = np.zeros(4 * 129 * 32, np.int32)
    o = np.zeros(4 * 129, np.int64)
    p, q = w.ctypes.data, o.ctypes.data
    outs = (p, p, q, q, q, q, q, p)
    assert T.ldatm_topic_phrases(None, 1, 2, 32, 1, *outs) == -1 and b"null" in T.ldatm_last_error()
    for n in (0, -1, capi.PHRASES_MAX + 1):
        assert T.ldatm_topic_phrases(handle, n, 2, 32, 1, *outs) == -1
        assert b"LDA_PHRASES_MAX" in T.ldatm_last_error()
    for lo, hi in ((1, 32), (0, 5), (5, 4), (2, 33), (-3, -2)):
        assert T.ldatm_topic_phrases(handle, 2, lo, hi, 1, *outs) == -1
        assert b"LDA_PHRASE_LEN_MAX" in T.ldatm_last_error()
    for mc in (0, -7):
        assert T.ldatm_topic_phrases(handle, 2, 2, 32, mc, *outs) == -1
        assert b"min_count" in T.ldatm_last_error()
    for i in range(len(outs)):
        args = list(outs)
        args[i] = None
        assert T.ldatm_topic_phrases(handle, 2, 2, 32, 1, *args) == -1
        assert b"null output" in T.ldatm_last_error()
    # the text calls check the same arguments
    size = C.c_size_t()
    assert T.ldatm_topic_phrases_text(None, 5, 2, 32, 1, None, 0, C.byref(size)) == -1
    assert T.ldatm_topic_phrases_text(handle, 0, 2, 32, 1, None, 0, C.byref(size)) == -1
    assert b"LDA_PHRASES_MAX" in T.ldatm_last_error()
    assert T.ldatm_print_topic_phrases(handle, b"/nonexistent/x", 5, 2, 40, 1) == -1
    assert b"LDA_PHRASE_LEN_MAX" in T.ldatm_last_error()
    assert T.ldatm_print_topic_phrases(handle, b"/nonexistent/x", 5, 2, 4, 0) == -1
    assert b"min_count" in T.ldatm_last_error()
    assert T.ldatm_print_topic_phrases(None, b"/nonexistent/x", 5, 2, 32, 1) == -1


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    assert callable(GibbsSampler.topic_phrases) and callable(GibbsSampler.phrase_counts)
    for name in ("topicPhrases", "getTopicPhrases", "printTopicPhrases", "topicPhrasesText"):
        assert callable(getattr(tm.ParallelTopicModel, name))
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    for bad in (0, -1, capi.PHRASES_MAX + 1):
        with pytest.raises(ValueError, match="n must be in"):
            g.topic_phrases(bad)
    for lo, hi in ((1, 4), (5, 4), (2, 33)):
        with pytest.raises(ValueError, match="lengths must satisfy"):
            g.topic_phrases(3, lo, hi)
    with pytest.raises(ValueError, match="one phrase per topic"):
        g.phrase_counts([0, 1], [(1, 2)])
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        for bad in (0, capi.PHRASES_MAX + 1):
            with pytest.raises(ValueError, match="n must be in"):
                m.topicPhrases(bad)
        with pytest.raises(ValueError, match="lengths must satisfy"):
            m.topicPhrases(3, 2, 33)
    finally:
        m._L = real
        m.close()


# ------------------------------------------------- the restatement, by hand
# four documents, K = 3, min_len 2, max_len 3 ('|' where the topic changes):
#   d0 words 1 2 3 | 1 2          z 0 0 0 | 1 1        the last run ends the document
#   d1 words 1 2 | 4 4 4 4        z 1 1 | 2 2 2 2      starts in d0's last topic: no join;
#                                                      then a run of max_len + 1
#   d2 words 1 2 5 | 1 2 | 7      z 0 0 0 | 2 2 | 0
#   d3 words 1 2 | 9 | 1 2 3      z 0 0 | 1 | 0 0 0    (1 2) is a prefix of (1 2 3) and (1 2 5)
DOC_OFF = np.array([0, 5, 11, 17, 23], np.int64)
WORDS = np.array([1, 2, 3, 1, 2, 1, 2, 4, 4, 4, 4, 1, 2, 5, 1, 2, 7, 1, 2, 9, 1, 2, 3], np.int32)
Z = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 0, 0, 0, 2, 2, 0, 0, 0, 1, 0, 0, 0], np.int32)


def test_restatement_runs():
    assert N.runs(Z, DOC_OFF) == [(0, 0, 3), (1, 3, 5), (1, 5, 7), (2, 7, 11), (0, 11, 14), (2, 14, 16), (0, 16, 17),
                                  (0, 17, 19), (1, 19, 20), (0, 20, 23)]


def test_restatement_table_typed_in():
    table, skipped = N.phrase_table(WORDS, Z, DOC_OFF, 2, 3)
    assert table == {(0, (1, 2, 3)): [2, 0],     # d0's start and d3's end
                     (1, (1, 2)): [2, 3],        # d0's end and d1's start: two runs, not one of four
                     (0, (1, 2, 5)): [1, 11],
                     (2, (1, 2)): [1, 14],
                     (0, (1, 2)): [1, 17]}
    assert skipped == 1                          # 4 4 4 4 is max_len + 1 long: not cut into pieces
    # with max_len 4 it qualifies, and d0 | d1 still do not join
    table4, skipped4 = N.phrase_table(WORDS, Z, DOC_OFF, 2, 4)
    assert skipped4 == 0 and table4[(2, (4, 4, 4, 4))] == [1, 7] and (1, (1, 2, 1, 2)) not in table4
    # min_len 3 drops the pairs
    table3, _ = N.phrase_table(WORDS, Z, DOC_OFF, 3, 3)
    assert table3 == {(0, (1, 2, 3)): [2, 0], (0, (1, 2, 5)): [1, 11]}


def test_restatement_order_and_arrays():
    w, lens, cnt, first, runs, distinct, skipped = N.expected_topic_phrases(WORDS, Z, DOC_OFF, 3, 4, 2, 3)
    # topic 0: count 2 first; then the prefix (1 2) before (1 2 5) at count 1
    assert w[0].tolist() == [[1, 2, 3], [1, 2, -1], [1, 2, 5], [-1, -1, -1]]
    assert lens.tolist() == [[3, 2, 3, 0], [2, 0, 0, 0], [2, 0, 0, 0]]
    assert cnt.tolist() == [[2, 1, 1, 0], [2, 0, 0, 0], [1, 0, 0, 0]]
    assert first.tolist() == [[0, 17, 11, -1], [3, -1, -1, -1], [14, -1, -1, -1]]
    assert runs.tolist() == [4, 2, 1] and distinct.tolist() == [3, 1, 1] and skipped == 1
    assert w.dtype == np.int32 and lens.dtype == np.int32 and cnt.dtype == np.int64 and first.dtype == np.int64
    assert N.content_tie(lens, cnt)
    # min_count 2 keeps the counted ones; runs and distinct are before min_count
    w2, lens2, cnt2, _, runs2, distinct2, _ = N.expected_topic_phrases(WORDS, Z, DOC_OFF, 3, 2, 2, 3, min_count=2)
    assert cnt2.tolist() == [[2, 0], [2, 0], [0, 0]] and lens2.tolist() == [[3, 0], [2, 0], [0, 0]]
    assert runs2.tolist() == [4, 2, 1] and distinct2.tolist() == [3, 1, 1]
    # n = 1 is the head of n = 4
    assert N.expected_topic_phrases(WORDS, Z, DOC_OFF, 3, 1, 2, 3)[0][:, 0].tolist() == w[:, 0].tolist()


# ------------------------------------------------------------ the text
def test_topic_phrases_text_from_given_arrays(libs):
    w, lens, cnt, *_ = N.expected_topic_phrases(WORDS, Z, DOC_OFF, 3, 4, 2, 3)
    names = ["w0", "new", "york", "city", None, "times"]
    assert tm.format_topic_phrases(w, lens, cnt, names) == ("#topic rank count phrase\n"
                                                            "0 0 2 new york city\n"
                                                            "0 1 1 new york\n"
                                                            "0 2 1 new york times\n"
                                                            "1 0 2 new york\n"
                                                            "2 0 1 new york\n")
    # without names, and for a word without one, the id stands
    assert tm.format_topic_phrases(w[2:], lens[2:], cnt[2:]) == "#topic rank count phrase\n0 0 1 1 2\n"
    assert tm.format_topic_phrases(np.array([[[4, 1]]]), np.array([[2]]), np.array([[7]]), names) == \
        "#topic rank count phrase\n0 0 7 4 new\n"
    empty = np.full((3, 2, 5), -1, np.int32)
    zero = np.zeros((3, 2), np.int32)
    assert tm.format_topic_phrases(empty, zero, zero) == "#topic rank count phrase\n"
    with pytest.raises(ValueError, match="max_len"):
        tm.format_topic_phrases(w, lens[:, :2], cnt)


# ------------------------------------------------- the multi-shard bound
def test_multi_shard_bound_from_typed_in_lists(libs):
    """Two shards, three topics, n = 4.  Topic 0: both lists are full with last
    counts 3 and 2, B = 5: the totals 9 and 6 are proven, 5 is not strictly
    above.  Topic 1: only shard 0's list is full (last count 1), B = 1: every
    total above 1 leads, the run stops at the first 1.  Topic 2: no list is
    full, B = 0: the union is everything, proven = n."""
    M = capi.PHRASES_MAX
    sc = np.zeros((2, 3, M), np.int64)
    sc[0, 0] = np.r_[[9, 7], np.full(M - 2, 3)]
    sc[1, 0] = np.r_[[4], np.full(M - 1, 2)]
    sc[0, 1] = np.r_[[5, 4, 2], np.full(M - 3, 1)]
    sc[1, 1, :3] = [6, 1, 1]
    sc[0, 2, :2] = [3, 1]
    totals = np.array([[9, 6, 5, 5], [11, 5, 2, 1], [3, 1, 0, 0]], np.int64)
    B, proven = tm.topic_phrases_bound(sc, totals)
    assert B.tolist() == [5, 1, 0]
    assert proven.tolist() == [2, 3, 4]
    eb, ep = N.bound_and_proven(sc, totals)
    assert eb.tolist() == B.tolist() and ep.tolist() == proven.tolist()
    # one shard whose lists are not full proves everything
    B1, p1 = tm.topic_phrases_bound(sc[1:, 1:], totals[1:])
    assert B1.tolist() == [0, 0] and p1.tolist() == [4, 4]
    with pytest.raises(ValueError, match="PHRASES_MAX"):
        tm.topic_phrases_bound(sc[:, :, :5], totals)
