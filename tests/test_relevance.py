"""CPU-side checks of the relevance-ranked topic words, the salient terms and
the LDAvis data (no device needed): the new calls are declared, bound and
exported and the ABI stays 8; bad arguments fail with a status and a message of
their own before any device work; the numpy restatement every GPU expectation
comes from (relevance_numpy) is checked against an example worked by hand;
printRelevantWords' text is checked from given arrays; the classical MDS and
its sign rule on three points with known distances.  The GPU behaviour is in
test_relevance_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

import relevance_numpy as N

SAMPLER_CALLS = ["lda_relevant_words", "lda_salient_words", "lda_word_rows", "lda_debug_relevance_slab_rows"]
MODEL_CALLS = ["ldatm_relevant_words", "ldatm_salient_words", "ldatm_word_rows", "ldatm_relevant_words_format",
               "ldatm_relevant_words_text", "ldatm_print_relevant_words"]
TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")
INVALID = -1


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
    assert "#define LDA_RELEVANCE_LAMBDAS_MAX %d\n" % capi.RELEVANCE_LAMBDAS_MAX in text
    assert "#define LDA_SALIENT_WORDS_MAX %d\n" % capi.SALIENT_WORDS_MAX in text
    assert capi.RELEVANCE_LAMBDAS_MAX == 128 and capi.SALIENT_WORDS_MAX == 256
    assert "#define LDA_ABI_VERSION 8" in text and L.lda_abi_version() == 8
    # the lambdas a pass handles: 64 KiB of LDS at 12 bytes x 64 topics x n per list
    assert [capi.relevance_batch(n) for n in (1, 10, 11, 21, 22, 42, 43, 64)] == [8, 8, 4, 4, 2, 2, 1, 1]


def test_sampler_calls_reject_a_null_context_and_the_hook_needs_none(libs):
    L, _ = libs
    lam = np.array([0.6])
    out = np.zeros(64, np.int64)
    p = out.ctypes.data
    assert L.lda_relevant_words(None, 1, 1, lam.ctypes.data, p, p, p, p, p) == INVALID
    assert b"null ctx" in L.lda_last_error()
    assert L.lda_salient_words(None, 1, p, p, p, p) == INVALID and b"null ctx" in L.lda_last_error()
    assert L.lda_word_rows(None, 0, None, None, None) == INVALID and b"null ctx" in L.lda_last_error()
    L.lda_debug_relevance_slab_rows(64)
    L.lda_debug_relevance_slab_rows(0)


def test_model_calls_name_the_bad_argument_before_any_device_work(libs, handle):
    """K = 4, no documents, possibly no GPU: every check comes before the
    first use of a device, so each failure names its own argument."""
    _, T = libs
    K, n = 4, 3
    big = np.zeros(129 * K * 65, np.float64)
    p = big.ctypes.data
    lam = np.linspace(0.0, 1.0, 129)
    lp = lam.ctypes.data

    def rel(nn, L, lams, outs=(p, p, p, p, p), h=handle):
        return T.ldatm_relevant_words(h, nn, L, lams, *outs)

    assert rel(n, 1, lp, h=None) == INVALID and b"null" in T.ldatm_last_error()
    for bad in (0, capi.TOP_WORDS_MAX + 1):
        assert rel(bad, 1, lp) == INVALID and b"LDA_TOP_WORDS_MAX" in T.ldatm_last_error()
    for bad in (0, 129):
        assert rel(n, bad, lp) == INVALID and b"LDA_RELEVANCE_LAMBDAS_MAX" in T.ldatm_last_error()
    assert rel(n, 1, None) == INVALID and b"null lambdas" in T.ldatm_last_error()
    for bad in (-1e-9, 1.0 + 1e-9, math.nan, math.inf):
        one = np.array([0.5, bad])
        assert rel(n, 2, one.ctypes.data) == INVALID and b"lambda must be finite" in T.ldatm_last_error()
    for i in range(5):
        outs = [p] * 5
        outs[i] = None
        assert rel(n, 1, lp, tuple(outs)) == INVALID and b"null output" in T.ldatm_last_error()
    # the limits themselves pass the argument checks: what fails then is the model without documents
    assert rel(capi.TOP_WORDS_MAX, 128, lp) != 0 and b"LDA_" not in T.ldatm_last_error()

    assert T.ldatm_salient_words(None, 5, p, p, p, p) == INVALID
    for bad in (0, capi.SALIENT_WORDS_MAX + 1):
        assert T.ldatm_salient_words(handle, bad, p, p, p, p) == INVALID
        assert b"LDA_SALIENT_WORDS_MAX" in T.ldatm_last_error()
    for i in range(4):
        outs = [p] * 4
        outs[i] = None
        assert T.ldatm_salient_words(handle, 5, *outs) == INVALID and b"null output" in T.ldatm_last_error()

    ids = np.array([0, -1], np.int32)
    assert T.ldatm_word_rows(None, 0, None, None, None) == INVALID
    assert T.ldatm_word_rows(handle, -1, ids.ctypes.data, p, p) == INVALID and b"bad sizes" in T.ldatm_last_error()
    assert T.ldatm_word_rows(handle, 2, None, p, p) == INVALID and b"null word list" in T.ldatm_last_error()
    assert T.ldatm_word_rows(handle, 2, ids.ctypes.data, p, p) == INVALID and b"out of range" in T.ldatm_last_error()
    assert T.ldatm_word_rows(handle, 0, None, None, None) == 0      # M = 0 touches nothing

    size = C.c_size_t()
    assert T.ldatm_relevant_words_text(None, 5, 0.6, None, 0, C.byref(size)) == INVALID
    assert T.ldatm_relevant_words_text(handle, 0, 0.6, None, 0, C.byref(size)) == INVALID
    assert b"LDA_TOP_WORDS_MAX" in T.ldatm_last_error()
    assert T.ldatm_print_relevant_words(handle, b"/nonexistent/x", 5, 1.5) == INVALID
    assert b"lambda must be finite" in T.ldatm_last_error()
    assert T.ldatm_print_relevant_words(None, b"/nonexistent/x", 5, 0.6) == INVALID


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.V, g.D, g._h, g._L = 4, 10, 3, None, _NoNative()
    for bad in (0, -1, capi.TOP_WORDS_MAX + 1):
        with pytest.raises(ValueError, match="n must be in"):
            g.relevant_words(bad)
    for bad in ([], np.linspace(0, 1, 129), -1e-9, 1.0 + 1e-9, [0.5, math.nan], math.inf, [[0.1, 0.2]]):
        with pytest.raises(ValueError, match="lambda"):
            g.relevant_words(5, bad)
    for bad in (0, capi.SALIENT_WORDS_MAX + 1):
        with pytest.raises(ValueError, match="n must be in"):
            g.salient_words(bad)
    for bad in ([-1], [3, 10]):
        with pytest.raises(ValueError, match="word ids"):
            g.word_rows(bad)
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        for bad in (0, capi.TOP_WORDS_MAX + 1):
            for call in (m.relevantWords, m.getRelevantWords, m.relevantWordsText,
                         lambda n: m.printRelevantWords("/nonexistent/x", n)):
                with pytest.raises(ValueError, match="n must be in"):
                    call(bad)
            with pytest.raises(ValueError, match="R must be in"):
                m.prepareVis(bad)
        for bad in (-0.1, 1.1, math.nan):
            for call in (lambda x: m.relevantWords(5, x), lambda x: m.getRelevantWords(5, x),
                         lambda x: m.relevantWordsText(5, x), lambda x: m.printRelevantWords("/nonexistent/x", 5, x)):
                with pytest.raises(ValueError, match="lambda"):
                    call(bad)
        with pytest.raises(ValueError, match="one value"):
            m.getRelevantWords(5, [0.1, 0.2])
        for bad in (0, capi.SALIENT_WORDS_MAX + 1):
            with pytest.raises(ValueError, match="n must be in"):
                m.salientWords(bad)
            with pytest.raises(ValueError, match="n must be in"):
                m.getSalientWords(bad)
        with pytest.raises(ValueError, match="word ids"):
            m.wordRows([2, -1])
        for bad in (0.0, -0.25, 1.5, math.nan, math.inf):
            with pytest.raises(ValueError, match="lambdaStep"):
                m.prepareVis(5, bad)
            with pytest.raises(ValueError, match="lambdaStep"):
                m.saveVis("/nonexistent/x", 5, bad)
    finally:
        m._L = real
        m.close()


# ------------------------------------------------- the restatement, by hand
# four words, two topics, beta = 0.25 (V beta = 1):
#          k0  k1   tw
#   w0      8   2   10
#   w1      1   0    1
#   w2      3   3    6
#   w3      0   4    4
#   nwsum  12   9    N = 21
NW = np.array([[8, 2], [1, 0], [3, 3], [0, 4]], np.int64)
NWSUM = np.array([12, 9], np.int64)
BETA = 0.25
TW = [10, 1, 6, 4]


def _lp(w, k):
    return math.log((NW[w, k] + BETA) / (NWSUM[k] + 1.0))


def _ltp(w):
    return math.log(TW[w] / 21.0)


def test_the_restatement_ranks_the_worked_example():
    """Topic 0 by probability (lambda = 1): w0 (8.25/13), w2 (3.25/13), w1
    (1.25/13).  By lift (lambda = 0): w1, all of whose single token is the
    topic's (2.02), then w0 (1.33), then w2 (0.875): the two orders differ.
    Topic 1: w3, w2, w0 under both.  n = 4: one empty slot per topic."""
    ids, cnt, tot, lp, ll = N.expected_relevant(NW, NWSUM, BETA, 4, [0.0, 1.0, 0.5])
    assert ids.dtype == np.int32 and cnt.dtype == np.int32 and tot.dtype == np.int64 and ids.shape == (3, 2, 4)
    assert ids[1].tolist() == [[0, 2, 1, -1], [3, 2, 0, -1]]
    assert ids[0].tolist() == [[1, 0, 2, -1], [3, 2, 0, -1]]
    assert ids[0, 0].tolist() != ids[1, 0].tolist()
    # lambda = 0.5, topic 0: keys logprob - 0.5 logtp
    key = {w: _lp(w, 0) - 0.5 * _ltp(w) for w in (0, 1, 2)}
    assert ids[2, 0, :3].tolist() == sorted(key, key=lambda w: -key[w]) == [0, 2, 1]
    assert cnt[0].tolist() == [[1, 8, 3, 0], [4, 3, 2, 0]] and tot[0].tolist() == [[1, 10, 6, 0], [4, 6, 10, 0]]
    for l in range(3):
        for k in range(2):
            for i in range(3):
                w = int(ids[l, k, i])
                assert lp[l, k, i] == _lp(w, k) and ll[l, k, i] == _lp(w, k) - _ltp(w)
            assert lp[l, k, 3] == 0.0 and ll[l, k, 3] == 0.0
    assert N.check_key_gaps(NW, NWSUM, BETA, [0.0, 0.5, 1.0]) > 0.05
    # two words with one row: equal keys, the smaller id first, and no gap is asked of them
    twin = np.vstack([NW, NW[1]])
    ids2 = N.expected_relevant(twin, NWSUM + NW[1], BETA, 5, [0.0])[0]
    assert ids2[0, 0].tolist()[:2] == [1, 4]
    N.check_key_gaps(twin, NWSUM + NW[1], BETA, [0.0, 1.0])
    with pytest.raises(AssertionError, match="adjacent keys"):
        N.check_key_gaps(NW, NWSUM, BETA, [0.0], gap=10.0)


def test_the_restatement_scores_the_worked_examples_saliency():
    """p = (12/21, 9/21).  w1 and w3 live in one topic: log(1 / p_k).  w0:
    0.8 log(0.8 / p_0) + 0.2 log(0.2 / p_1).  w2 (half and half) is the least
    distinctive.  Saliency order: w3 (0.161), w0 (0.0556), w1 (0.0266), w2
    (0.0029)."""
    p0, p1 = 12 / 21, 9 / 21
    dist = [0.8 * math.log(0.8 / p0) + 0.2 * math.log(0.2 / p1), math.log(1 / p0),
            0.5 * math.log(0.5 / p0) + 0.5 * math.log(0.5 / p1), math.log(1 / p1)]
    ids, tot, sal, d = N.expected_salient(NW, NWSUM, 6)
    assert ids.tolist() == [3, 0, 1, 2, -1, -1] and tot.tolist() == [4, 10, 1, 6, 0, 0]
    for i, w in enumerate((3, 0, 1, 2)):
        assert d[i] == pytest.approx(dist[w], rel=1e-15) and sal[i] == pytest.approx(TW[w] / 21 * dist[w], rel=1e-15)
    assert sal[4:].tolist() == [0.0, 0.0] and d[4:].tolist() == [0.0, 0.0]
    assert sal[0] == pytest.approx(0.16139, rel=1e-4) and sal[3] == pytest.approx(0.002946, rel=1e-3)
    # a word without tokens is no candidate
    ids = N.expected_salient(np.vstack([NW, [0, 0]]), NWSUM, 6)[0]
    assert ids.tolist() == [3, 0, 1, 2, -1, -1]
    assert N.check_saliency_gaps(NW, NWSUM, 3) > 0.1


# ------------------------------------------------------------ the text
def test_relevant_words_text_from_given_arrays(libs):
    ids = np.array([[2, 1, -1], [0, -1, -1]], np.int32)
    cnt = np.array([[3, 1, 0], [7, 0, 0]], np.int32)
    tot = np.array([[5, 9, 0], [40, 0, 0]], np.int64)
    lp = np.array([[-1.5, -2.25, 0.0], [-0.7, 0.0, 0.0]])
    ll = np.array([[0.5, -0.125, 0.0], [0.3, 0.0, 0.0]])
    text = tm.format_relevant_words(ids, cnt, tot, lp, ll, 0.5, names=["n0", None, "two words"])
    r = -0.7 - (1.0 - 0.5) * (-0.7 - 0.3)
    assert text == ("#topic rank word count total relevance logprob loglift\n"
                    "0 0 two words 3 5 -0.5 -1.5 0.5\n"
                    "0 1 1 1 9 -1.1875 -2.25 -0.125\n"
                    f"1 0 n0 7 40 {tm.format_double(r)} -0.7 0.3\n")
    # lambda = 1: the relevance is the log probability; without names the ids
    assert tm.format_relevant_words(ids[:1, :1], cnt[:1, :1], tot[:1, :1], lp[:1, :1], ll[:1, :1], 1.0) == \
        "#topic rank word count total relevance logprob loglift\n0 0 2 3 5 -1.5 -1.5 0.5\n"
    empty = np.full((3, 2), -1, np.int32)
    zero = np.zeros((3, 2))
    assert tm.format_relevant_words(empty, zero, zero, zero, zero) == \
        "#topic rank word count total relevance logprob loglift\n"
    with pytest.raises(ValueError, match="one shape"):
        tm.format_relevant_words(ids, cnt[:, :2], tot, lp, ll)
    r3 = tm.TopicRelevance(np.array([0.5]), ids[None], cnt[None], tot[None], lp[None], ll[None]).relevance(0)
    assert r3[0, 0] == -0.5 and r3[0, 1] == -1.1875 and np.isnan(r3[0, 2]) and r3[1, 0] == r


# ------------------------------------------------------------- the MDS
@pytest.mark.parametrize("mds", [tm.classical_mds, N.classical_mds])
def test_classical_mds_on_three_points(mds):
    # three points on a line at 0, 1 and 3: the centred coordinates, the far point positive
    x, y = mds(np.array([[0, 1, 3], [1, 0, 2], [3, 2, 0.0]]))
    np.testing.assert_allclose(x, [-4 / 3, -1 / 3, 5 / 3], atol=1e-12)
    np.testing.assert_allclose(y, [0, 0, 0], atol=1e-7)
    # the same line mirrored: the sign rule turns it the same way round
    x, _ = mds(np.array([[0, 2, 3], [2, 0, 1], [3, 1, 0.0]]))
    np.testing.assert_allclose(x, [5 / 3, -1 / 3, -4 / 3], atol=1e-12)
    # a 3-4-5 triangle is reproduced exactly in two dimensions
    D = np.array([[0, 3, 4], [3, 0, 5], [4, 5, 0.0]])
    x, y = mds(D)
    np.testing.assert_allclose(N.pairwise(x, y), D, atol=1e-12)
    for a in (x, y):
        assert a[int(np.argmax(np.abs(a)))] > 0
    # K = 1: both axes 0; K = 2: the points on the x axis, the first positive (a tie: lowest index)
    x, y = mds(np.zeros((1, 1)))
    assert x.tolist() == [0.0] and y.tolist() == [0.0]
    x, y = mds(np.array([[0, 2.0], [2.0, 0]]))
    np.testing.assert_allclose(x, [1.0, -1.0], atol=1e-12)
    assert y.tolist() == [0.0, 0.0]


def test_the_two_mds_agree_and_the_slider_values():
    rng = np.random.default_rng(3)
    pts = rng.random((7, 4))
    D = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1))
    a, b = tm.classical_mds(D), N.classical_mds(D)
    np.testing.assert_allclose(a[0], b[0], atol=1e-12)
    np.testing.assert_allclose(a[1], b[1], atol=1e-12)
    assert tm.vis_lambdas(0.25).tolist() == [0.0, 0.25, 0.5, 0.75, 1.0] == N.vis_lambdas(0.25).tolist()
    lam = tm.vis_lambdas(0.01)
    assert lam.size == 101 and lam[0] == 0.0 and lam[-1] == 1.0 and np.all(np.diff(lam) > 0)
    assert np.array_equal(lam, N.vis_lambdas(0.01))
    assert tm.vis_lambdas(0.3).tolist() == [0.0, 0.3, 0.6, 0.8999999999999999, 1.0]
    assert tm.vis_lambdas(0.004).size == 251                       # more than one call's 128


def test_the_restatements_vis_dict_on_the_worked_example():
    """Topic 0 (12 tokens) is shown first.  R = 2, step 0.5: topic 0's lists
    are (w1, w0), (w0, w2), (w0, w2) under lambda 0, 0.5, 1: the union w1, w0,
    w2 in first-seen order."""
    js = np.array([[0.0, 0.2], [0.2, 0.0]])
    vis = N.expected_vis(NW, NWSUM, BETA, 2, 0.5, js, names=["a", "b", "c", "d"])
    assert vis["topic.order"] == [1, 2] and vis["R"] == 2 and vis["lambda.step"] == 0.5
    assert vis["mdsDat"]["Freq"] == [100 * 12 / 21, 100 * 9 / 21] and vis["mdsDat"]["topics"] == [1, 2]
    np.testing.assert_allclose(vis["mdsDat"]["x"], [0.1, -0.1], atol=1e-15)
    assert vis["mdsDat"]["y"] == [0.0, 0.0] and vis["mdsDat"]["cluster"] == [1, 1]
    t = vis["tinfo"]
    assert t["Term"] == ["d", "a", "b", "a", "c", "d", "c"]
    assert t["Category"] == ["Default"] * 2 + ["Topic1"] * 3 + ["Topic2"] * 2
    assert t["Freq"] == [4, 10, 1, 8, 3, 4, 3] and t["Total"] == [4, 10, 1, 10, 6, 4, 6]
    assert t["logprob"][:2] == [2.0, 1.0] and t["loglift"][:2] == [2.0, 1.0]
    assert t["logprob"][2] == _lp(1, 0) and t["loglift"][3] == _lp(0, 0) - _ltp(0)
    tt = vis["token.table"]
    assert tt["Term"] == ["a", "a", "b", "c", "c", "d"] and tt["Topic"] == [1, 2, 1, 1, 2, 2]
    assert tt["Freq"] == [0.8, 0.2, 1.0, 0.5, 0.5, 1.0]
    assert vis["plot.opts"] == {"xlab": "PC1", "ylab": "PC2"}
