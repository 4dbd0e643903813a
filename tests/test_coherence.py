"""CPU-side checks of reference-corpus coherence (no device needed): the new
calls are declared, bound and exported; ldatm_coherence_finish (host only)
equals the brute-force restatement (tests/coherence_numpy.py) on random integer
triangles and gives the hand-computed values of the worked example; bad
arguments fail with a status and a message naming the argument before any
device work.  The GPU behaviour is in test_coherence_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import coherence_numpy as N
from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

SAMPLER_CALLS = ["lda_word_cooccurrences", "lda_debug_cooc_chunk_tokens"]
MODEL_CALLS = ["ldatm_word_cooccurrences", "ldatm_coherence_finish", "ldatm_topic_coherence"]
TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")
INVALID = -1

# the worked example: five documents (one empty, one with tokens outside the
# alphabet) and two lists, the second with an empty slot
EX_DOCS = [[0, 1, 2, 1], [2, 3], [], [-1, 0, -1, -1, 1], [1, 3, 0]]
EX_IDS = np.array([[0, 1, 2], [1, 3, -1]], np.int32)
#            window: (units, topic 0, topic 1); cells (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
EX_WANT = {0: (4, [3, 3, 3, 1, 1, 2], [3, 1, 2, 0, 0, 0]),
           2: (10, [4, 1, 5, 0, 2, 3], [5, 1, 3, 0, 0, 0]),
           # windows of one token: the diagonals are the term frequencies (word 0 three times,
           # word 1 four times, word 2 twice, word 3 twice) and no two words share a unit
           1: (14, [3, 0, 4, 0, 0, 2], [4, 0, 2, 0, 0, 0]),
           # at least the longest document: the documents themselves
           5: (4, [3, 3, 3, 1, 1, 2], [3, 1, 2, 0, 0, 0])}


def example_corpus():
    off = np.zeros(len(EX_DOCS) + 1, np.int64)
    np.cumsum([len(d) for d in EX_DOCS], out=off[1:])
    return off, np.array([w for d in EX_DOCS for w in d], np.int32)


@pytest.fixture(scope="module")
def libs():
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(tm.TM_LIB_PATH)):
        from ldagibbssampling_amd.build import build_library
        build_library()
    return capi.load(), tm.load_tm()


@pytest.fixture()
def handle(libs):
    """A model of K = 4 topics over an alphabet of V = 50 with no documents."""
    _, T = libs
    h = C.c_void_p()
    assert T.ldatm_create(C.byref(h), 4, 1.0, 0.01) == 0
    assert T.ldatm_set_alphabet(h, 50, None) == 0
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
    assert "#define LDA_COOC_WINDOW_MAX %d\n" % capi.COOC_WINDOW_MAX in open(capi.HEADER_PATH).read()
    assert capi.COOC_WINDOW_MAX == 256
    tmh = open(TM_HEADER).read()
    for name, value in tm.COHERENCE_MEASURES.items():
        macro = {"u_mass": "UMASS", "c_uci": "UCI", "c_npmi": "NPMI"}[name]
        assert "#define LDATM_COHERENCE_%s %d\n" % (macro, value) in tmh
    assert callable(tm.coherence_finish) and L.lda_abi_version() == 8


# ---- the restatement on the worked example -------------------------------
def test_the_restatement_counts_the_worked_example():
    off, words = example_corpus()
    for window, (units, t0, t1) in EX_WANT.items():
        cooc, u = N.cooccurrences(EX_IDS, off, words, window)
        assert u == units and cooc.tolist() == [t0, t1], window


def test_finish_gives_the_worked_examples_hand_values(libs):
    """Window 0: N = 4.  Topic 0 (D = 3, 3, 2; cells (1,0) = 3, (2,0) = (2,1) =
    1) keeps three pairs, topic 1 (D = 3, 2; cell 1; an empty slot) one."""
    units, t0, t1 = EX_WANT[0]
    cooc = np.array([t0, t1], np.int64)
    log = math.log
    sums, pairs = tm.coherence_finish("u_mass", cooc, units)
    assert pairs.tolist() == [3, 1]
    want0 = 0.0
    for x in (log((3 + 1.0) / 3), log((1 + 1.0) / 3), log((1 + 1.0) / 3)):
        want0 += x
    assert abs(sums[0] - want0) <= 4 * 2.0 ** -52 and abs(sums[1] - log((1 + 1.0) / 3)) <= 2.0 ** -52
    e = 1e-12
    uci = [log((3 / 4 + e) / ((3 / 4) * (3 / 4))), log((1 / 4 + e) / ((2 / 4) * (3 / 4))),
           log((1 / 4 + e) / ((2 / 4) * (3 / 4)))]
    sums, pairs = tm.coherence_finish("c_uci", cooc, units)
    assert pairs.tolist() == [3, 1]
    assert abs(sums[0] - (uci[0] + uci[1] + uci[2])) <= 4 * 2.0 ** -52
    assert abs(sums[1] - log((1 / 4 + e) / ((2 / 4) * (3 / 4)))) <= 2.0 ** -52
    npmi = [uci[0] / -log(3 / 4 + e), uci[1] / -log(1 / 4 + e), uci[2] / -log(1 / 4 + e)]
    sums, pairs = tm.coherence_finish("c_npmi", cooc, units)
    assert abs(sums[0] - (npmi[0] + npmi[1] + npmi[2])) <= 8 * 2.0 ** -52
    # words 0 and 1 share three of four documents with three each: positive; 2 with either: negative
    assert npmi[0] > 0 > npmi[1]
    # an explicit epsilon replaces the default; the integer measure is taken too
    s2, _ = tm.coherence_finish(tm.COHERENCE_MEASURES["u_mass"], cooc, units, epsilon=0.5)
    assert abs(s2[1] - log((1 + 0.5) / 3)) <= 2.0 ** -52


# ---- ldatm_coherence_finish against the restatement ----------------------
def _random_triangles(rng, K, n, units):
    """Consistent triangles: D(i, j) <= min(D(i), D(j)) <= N, with words of
    D = 0, pairs of D(i, j) = N and D(i, j) = 0, and empty slots."""
    tri = np.zeros((K, n * (n + 1) // 2), np.int64)
    for k in range(K):
        D = rng.integers(0, units + 1, n)
        D[rng.random(n) < 0.15] = 0           # a word in no unit, or an empty slot
        D[rng.random(n) < 0.15] = units       # a word in every unit
        for i in range(n):
            tri[k, i * (i + 1) // 2 + i] = D[i]
            for j in range(i):
                hi = min(D[i], D[j])
                lo = max(0, D[i] + D[j] - units)
                tri[k, i * (i + 1) // 2 + j] = rng.integers(lo, hi + 1)
    return tri


@pytest.mark.parametrize("n,units", [(1, 7), (2, 1), (10, 40), (64, 1000), (20, 0), (12, 2 ** 40)])
def test_finish_equals_the_restatement(libs, n, units):
    """Tolerance, derived: both sides evaluate the same IEEE expression, so a
    term differs by at most one ulp of each of its logarithms (2^-52 of the
    term, two logarithms for NPMI) and the ordered sum of p terms by at most
    4 p 2^-53 sum |term| (p roundings of a partial sum bounded by sum |term|,
    with a factor of 4 to spare)."""
    rng = np.random.default_rng(n * 7919 + units % 1000)
    K = 6
    tri = _random_triangles(rng, K, n, units) if units else rng.integers(0, 5, (K, n * (n + 1) // 2))
    if units:
        i, j = np.tril_indices(n)
        assert n == 1 or units == 1 or ((tri[:, i == j] == 0).any() and (tri[:, i != j] == units).any())
    for measure in N.MEASURES:
        for eps in (None, 0.00137):       # never D(i, j) / N + eps == 1 for these N
            sums, pairs = tm.coherence_finish(measure, tri, units, epsilon=eps)
            ws, wp, mags = N.finish(measure, tri, units, eps)
            np.testing.assert_array_equal(pairs, wp)
            logs = 2 if measure == "c_npmi" else 1
            tol = 4 * wp * 2.0 ** -53 * mags + logs * 2.0 ** -52 * mags
            assert np.all(np.abs(sums - ws) <= tol), (measure, np.abs(sums - ws).max(), tol)
            assert np.isfinite(sums).all()
            if n == 1 or units == 0:
                assert not pairs.any() and not sums.any()


def test_finish_rejects_bad_arguments(libs):
    _, T = libs
    tri = np.zeros((3, 6), np.int64)
    sums, pairs = np.zeros(3), np.zeros(3, np.int64)

    def call(K=3, n=3, measure=0, c=tri.ctypes.data, units=5, s=sums.ctypes.data, p=pairs.ctypes.data):
        return T.ldatm_coherence_finish(K, n, measure, -1.0, c, units, s, p)

    assert call() == 0
    assert call(K=0) == INVALID and b"bad sizes" in T.ldatm_last_error()
    assert call(units=-1) == INVALID and b"bad sizes" in T.ldatm_last_error()
    for bad in (0, 65):
        assert call(n=bad) == INVALID and b"LDA_DIAG_WORDS_MAX" in T.ldatm_last_error()
    for bad in (-1, 3):
        assert call(measure=bad) == INVALID and b"measure" in T.ldatm_last_error()
    assert call(c=None) == INVALID and b"null cooc" in T.ldatm_last_error()
    assert call(s=None) == INVALID and b"null output" in T.ldatm_last_error()
    assert call(p=None) == INVALID and b"null output" in T.ldatm_last_error()
    with pytest.raises(ValueError, match="measure must be"):
        tm.coherence_finish("c_v", tri, 5)
    with pytest.raises(ValueError, match="cooc must be"):
        tm.coherence_finish("u_mass", np.zeros((3, 5), np.int64), 5)


# ---- errors before any device work ---------------------------------------
def test_sampler_call_rejects_a_null_context(libs):
    L, _ = libs
    ids = np.zeros(8, np.int32)
    out = np.zeros(64, np.int64)
    p = out.ctypes.data
    assert L.lda_word_cooccurrences(None, 1, ids.ctypes.data, 0, 0, None, None, p, p) == INVALID
    assert b"null ctx" in L.lda_last_error()
    L.lda_debug_cooc_chunk_tokens(0)        # the hook takes a call without a context


def test_model_calls_name_the_bad_argument_before_any_device_work(libs, handle):
    """K = 4, V = 50, no documents, possibly no GPU: every check comes before
    the first use of a device, so each failure names its own argument."""
    _, T = libs
    K, V, n = 4, 50, 3
    good = np.array([[0, 1, 2], [3, -1, 4], [-1, -1, -1], [49, 0, 7]], np.int32)
    out = np.zeros(K * 65 * 33, np.int64)
    off = np.array([0, 2, 2, 5], np.int64)
    words = np.array([0, -1, 49, 3, 3], np.int32)
    p, g = out.ctypes.data, good.ctypes.data

    def failed(status, word):
        return status == INVALID and word in T.ldatm_last_error()

    def cooc(h=handle, n=n, ids=g, window=0, Dh=3, off=off.ctypes.data, w=words.ctypes.data, o0=p, o1=p):
        return T.ldatm_word_cooccurrences(h, n, ids, window, Dh, off, w, o0, o1)

    assert failed(cooc(h=None), b"null model")
    for bad in (0, -1, 65):
        assert failed(cooc(n=bad), b"LDA_DIAG_WORDS_MAX")
    assert failed(cooc(ids=None), b"null word_ids")
    for bad in (-2, V):
        ids = good.copy()
        ids[3, 1] = bad
        assert failed(cooc(ids=ids.ctypes.data), b"outside [-1, V)")
    ids = good.copy()
    ids[3, 2] = 49                      # twice in topic 3's list
    assert failed(cooc(ids=ids.ctypes.data), b"twice")
    ids = good.copy()
    ids[0, 0] = 3                       # in topic 1's list too: allowed, so the next check speaks
    assert failed(cooc(ids=ids.ctypes.data, window=-1), b"LDA_COOC_WINDOW_MAX")
    assert failed(cooc(window=257), b"LDA_COOC_WINDOW_MAX")
    assert failed(cooc(o0=None), b"null output")
    assert failed(cooc(o1=None), b"null output")
    assert failed(cooc(Dh=-1), b"bad sizes")
    bad_off = np.array([0, 3, 2, 5], np.int64)
    assert failed(cooc(off=bad_off.ctypes.data), b"doc_off not monotone")
    assert failed(cooc(w=None), b"words is null")
    for bad in (-2, V):
        w = words.copy()
        w[4] = bad
        assert failed(cooc(w=w.ctypes.data), b"out of range [-1, V)")

    vals = np.zeros(K)

    def coh(h=handle, measure=2, n=n, window=10, Dh=3, off=off.ctypes.data, w=words.ctypes.data,
            v=vals.ctypes.data, pr=p, u=p):
        return T.ldatm_topic_coherence(h, measure, n, window, -1.0, Dh, off, w, v, pr, None, None, u)

    assert failed(coh(h=None), b"null model")
    for bad in (-1, 3):
        assert failed(coh(measure=bad), b"measure must be")
    for bad in (0, 65):
        assert failed(coh(n=bad), b"LDA_DIAG_WORDS_MAX")
    for bad in (-1, 257):
        assert failed(coh(window=bad), b"LDA_COOC_WINDOW_MAX")
    assert failed(coh(Dh=-1), b"bad sizes")
    assert failed(coh(off=bad_off.ctypes.data), b"doc_off not monotone")
    assert failed(coh(w=None), b"words is null")
    w = words.copy()
    w[0] = V
    assert failed(coh(w=w.ctypes.data), b"out of range [-1, V)")
    assert failed(coh(v=None), b"null output")
    assert failed(coh(pr=None), b"null output")
    assert failed(coh(u=None), b"null output")


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    with pytest.raises(ValueError, match="word_ids must be"):
        g.word_cooccurrences(np.zeros((3, 2), np.int32))
    for bad in (0, 65):
        with pytest.raises(ValueError, match="n must be in"):
            g.word_cooccurrences(np.zeros((4, bad), np.int32))
    for bad in (-1, 257):
        with pytest.raises(ValueError, match="window must be in"):
            g.word_cooccurrences(np.zeros((4, 2), np.int32), window=bad)
    with pytest.raises(ValueError, match="words is shorter"):
        g.word_cooccurrences(np.zeros((4, 2), np.int32), doc_off=[0, 3], words=[1])
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        with pytest.raises(ValueError, match="measure must be one of"):
            m.getCoherence("c_v")
        for bad in (0, 65):
            with pytest.raises(ValueError, match="numTopWords must be in"):
                m.getCoherence("c_npmi", bad)
        for bad in (-1, 257):
            with pytest.raises(ValueError, match="window must be in"):
                m.getCoherence("c_npmi", window=bad)
            with pytest.raises(ValueError, match="window must be in"):
                m.wordCooccurrences(np.zeros((4, 2), np.int32), window=bad)
        with pytest.raises(ValueError, match="epsilon must be"):
            m.getCoherence("u_mass", epsilon=-0.5)
        with pytest.raises(ValueError, match="reference must be"):
            m.getCoherence("u_mass", reference=[[0, 1]])
        with pytest.raises(ValueError, match="word_ids must be"):
            m.wordCooccurrences(np.zeros((5, 2), np.int32))
    finally:
        m._L = real
        m.close()
