"""CPU-side checks of the topic diagnostics (no device needed): the new calls
are declared, bound and exported; bad arguments fail with a status and a
message naming the argument before any device work; ldatm_diagnostics_finish
(host only) equals a numpy restatement of its eleven formulas on hand-built
integer statistics and refuses statistics that do not add up.  The GPU
behaviour is in test_diagnostics_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

SAMPLER_CALLS = ["lda_topic_codocuments", "lda_topic_word_stats"]
MODEL_CALLS = ["ldatm_topic_codocuments", "ldatm_topic_statistics", "ldatm_diagnostics_finish",
               "ldatm_topic_diagnostics"]
TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")
INVALID, INTERNAL = -1, -6


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
    assert set(SAMPLER_CALLS) <= _declared(capi.HEADER_PATH, "lda_")
    assert set(SAMPLER_CALLS) <= set(capi.SIGNATURES)
    assert set(SAMPLER_CALLS) <= _exported(capi.LIB_PATH, "lda_")
    assert set(MODEL_CALLS) <= _declared(TM_HEADER, "ldatm_")
    assert set(MODEL_CALLS) <= set(tm.TM_SIGNATURES)
    assert set(MODEL_CALLS) <= _exported(tm.TM_LIB_PATH, "ldatm_")


def test_caps_and_columns_match_the_headers_and_the_abi_stays_8(libs):
    L, _ = libs
    text = open(capi.HEADER_PATH).read()
    assert "#define LDA_DIAG_WORDS_MAX %d\n" % capi.DIAG_WORDS_MAX in text
    assert "#define LDA_DIAG_PROPS_MAX %d\n" % capi.DIAG_PROPS_MAX in text
    assert capi.DIAG_WORDS_MAX == 64 and capi.DIAG_PROPS_MAX == 8
    tmh = open(TM_HEADER).read()
    assert "#define LDATM_DIAG_COLUMNS %d\n" % len(tm.DIAG_COLUMNS) in tmh and len(tm.DIAG_COLUMNS) == 11
    assert "#define LDATM_DIAG_PROPS %d\n" % len(tm.DIAG_PROPS) in tmh
    for i, name in enumerate(tm.DIAG_COLUMNS):
        assert "#define LDATM_DIAG_%s %d\n" % (name.upper(), i) in tmh
    assert tm.DIAG_PROPS == (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
    assert L.lda_abi_version() == 8


def test_sampler_calls_reject_a_null_context(libs):
    L, _ = libs
    ids = np.zeros(8, np.int32)
    out = np.zeros(64, np.int64)
    p = out.ctypes.data
    assert L.lda_topic_codocuments(None, 1, ids.ctypes.data, 0, None, p, p) == INVALID
    assert b"null ctx" in L.lda_last_error()
    assert L.lda_topic_word_stats(None, 1, ids.ctypes.data, p, p, p, p) == INVALID
    assert b"null ctx" in L.lda_last_error()


def test_model_calls_name_the_bad_argument_before_any_device_work(libs, handle):
    """K = 4, V = 50, no documents, possibly no GPU: every check comes before
    the first use of a device, so each failure names its own argument."""
    _, T = libs
    K, V, n = 4, 50, 3
    good = np.array([[0, 1, 2], [3, -1, 4], [-1, -1, -1], [49, 0, 7]], np.int32)
    props = np.array(tm.DIAG_PROPS, np.float64)
    out = np.zeros(K * 65 * 33, np.int64)
    p, g, pr = out.ctypes.data, good.ctypes.data, props.ctypes.data

    def codoc(h=handle, n=n, ids=g, P=7, props=pr, o0=p, o1=p):
        return T.ldatm_topic_codocuments(h, n, ids, P, props, o0, o1)

    def failed(status, word):
        return status == INVALID and word in T.ldatm_last_error()

    assert failed(codoc(h=None), b"null model")
    for bad in (0, -1, 65):
        assert failed(codoc(n=bad), b"LDA_DIAG_WORDS_MAX")
    assert failed(codoc(ids=None), b"null word_ids")
    for bad in (-2, V):
        ids = good.copy()
        ids[3, 1] = bad
        assert failed(codoc(ids=ids.ctypes.data), b"outside [-1, V)")
    ids = good.copy()
    ids[3, 2] = 49                      # twice in topic 3's list
    assert failed(codoc(ids=ids.ctypes.data), b"twice")
    ids = good.copy()
    ids[0, 0] = 3                       # in topic 1's list too: allowed, so the next check speaks
    assert failed(codoc(ids=ids.ctypes.data, P=9), b"LDA_DIAG_PROPS_MAX")
    assert failed(codoc(P=-1), b"LDA_DIAG_PROPS_MAX")
    assert failed(codoc(props=None), b"null props")
    for bad in ([0.1, 0.05], [0.1, 0.1], [0.0, 0.5], [0.5, 1.5], [float("nan")]):
        b = np.array(bad, np.float64)
        assert failed(codoc(P=len(b), props=b.ctypes.data), b"props must be strictly ascending")
    assert failed(codoc(o0=None), b"null output")
    assert failed(codoc(o1=None), b"null output")

    def stats(h=handle, n=n, a=(p,) * 7):
        return T.ldatm_topic_statistics(h, n, *a)

    assert failed(stats(h=None), b"null model")
    for bad in (0, 65):
        assert failed(stats(n=bad), b"LDA_DIAG_WORDS_MAX")
    assert failed(stats(a=(None,) + (p,) * 6), b"null word_ids")
    for i in range(1, 7):
        assert failed(stats(a=(p,) * i + (None,) + (p,) * (6 - i)), b"null output")

    assert failed(T.ldatm_topic_diagnostics(None, n, p, p), b"null model")
    for bad in (0, 65):
        assert failed(T.ldatm_topic_diagnostics(handle, bad, p, p), b"LDA_DIAG_WORDS_MAX")
    assert failed(T.ldatm_topic_diagnostics(handle, n, None, p), b"null output")


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    for call in (g.topic_codocuments, g.topic_word_stats):
        with pytest.raises(ValueError, match="word_ids must be"):
            call(np.zeros((3, 2), np.int32))
        with pytest.raises(ValueError, match="n must be in"):
            call(np.zeros((4, 65), np.int32))
        with pytest.raises(ValueError, match="n must be in"):
            call(np.zeros((4, 0), np.int32))
    with pytest.raises(ValueError, match="at most 8 props"):
        g.topic_codocuments(np.zeros((4, 2), np.int32), props=np.linspace(0.1, 0.9, 9))
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        for bad in (0, 65):
            with pytest.raises(ValueError, match="numTopWords must be in"):
                m.getDiagnostics(bad)
            with pytest.raises(ValueError, match="numTopWords must be in"):
                m.topicStatistics(bad)
        with pytest.raises(ValueError, match="word_ids must be"):
            m.topicCodocuments(np.zeros((5, 2), np.int32))
    finally:
        m._L = real
        m.close()


def test_python_faces_fail_loudly_without_a_gpu(libs):
    import torch
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    try:
        il = tm.InstanceList(tm.Alphabet(range(3)))
        il.add(tm.Instance([0, 1]))
        il.add(tm.Instance([2]))
        m.addInstances(il)
        ids = np.array([[0], [1], [2], [-1]], np.int32)
        calls = (lambda: m.getDiagnostics(2), lambda: m.topicStatistics(2), lambda: m.topicCodocuments(ids))
        if not torch.cuda.is_available():
            for call in calls:
                with pytest.raises(capi.LdaError):
                    call()
        else:
            d = m.getDiagnostics(2)
            assert d.tokens.sum() == 3 and len(d.as_rows()) == 4
    finally:
        m.close()


# ---- ldatm_diagnostics_finish against a numpy restatement -----------------
K, N_WORDS, V, BETA, MAX_LEN = 5, 4, 50, 0.01, 12


def _hand_built():
    """Integer statistics of five topics: 0 ordinary, with a listed word of
    count 0; 1 empty (T = 0); 2 with two words of four; 3 living in one
    document, with an empty slot in the middle of its list; 4 spread so thin
    that no document reaches 0.02."""
    s = {}
    s["nwsum"] = np.array([40, 0, 25, 10, 30], np.int32)
    H = np.zeros((K, MAX_LEN + 1), np.int64)
    H[0, [1, 2, 4, 12]] = [6, 5, 3, 1]
    H[2, [1, 2, 3]] = [5, 4, 4]
    H[3, 10] = 1
    H[4, 1] = 30
    s["hist"] = H
    s["ids"] = np.array([[5, 8, 20, 31], [-1, -1, -1, -1], [7, 9, -1, -1], [3, -1, 11, 4], [1, 2, 6, 5]], np.int32)
    s["counts"] = np.array([[15, 9, 0, 4], [0] * 4, [12, 5, 0, 0], [6, 0, 3, 1], [4, 3, 3, 2]], np.int32)
    s["totals"] = np.array([[20, 9, 3, 30], [0] * 4, [12, 40, 0, 0], [8, 0, 3, 17], [4, 5, 3, 22]], np.int64)
    s["shares"] = np.array([[0.37, 0.251, 0.0123, 0.9], [0.0] * 4, [0.48, 1.7, 0.0, 0.0], [0.6, 0.0, 0.301, 2.2],
                            [0.13, 0.11, 0.1, 0.77]], np.float64)
    s["sumsq"] = np.array([400, 0, 181, 46, 60], np.uint64)
    tri = np.zeros((K, N_WORDS * (N_WORDS + 1) // 2), np.int64)
    #          (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) (3,0) (3,1) (3,2) (3,3)
    tri[0] = [9, 4, 6, 0, 0, 0, 2, 0, 0, 4]
    tri[2] = [8, 3, 5, 0, 0, 0, 0, 0, 0, 0]
    tri[3] = [1, 0, 0, 1, 0, 1, 1, 0, 1, 1]
    tri[4] = [4, 0, 3, 1, 0, 3, 0, 0, 0, 2]
    s["codoc"] = tri
    s["stats"] = np.array([[15, 4, 15, 14, 11, 8, 5, 3, 1], [0] * 9, [13, 2, 13, 13, 9, 6, 4, 2, 2],
                           [1, 1, 1, 1, 1, 1, 1, 1, 1], [30, 0, 12, 0, 0, 0, 0, 0, 0]], np.int64)
    return s


def _finish(s):
    return tm.diagnostics_finish(V, BETA, s["nwsum"], s["hist"], s["ids"], s["counts"], s["totals"], s["shares"],
                                 s["sumsq"], s["codoc"], s["stats"])


def restate(V, beta, nwsum, hist, ids, counts, totals, shares, sumsq, codoc, stats):
    """The eleven columns as the header states them, in plain Python floats."""
    K, n = ids.shape
    out = np.zeros((K, 11))
    N = float(sum(int(t) for t in nwsum))
    ratio = lambda a, b: 0.0 if b == 0 else float(a) / float(b)   # noqa: E731
    xlog = lambda x, arg: 0.0 if x == 0 else x * math.log(arg)   # noqa: E731
    for k in range(K):
        T = float(nwsum[k])
        if T == 0:
            continue
        Dk = int(stats[k, 0])
        slots = [i for i in range(n) if ids[k, i] >= 0]
        cell = lambda i, j: float(codoc[k, i * (i + 1) // 2 + j])   # noqa: E731
        c = [float(counts[k, i]) for i in slots]
        out[k, 0] = T
        out[k, 1] = math.log(T) - sum(float(hist[k, x]) * (x * math.log(x)) for x in range(1, hist.shape[1])) / T
        out[k, 2] = sum(math.log((cell(slots[a], slots[b]) + beta) / (cell(slots[b], slots[b]) + beta))
                        for a in range(1, len(slots)) for b in range(a))
        out[k, 3] = sum(xlog(x / T, x / T * V) for x in c)
        out[k, 4] = sum(xlog(x / T, (x / T) / (float(totals[k, i]) / N)) for x, i in zip(c, slots))
        out[k, 5] = ratio(T * T, int(sumsq[k]))
        d = [cell(i, i) for i in slots]
        js = 0.0
        for x, y in zip(c, d):
            p, q = ratio(x, sum(c)), ratio(y, sum(d))
            mu = (p + q) / 2
            js += 0.5 * xlog(p, p / mu if p else 1.0) + 0.5 * xlog(q, q / mu if q else 1.0)
        out[k, 6] = js
        out[k, 7] = ratio(stats[k, 1], Dk)
        out[k, 8] = ratio(stats[k, 2 + 6], stats[k, 2 + 1])
        out[k, 9] = ratio(stats[k, 2 + 5], Dk)
        out[k, 10] = sum(((beta + x) / (V * beta + T)) / shares[k, i] for x, i in zip(c, slots)) / len(slots) \
            if slots else 0.0
    return out


def test_finish_equals_the_numpy_restatement(libs):
    """rtol = atol = 1e-12: each column is a sum of at most a few thousand fp64
    terms, each good to a few ulps of 2.2e-16; the coherence terms share a sign;
    the entropy is a difference that cancels, hence the atol."""
    s = _hand_built()
    got = _finish(s)
    want = restate(V, BETA, s["nwsum"], s["hist"], s["ids"], s["counts"], s["totals"], s["shares"], s["sumsq"],
                   s["codoc"], s["stats"])
    assert got.shape == (K, 11) and np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    col = {name: got[:, i] for i, name in enumerate(tm.DIAG_COLUMNS)}
    assert (got[1] == 0).all()                                # the empty topic: every column 0
    assert abs(col["document_entropy"][3]) <= 1e-12          # one document: entropy 0
    assert col["rank_1_docs"][3] == 1.0 and col["allocation_ratio"][3] == 1.0
    assert col["allocation_ratio"][4] == 0.0 and col["rank_1_docs"][4] == 0.0   # nothing at 0.02: 0, not inf
    assert col["coherence"][2] == math.log((3 + BETA) / (8 + BETA))             # two words: one term
    assert (col["coherence"] <= 0).all() and col["tokens"].tolist() == [40, 0, 25, 10, 30]
    # hand figures: the entropy of topic 4 (thirty documents of one token) is log 30
    assert abs(col["document_entropy"][4] - math.log(30)) < 1e-12
    assert abs(col["eff_num_words"][0] - 4.0) < 1e-12         # 40^2 / 400


def test_finish_refuses_statistics_that_do_not_add_up(libs):
    _, T = libs
    s = _hand_built()
    s["stats"][0, 0] += 1               # D_0 no longer the sum of H[0]
    with pytest.raises(capi.LdaError) as e:
        _finish(s)
    assert e.value.status == INTERNAL and "histogram" in str(e.value)
    s = _hand_built()
    s["hist"][3, 2] = 1                 # also for a topic in one document
    with pytest.raises(capi.LdaError) as e:
        _finish(s)
    assert e.value.status == INTERNAL


def test_finish_rejects_bad_arguments(libs):
    _, T = libs
    s = _hand_built()
    a = [s["nwsum"], s["hist"], s["ids"], s["counts"], s["totals"], s["shares"], s["sumsq"], s["codoc"], s["stats"]]
    out = np.zeros((K, 11))
    p = [x.ctypes.data for x in a]

    def call(n=N_WORDS, ptrs=p, o=out.ctypes.data):
        return T.ldatm_diagnostics_finish(K, V, n, BETA, ptrs[0], MAX_LEN, *ptrs[1:], o)

    assert call() == 0
    for bad in (0, 65):
        assert call(n=bad) == INVALID and b"LDA_DIAG_WORDS_MAX" in T.ldatm_last_error()
    names = [b"nwsum", b"topic_doc_counts", b"word_ids"] + [b"statistics"] * 6
    for i, name in enumerate(names):
        q = list(p)
        q[i] = None
        assert call(ptrs=q) == INVALID and b"null " + name in T.ldatm_last_error()
    assert call(o=None) == INVALID and b"null output" in T.ldatm_last_error()
