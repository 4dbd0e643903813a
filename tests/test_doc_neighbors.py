"""CPU-side checks of the nearest-document calls (no device needed):
lda_doc_distances / lda_doc_nearest / lda_doc_neighbors, their test hook and
their ldatm_ mirrors are declared, bound and exported; bad arguments fail with
a status and a message of their own before any device work; the text helper
formats given arrays; the Python faces check their arguments before any native
call; and the numpy restatement that checks the device
(tests/doc_neighbors_numpy.py) is itself checked on a three-document example
worked by hand.  The GPU behaviour is in test_doc_neighbors_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import doc_neighbors_numpy as DN
from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

SAMPLER_CALLS = ["lda_doc_distances", "lda_doc_nearest", "lda_doc_neighbors", "lda_debug_doc_nearest_chunk"]
MODEL_CALLS = ["ldatm_document_distances", "ldatm_nearest_documents", "ldatm_document_neighbors",
               "ldatm_document_neighbors_text", "ldatm_print_document_neighbors", "ldatm_document_neighbors_format"]
TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")
INVALID = -1


@pytest.fixture(scope="module")
def libs():
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(tm.TM_LIB_PATH)):
        from ldagibbssampling_amd.build import build_library
        build_library()
    return capi.load(), tm.load_tm()


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


def test_defines_match_the_header_and_the_abi_stays_8(libs):
    L, _ = libs
    text = open(capi.HEADER_PATH).read()
    assert "#define LDA_DOC_NEAREST_MAX %d\n" % capi.DOC_NEAREST_MAX in text
    assert capi.DOC_NEAREST_MAX == 64
    assert capi.DOC_METRICS == {"cosine": 0, "hellinger": 1, "jensen_shannon": 2} == DN.METRICS
    for name, value in capi.DOC_METRICS.items():
        assert capi.TOPIC_METRICS[name] == value      # the LDA_TOPIC_* numbers
    assert "#define LDA_ABI_VERSION 8\n" in text
    assert L.lda_abi_version() == 8


def test_sampler_calls_reject_a_null_context(libs):
    L, _ = libs
    out = np.zeros(8, np.float64)
    ids = np.zeros(8, np.int64)
    theta = np.full(4, 0.25)
    po, pi, pt = out.ctypes.data, ids.ctypes.data, theta.ctypes.data
    assert L.lda_doc_distances(None, 0, 1, pt, None, 0, 1, None, po) == INVALID
    assert b"null ctx" in L.lda_last_error()
    assert L.lda_doc_nearest(None, 1, 2, 1, pt, None, None, 1, pi, po) == INVALID
    assert b"null ctx" in L.lda_last_error()
    assert L.lda_doc_neighbors(None, 2, 2, 0, 1, None, 1, pi, po) == INVALID
    assert b"null ctx" in L.lda_last_error()
    # the null context is named before any other bad argument
    assert L.lda_doc_nearest(None, 9, 0, -1, None, None, None, 0, None, None) == INVALID
    assert b"null ctx" in L.lda_last_error()
    L.lda_debug_doc_nearest_chunk(64, 64)
    L.lda_debug_doc_nearest_chunk(0, 0)


def test_model_calls_reject_bad_arguments_before_any_device_work(libs):
    """A model without documents and without a GPU: the argument checks come
    first, in the header's order, so each call names its own argument."""
    _, T = libs
    h = C.c_void_p()
    K = 4
    assert T.ldatm_create(C.byref(h), K, 1.0, 0.01) == 0
    try:
        out = np.zeros(64, np.float64)
        ids = np.zeros(64, np.int64)
        theta = np.full((2, K), 0.25)
        counts = np.ones((2, K), np.int32)
        po, pi, pt, pc = out.ctypes.data, ids.ctypes.data, theta.ctypes.data, counts.ctypes.data
        doc0 = np.zeros(1, np.int64)
        pd = doc0.ctypes.data

        def failed(status, word):
            return status == INVALID and word in T.ldatm_last_error()

        dist = lambda *a: T.ldatm_document_distances(*a)
        near = lambda *a: T.ldatm_nearest_documents(*a)
        nbrs = lambda *a: T.ldatm_document_neighbors(*a)
        assert failed(dist(None, 0, 1, pt, None, 0, None, po), b"null")
        assert failed(near(None, 0, 1, 1, pt, None, None, 1, pi, po), b"null")
        assert failed(nbrs(None, 0, 1, 0, None, 1, pi, po), b"null")
        assert failed(T.ldatm_document_neighbors_text(None, 1, 0, 1, None, 0, None), b"null")
        assert failed(T.ldatm_print_document_neighbors(None, b"/nonexistent/x", 1, 0, 1), b"null")
        for metric in (-1, 3, 99):
            assert failed(dist(h, metric, 1, pt, None, 0, None, po), b"metric")
            assert failed(near(h, metric, 1, 1, pt, None, None, 1, pi, po), b"metric")
            assert failed(nbrs(h, metric, 1, 0, None, 1, pi, po), b"metric")
            assert failed(T.ldatm_document_neighbors_text(h, 1, metric, 1, None, 0, None), b"metric")
        for n in (0, -1, capi.DOC_NEAREST_MAX + 1):
            assert failed(near(h, 1, n, 1, pt, None, None, 1, pi, po), b"LDA_DOC_NEAREST_MAX")
            assert failed(nbrs(h, 1, n, 0, None, 1, pi, po), b"LDA_DOC_NEAREST_MAX")
            assert failed(T.ldatm_document_neighbors_text(h, n, 1, 1, None, 0, None), b"LDA_DOC_NEAREST_MAX")
        for a, b in ((pt, pc), (None, None)):
            assert failed(dist(h, 1, 1, a, b, 0, None, po), b"theta / counts")
            assert failed(near(h, 1, 1, 1, a, b, None, 1, pi, po), b"theta / counts")
        assert failed(dist(h, 1, 1, pt, None, 1, pd, None), b"null output")
        assert failed(near(h, 1, 1, 1, pt, None, None, 1, None, po), b"null output")
        assert failed(near(h, 1, 1, 1, None, pc, None, 1, pi, None), b"null output")
        assert failed(nbrs(h, 1, 1, 1, pd, 1, None, po), b"null output")
        assert failed(dist(h, 1, -1, pt, None, 0, None, po), b"bad sizes")
        assert failed(dist(h, 1, 1, pt, None, -1, None, po), b"bad sizes")
        assert failed(near(h, 1, 1, -1, pt, None, None, 1, pi, po), b"bad sizes")
        assert failed(nbrs(h, 1, 1, -1, None, 1, pi, po), b"bad sizes")
        # no documents: every id is outside [0, D), and M must be D without a list
        assert failed(dist(h, 1, 1, pt, None, 1, pd, po), b"document id")
        assert failed(dist(h, 1, 1, pt, None, 3, None, po), b"number of documents")
        assert failed(nbrs(h, 1, 1, 1, pd, 1, pi, po), b"document id")
        assert failed(nbrs(h, 1, 1, 3, None, 1, pi, po), b"number of documents")
        for bad in (0, -5):
            assert failed(near(h, 1, 1, 1, pt, None, None, bad, pi, po), b"min_tokens")
            assert failed(nbrs(h, 1, 1, 0, None, bad, pi, po), b"min_tokens")
            assert failed(T.ldatm_document_neighbors_text(h, 1, 1, bad, None, 0, None), b"min_tokens")
        for bad in (0, 5, -2):
            skip = np.array([-1, bad], np.int64)
            assert failed(near(h, 1, 1, 2, pt, None, skip.ctypes.data, 1, pi, po), b"skip")
        for bad in (-0.25, np.nan, np.inf):
            t = theta.copy()
            t[1, 2] = bad
            assert failed(dist(h, 1, 2, t.ctypes.data, None, 0, None, po), b"theta holds")
            assert failed(near(h, 1, 1, 2, t.ctypes.data, None, None, 1, pi, po), b"theta holds")
        t = theta.copy()
        t[1] = 0.0
        assert failed(near(h, 1, 1, 2, t.ctypes.data, None, None, 1, pi, po), b"theta row sums to zero")
        c = counts.copy()
        c[1, 3] = -1
        assert failed(dist(h, 1, 2, None, c.ctypes.data, 0, None, po), b"counts holds a negative")
        assert failed(near(h, 1, 1, 2, None, c.ctypes.data, None, 1, pi, po), b"counts holds a negative")
        # the order: metric before n before the query forms before the output
        assert failed(near(h, 7, 0, 1, None, None, None, 0, None, None), b"metric")
        assert failed(near(h, 1, 0, 1, None, None, None, 0, None, None), b"LDA_DOC_NEAREST_MAX")
        assert failed(near(h, 1, 1, 1, None, None, None, 0, None, None), b"theta / counts")
        assert failed(near(h, 1, 1, 1, pt, None, None, 0, None, None), b"null output")
        # nothing to do: success, nothing touched
        assert dist(h, 1, 0, pt, None, 0, None, None) == 0
        assert near(h, 1, 1, 0, pt, None, None, 1, None, None) == 0
        assert nbrs(h, 1, 1, 0, None, 1, None, None) == 0
    finally:
        T.ldatm_destroy(h)


def test_the_format_helper_writes_the_text_from_arrays(libs):
    ids = np.array([[1, 2], [0, -1], [-1, -1]], np.int64)
    vals = np.array([[0.0, 0.5], [1e-5, np.nan], [np.nan, np.nan]])
    text = tm.format_document_neighbors(ids, vals, docs=[5, 7, 9], names=["a", "b", None])
    assert text == ("#doc neighbor name value\n"
                    "5 1 b 0.0\n"
                    "5 2 null-source 0.5\n"
                    "7 0 a 1.0E-5\n")
    # without docs the query of row j is j; without names every name is null-source
    assert tm.format_document_neighbors(ids[:1], vals[:1]) == ("#doc neighbor name value\n"
                                                               "0 1 null-source 0.0\n"
                                                               "0 2 null-source 0.5\n")
    assert tm.format_document_neighbors(np.zeros((0, 3), np.int64), np.zeros((0, 3))) == "#doc neighbor name value\n"
    with pytest.raises(ValueError):
        tm.format_document_neighbors(ids, vals[:2])
    with pytest.raises(ValueError):
        tm.format_document_neighbors(ids, vals, docs=[1])
    _, T = libs
    size = C.c_size_t()
    assert T.ldatm_document_neighbors_format(1, 0, None, ids.ctypes.data, vals.ctypes.data, None, 0, None, 0,
                                             C.byref(size)) == INVALID
    assert T.ldatm_document_neighbors_format(1, 2, None, None, vals.ctypes.data, None, 0, None, 0,
                                             C.byref(size)) == INVALID


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    for name in ("doc_distances", "nearest_docs", "doc_neighbors"):
        assert callable(getattr(GibbsSampler, name))
    for name in ("documentDistances", "nearestDocuments", "documentNeighbors", "getDocumentNeighbors",
                 "documentNeighborsText", "printDocumentNeighbors"):
        assert callable(getattr(tm.ParallelTopicModel, name))
    assert callable(tm.TopicInferencer.nearestInstances)

    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.V, g.D, g._h, g._L = 4, 3, 3, None, _NoNative()
    theta = np.full((2, 4), 0.25)
    counts = np.ones((2, 4), np.int32)
    for bad in ("euclid", "kullback_leibler", "", 3, -1, 2.0, True):
        with pytest.raises(ValueError, match="metric must be"):
            g.doc_distances(bad, theta=theta)
        with pytest.raises(ValueError, match="metric must be"):
            g.nearest_docs(3, bad, theta=theta)
        with pytest.raises(ValueError, match="metric must be"):
            g.doc_neighbors(3, bad)
    for bad in (0, -1, capi.DOC_NEAREST_MAX + 1):
        with pytest.raises(ValueError, match="n must be in"):
            g.nearest_docs(bad, theta=theta)
        with pytest.raises(ValueError, match="n must be in"):
            g.doc_neighbors(bad)
    for kw in ({}, {"theta": theta, "counts": counts}):
        with pytest.raises(ValueError, match="exactly one of theta and counts"):
            g.doc_distances("cosine", **kw)
        with pytest.raises(ValueError, match="exactly one of theta and counts"):
            g.nearest_docs(2, **kw)
    with pytest.raises(ValueError, match="theta must have shape"):
        g.doc_distances("cosine", theta=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="counts must have shape"):
        g.nearest_docs(2, counts=np.zeros((2, 5), np.int32))
    with pytest.raises(ValueError, match="counts must be"):
        g.nearest_docs(2, counts=np.full((2, 4), 0.5))
    with pytest.raises(ValueError, match="counts must be"):
        g.nearest_docs(2, counts=np.full((2, 4), -1))
    with pytest.raises(ValueError, match="skip must hold"):
        g.nearest_docs(2, theta=theta, skip=[0])
    # valid arguments reach the native call
    with pytest.raises(AssertionError, match="native call lda_doc_distances"):
        g.doc_distances("hellinger", counts=counts)
    with pytest.raises(AssertionError, match="native call lda_doc_nearest"):
        g.nearest_docs(2, theta=theta, skip=[0, -1])
    with pytest.raises(AssertionError, match="native call lda_doc_neighbors"):
        g.doc_neighbors(2, "jensen_shannon", docs=[2, 0])

    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    il = tm.InstanceList(tm.Alphabet(["a", "b", "c"]))
    il.add(tm.Instance([0, 1]))
    m.addInstances(il)
    real = m._L
    try:
        m._L = _NoNative()
        for bad in ("manhattan", 9, "kullback_leibler"):
            with pytest.raises(ValueError, match="metric must be"):
                m.documentDistances(theta=theta, metric=bad)
            with pytest.raises(ValueError, match="metric must be"):
                m.nearestDocuments(theta, 2, metric=bad)
            with pytest.raises(ValueError, match="metric must be"):
                m.documentNeighbors(2, metric=bad)
            with pytest.raises(ValueError, match="metric must be"):
                m.printDocumentNeighbors("unused", 2, bad)
            with pytest.raises(ValueError, match="metric must be"):
                m.getInferencer().nearestInstances([tm.Instance([0])], 2, bad)
        for bad in (0, capi.DOC_NEAREST_MAX + 1):
            with pytest.raises(ValueError, match="n must be in"):
                m.nearestDocuments(theta, bad)
            with pytest.raises(ValueError, match="n must be in"):
                m.documentNeighbors(bad)
            with pytest.raises(ValueError, match="n must be in"):
                m.getDocumentNeighbors(0, bad)
            with pytest.raises(ValueError, match="n must be in"):
                m.documentNeighborsText(bad)
            with pytest.raises(ValueError, match="n must be in"):
                m.getInferencer().nearestInstances([tm.Instance([0])], bad)
        with pytest.raises(ValueError, match="exactly one of theta and counts"):
            m.documentDistances()
        with pytest.raises(ValueError, match="exactly one of theta and counts"):
            m.documentDistances(theta=theta, counts=counts)
        with pytest.raises(ValueError, match="exactly one of theta and counts"):
            m.nearestDocuments(None, 2)
        with pytest.raises(ValueError, match="exactly one of theta and counts"):
            m.nearestDocuments(theta, 2, counts=counts)
    finally:
        m._L = real
        m.close()


# ------------------------------------------------------- the restatement itself
def test_restatement_on_a_hand_worked_example():
    """Three documents, K = 3, alpha = (0.5, 0.5, 1): A = 2.  Documents 0 and 1
    hold the counts (2, 1, 1), document 2 holds (0, 0, 4); every length is 4,
    so every denominator is 6: p_0 = p_1 = (2.5, 1.5, 2) / 6, p_2 = (0.5, 0.5,
    5) / 6."""
    alpha = np.array([0.5, 0.5, 1.0])
    nd = np.array([[2, 1, 1], [2, 1, 1], [0, 0, 4]], np.int32)
    p = [2.5 / 6, 1.5 / 6, 2.0 / 6]
    q = [0.5 / 6, 0.5 / 6, 5.0 / 6]
    rows = DN.rows_from_counts(nd, alpha)
    np.testing.assert_allclose(rows, np.array([p, p, q]), rtol=0, atol=1e-16)
    dot = lambda a, b: sum(x * y for x, y in zip(a, b))
    want = {
        "cosine": dot(p, q) / math.sqrt(dot(p, p) * dot(q, q)),
        "hellinger": math.sqrt(sum((math.sqrt(x) - math.sqrt(y)) ** 2 for x, y in zip(p, q)) / 2),
        "jensen_shannon": 0.5 * (sum(x * math.log(x) for x in p) + sum(y * math.log(y) for y in q)
                                 - sum((x + y) * math.log((x + y) / 2) for x, y in zip(p, q))),
    }
    # by hand: p.q = 12 / 36, |p|^2 = 12.5 / 36, |q|^2 = 25.5 / 36
    assert abs(want["cosine"] - 12 / math.sqrt(12.5 * 25.5)) < 1e-15
    for name, same in (("cosine", 1.0), ("hellinger", 0.0), ("jensen_shannon", 0.0)):
        d = DN.distances(rows, rows, name)
        assert d.shape == (3, 3)
        np.testing.assert_allclose(d[0, 2], want[name], rtol=0, atol=1e-15)
        np.testing.assert_array_equal(d[0], d[1])                   # identical rows, identical values
        np.testing.assert_allclose(d, d.T, rtol=0, atol=1e-15)
        assert abs(d[0, 1] - same) < 1e-15 and abs(d[2, 2] - same) < 1e-15
        assert not np.signbit(d).any()
        np.testing.assert_array_equal(DN.distances(rows, rows, DN.METRICS[name]), d)
    h2 = DN.distances(rows, rows, "hellinger", squared_hellinger=True)
    np.testing.assert_allclose(h2, DN.distances(rows, rows, "hellinger") ** 2, rtol=0, atol=1e-15)
    # a theta query with a zero entry: x ln x = 0 at 0
    js = DN.distances([[0.0, 0.5, 0.5]], rows[:1], "jensen_shannon")[0, 0]
    t = [0.0, 0.5, 0.5]
    by_hand = 0.5 * (sum(x * math.log(x) for x in p) + 2 * 0.5 * math.log(0.5)
                     - sum((x + y) * math.log((x + y) / 2) for x, y in zip(p, t)))
    assert abs(js - by_hand) < 1e-15

    # the selection: value in the metric's order, ties by ascending id
    d = DN.distances(rows, rows, "hellinger")
    ids, vals = DN.nearest(d, 2, "hellinger", skip=[0, 1, 2])
    assert ids.tolist() == [[1, 2], [0, 2], [0, 1]]                 # document 2 is as far from 0 as from 1
    assert vals[0, 0] == d[0, 1] and vals[2].tolist() == [d[2, 0], d[2, 1]]
    ids, vals = DN.nearest(d, 4, "hellinger", skip=[0, 1, 2])
    assert ids[:, 2:].tolist() == [[-1, -1]] * 3 and np.isnan(vals[:, 2:]).all()
    c = DN.distances(rows, rows, "cosine")
    ids, _ = DN.nearest(c, 3, "cosine")
    assert ids.tolist() == [[0, 1, 2], [0, 1, 2], [2, 0, 1]]        # larger is nearer
    ids, _ = DN.nearest(c, 3, "cosine", lengths=[4, 2, 4], min_tokens=3, skip=[-1, -1, 2])
    assert ids.tolist() == [[0, 2, -1], [0, 2, -1], [0, -1, -1]]
    ids, vals = DN.nearest(c[:, [2, 0]], 1, "cosine", ids=[7, 3])
    assert ids.tolist() == [[3], [3], [7]] and vals[2, 0] == c[2, 2]
