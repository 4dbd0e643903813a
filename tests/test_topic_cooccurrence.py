"""CPU-side checks of the topic co-occurrence readout (no device needed):
lda_topic_cooccurrence, its hook and the ldatm_ calls are declared, bound and
exported and the ABI stays 8; bad arguments fail with a status and a message
naming the argument before any device work; the numpy restatement every GPU
expectation comes from (topic_cooccurrence_numpy) is checked against an example
worked by hand; topic_correlation_finish (the C call through its Python twin)
is checked against direct numpy formulas on those integers at rtol 1e-12, the
project's fp64 bar, and its non-finite cases by kind; the partner selection and
the text are checked from given arrays.  The GPU behaviour is in
test_topic_cooccurrence_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

import topic_cooccurrence_numpy as N

SAMPLER_CALLS = ["lda_topic_cooccurrence", "lda_debug_topic_cooccurrence_global"]
MODEL_CALLS = ["ldatm_topic_cooccurrence", "ldatm_topic_correlation_finish", "ldatm_topic_correlations",
               "ldatm_topic_partners", "ldatm_topic_partners_select", "ldatm_topic_correlations_text",
               "ldatm_print_topic_correlations", "ldatm_topic_correlations_format"]
TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")
RTOL = 1e-12


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
    assert "#define LDA_TOPIC_COOC_LDS_TOPICS %d\n" % capi.TOPIC_COOC_LDS_TOPICS in text
    assert "#define LDA_ABI_VERSION 8" in text and L.lda_abi_version() == 8
    tm_text = open(TM_HEADER).read()
    for name, v in tm.CORR_MEASURES.items():
        assert "#define LDATM_CORR_%s %d\n" % (name.upper(), v) in tm_text
    for name, v in tm.COOC_TABLES.items():
        assert "#define LDATM_COOC_%s %d\n" % (name.upper(), v) in tm_text
    assert set(tm.MEASURE_TABLE) == set(tm.CORR_MEASURES) and set(tm.MEASURE_TABLE.values()) == set(tm.COOC_TABLES)
    assert capi.TOPIC_COOC_STATS == N.STATS == tuple(tm.COOC_TABLES)


def test_sampler_call_rejects_a_null_context_and_the_hook_needs_none(libs):
    L, _ = libs
    out = np.zeros(16, np.int64)
    p = out.ctypes.data
    assert L.lda_topic_cooccurrence(None, 10, 2, 0.05, p, p, p, None, None, None) == -1
    assert b"null ctx" in L.lda_last_error()
    L.lda_debug_topic_cooccurrence_global(1)
    L.lda_debug_topic_cooccurrence_global(0)


BAD_PROPS = (-1e-9, 1.0 + 1e-9, 2.0, math.nan, math.inf, -math.inf)


def test_model_calls_reject_bad_arguments_before_any_device_work(libs, handle):
    """A model without documents and without a GPU: the argument checks come
    first, so each call names its own argument, not the missing device."""
    _, T = libs
    a = np.zeros(16, np.int64)
    f = np.zeros(16, np.float64)
    ids = np.zeros(16, np.int32)
    p, fp, ip = a.ctypes.data, f.ctypes.data, ids.ctypes.data
    err = T.ldatm_last_error
    used = C.c_int64()
    u = C.byref(used)
    cooc = T.ldatm_topic_cooccurrence
    assert cooc(None, 10, 2, 0.05, u, p, p, p, p, p) == -1 and b"null" in err()
    for args in ((None, p, p), (u, None, p), (u, p, None)):
        assert cooc(handle, 10, 2, 0.05, *args, p, None, None) == -1 and b"null output" in err()
    for mt in (0, -3):
        assert cooc(handle, mt, 2, 0.05, u, p, p, p, p, p) == -1 and b"min_tokens" in err()
    for mc in (0, -1):
        assert cooc(handle, 10, mc, 0.05, u, p, p, p, p, p) == -1 and b"min_count" in err()
    for mp in BAD_PROPS:
        assert cooc(handle, 10, 2, mp, u, p, p, p, p, p) == -1 and b"min_prop" in err()
    # the matrix, the partners and the text check the measure and the same thresholds
    corr, part = T.ldatm_topic_correlations, T.ldatm_topic_partners
    assert corr(None, 1, 10, 2, 0.05, fp) == -1 and b"null" in err()
    assert part(None, 1, 10, 2, 0.05, 3, ip, fp) == -1 and b"null" in err()
    for m in (-1, 6, 99):
        assert corr(handle, m, 10, 2, 0.05, fp) == -1 and b"measure" in err()
        assert part(handle, m, 10, 2, 0.05, 3, ip, fp) == -1 and b"measure" in err()
    assert corr(handle, 1, 0, 2, 0.05, fp) == -1 and b"min_tokens" in err()
    assert corr(handle, 1, 10, 0, 0.05, fp) == -1 and b"min_count" in err()
    assert part(handle, 1, 0, 2, 0.05, 3, ip, fp) == -1 and b"min_tokens" in err()
    assert part(handle, 1, 10, 0, 0.05, 3, ip, fp) == -1 and b"min_count" in err()
    for mp in BAD_PROPS:
        assert corr(handle, 1, 10, 2, mp, fp) == -1 and b"min_prop" in err()
        assert part(handle, 1, 10, 2, mp, 3, ip, fp) == -1 and b"min_prop" in err()
    assert corr(handle, 1, 10, 2, 0.05, None) == -1 and b"null output" in err()
    for n in (0, -2):
        assert part(handle, 1, 10, 2, 0.05, n, ip, fp) == -1 and b"n must be" in err()
    for args in ((None, fp), (ip, None)):
        assert part(handle, 1, 10, 2, 0.05, 3, *args) == -1 and b"null output" in err()
    size = C.c_size_t()
    text, prnt = T.ldatm_topic_correlations_text, T.ldatm_print_topic_correlations
    assert text(None, 1, 3, 10, 2, 0.05, None, 0, C.byref(size)) == -1
    assert text(handle, 7, 3, 10, 2, 0.05, None, 0, C.byref(size)) == -1 and b"measure" in err()
    assert text(handle, 1, 0, 10, 2, 0.05, None, 0, C.byref(size)) == -1 and b"n must be" in err()
    assert prnt(handle, b"/nonexistent/x", 1, 3, 0, 2, 0.05) == -1 and b"min_tokens" in err()
    assert prnt(handle, b"/nonexistent/x", 1, 3, 10, 0, 0.05) == -1 and b"min_count" in err()
    assert prnt(handle, b"/nonexistent/x", 1, 3, 10, 2, math.nan) == -1 and b"min_prop" in err()
    assert prnt(None, b"/nonexistent/x", 1, 3, 10, 2, 0.05) == -1
    assert not a.any() and not f.any() and not ids.any()          # nothing was written


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    assert callable(GibbsSampler.topic_cooccurrence)
    for name in ("topicCooccurrence", "topicCorrelations", "topicPartners", "getTopicPartners", "topicGraph",
                 "printTopicCorrelations", "topicCorrelationsText"):
        assert callable(getattr(tm.ParallelTopicModel, name))
    assert capi.topic_cooc_stats("overlap") == ("overlap",)
    assert capi.topic_cooc_stats(["product", "codocs"]) == ("codocs", "product") and capi.topic_cooc_stats(()) == ()
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    with pytest.raises(ValueError, match="unknown statistic"):
        g.topic_cooccurrence(stats=("codocs", "npmi"))
    with pytest.raises(ValueError, match="min_tokens"):
        g.topic_cooccurrence(min_tokens=0)
    with pytest.raises(ValueError, match="min_count"):
        g.topic_cooccurrence(min_count=0)
    for bad in BAD_PROPS:
        with pytest.raises(ValueError, match="min_prop"):
            g.topic_cooccurrence(min_prop=bad)
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        with pytest.raises(ValueError, match="unknown statistic"):
            m.topicCooccurrence(stats=("tokens",))
        with pytest.raises(ValueError, match="min_prop"):
            m.topicCooccurrence(minProp=math.nan)
        for call in (m.topicCorrelations, m.topicGraph):
            with pytest.raises(ValueError, match="unknown measure"):
                call("spearman")
            with pytest.raises(ValueError, match="min_tokens"):
                call("npmi", minTokens=0)
        for call in (m.topicPartners, m.getTopicPartners, m.topicCorrelationsText):
            with pytest.raises(ValueError, match="n must be"):
                call(0)
            with pytest.raises(ValueError, match="unknown measure"):
                call(3, "kendall")
            with pytest.raises(ValueError, match="min_count"):
                call(3, "npmi", minCount=0)
        with pytest.raises(ValueError, match="n must be"):
            m.printTopicCorrelations("/nonexistent/x", 0)
        with pytest.raises(ValueError, match="unknown measure"):
            m.printTopicCorrelations("/nonexistent/x", 3, "kendall")
    finally:
        m._L = real
        m.close()


# ------------------------------------------------- the restatement, by hand
# K = 4, min_tokens 4, min_count 2, min_prop 0.25:
#   d0 [0 0 1 1 1 2]           L 6,  n (2 3 1 0), 0.25 L = 1.5: 0 and 1 present, 2 under min_count
#   d1 []                      empty
#   d2 [0 0 0]                 L 3: under min_tokens, counts nowhere
#   d3 [3 3 0 0 0 0 0 0]       L 8,  n (6 0 0 2), 0.25 L = 2.0: topic 3 exactly at min_count and at min_prop L
#   d4 [1 1 1 2 x 9]           L 12, n (0 3 9 0), 0.25 L = 3.0: topic 1 exactly at min_prop L
#   d5 [0 0 1 x 10]            L 12, n (2 10 0 0): topic 0 at min_count but under 3.0: absent
DOC_OFF = np.array([0, 6, 6, 9, 17, 29, 41], np.int64)
Z = np.array([0, 0, 1, 1, 1, 2] + [0, 0, 0] + [3, 3, 0, 0, 0, 0, 0, 0] + [1, 1, 1] + [2] * 9 + [0, 0] + [1] * 10,
             np.int32)
USED = 4
TOKENS = [10, 16, 10, 2]
PRESENT = [2, 3, 1, 1]
CODOCS = [[2, 1, 0, 1], [1, 3, 1, 0], [0, 1, 1, 0], [1, 0, 0, 1]]
OVERLAP = [[10, 4, 1, 2], [4, 16, 4, 0], [1, 4, 10, 0], [2, 0, 0, 2]]
PRODUCT = [[44, 26, 2, 12], [26, 118, 30, 0], [2, 30, 82, 0], [12, 0, 0, 4]]
ND_USED = np.array([[2, 3, 1, 0], [6, 0, 0, 2], [0, 3, 9, 0], [2, 10, 0, 0]], np.float64)


def test_restatement_against_the_hand_worked_example():
    assert len(Z) == DOC_OFF[-1]
    e = N.expected_cooccurrence(Z, DOC_OFF, 4, min_tokens=4, min_count=2, min_prop=0.25)
    assert e["docs_used"] == USED
    assert e["tokens"].tolist() == TOKENS and e["present"].tolist() == PRESENT
    assert e["codocs"].tolist() == CODOCS and e["overlap"].tolist() == OVERLAP and e["product"].tolist() == PRODUCT
    for s in N.STATS:
        assert e[s].dtype == np.int64 and np.array_equal(e[s], e[s].T)
    assert np.diag(e["codocs"]).tolist() == PRESENT and np.diag(e["overlap"]).tolist() == TOKENS
    nd = N.doc_topic_counts(Z, DOC_OFF, 4)
    assert nd[[0, 3, 4, 5]].tolist() == ND_USED.astype(np.int64).tolist() and not nd[1].any()
    # only the requested tables exist, and the others do not change
    one = N.expected_cooccurrence(Z, DOC_OFF, 4, 4, 2, 0.25, stats=("overlap",))
    assert set(one) == {"docs_used", "tokens", "present", "overlap"} and one["overlap"].tolist() == OVERLAP


def test_restatement_thresholds_move_presence_only():
    # a hair above 0.25 drops the two topics that sat exactly on min_prop L
    e = N.expected_cooccurrence(Z, DOC_OFF, 4, 4, 2, np.nextafter(0.25, 1.0))
    assert e["present"].tolist() == [2, 2, 1, 0] and e["codocs"][0, 3] == 0 and e["codocs"][1, 2] == 0
    assert e["overlap"].tolist() == OVERLAP and e["product"].tolist() == PRODUCT and e["tokens"].tolist() == TOKENS
    # min_count 3 drops the counts of 2; min_tokens 1 takes d2 in
    e = N.expected_cooccurrence(Z, DOC_OFF, 4, 4, 3, 0.0)
    assert e["present"].tolist() == [1, 3, 1, 0]
    e = N.expected_cooccurrence(Z, DOC_OFF, 4, 1, 1, 0.0)
    assert e["docs_used"] == 5 and e["tokens"].tolist() == [13, 16, 10, 2] and e["present"].tolist() == [4, 3, 2, 1]
    assert e["product"][0, 0] == 44 + 9
    e = N.expected_cooccurrence(Z, DOC_OFF, 4, 13, 1, 0.0)
    assert e["docs_used"] == 0 and not any(e[s].any() for s in N.STATS + ("tokens", "present"))


# ------------------------------------------------------------- the measures
def _ints():
    return (USED, np.array(TOKENS, np.int64), np.array(PRESENT, np.int64),
            {"codocs": np.array(CODOCS, np.int64), "overlap": np.array(OVERLAP, np.int64),
             "product": np.array(PRODUCT, np.int64)})


def test_finish_against_direct_numpy_formulas(libs):
    D, tok, pre, tabs = _ints()
    Cm, M, S = (tabs[s].astype(np.float64) for s in N.STATS)
    c, n = pre.astype(np.float64), tok.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pmi = np.log(D * Cm / np.outer(c, c))
        npmi = np.where(Cm == 0, -1.0, pmi / -np.log(Cm / D))
        direct = {
            "pmi": pmi,
            "npmi": npmi,
            "jaccard": Cm / (c[:, None] + c[None, :] - Cm),
            "overlap": M / (n[:, None] + n[None, :] - M),
            "cosine": (ND_USED / np.linalg.norm(ND_USED, axis=0)).T @ (ND_USED / np.linalg.norm(ND_USED, axis=0)),
            "pearson": np.corrcoef(ND_USED, rowvar=False),
        }
    for measure, want in direct.items():
        got = tm.topic_correlation_finish(measure, D, tok, pre, tabs[tm.MEASURE_TABLE[measure]])
        assert got.shape == (4, 4) and got.dtype == np.float64
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), measure
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=0, err_msg=measure)
        assert np.array_equal(got[~fin], want[~fin]), measure          # pmi's -inf where C_kl = 0
        # the Python restatement cell by cell gives the same bits
        assert N.same_floats(got, N.finish(measure, D, tok, pre, tabs[tm.MEASURE_TABLE[measure]])), measure
        assert np.array_equal(got, got.T, equal_nan=True)
    got = tm.topic_correlation_finish("pmi", D, tok, pre, tabs["codocs"])
    assert got[0, 2] == -math.inf and got[0, 1] == math.log(4 * 1 / (2 * 3))
    got = tm.topic_correlation_finish("npmi", D, tok, pre, tabs["codocs"])
    assert got[0, 2] == -1.0 and got[1, 3] == -1.0
    got = tm.topic_correlation_finish("pearson", D, tok, pre, tabs["product"])
    assert np.all(np.diag(got) == 1.0)
    assert np.all(np.diag(tm.topic_correlation_finish("jaccard", D, tok, pre, tabs["codocs"])) == 1.0)


def test_finish_non_finite_cases_by_kind(libs):
    """Topic 1 is never present and has no tokens; topics 0 and 2 are present
    in every used document; topic 3's count is the same in every document."""
    D = 3
    tok = np.array([9, 0, 6, 6], np.int64)
    pre = np.array([3, 0, 3, 1], np.int64)
    cod = np.array([[3, 0, 3, 1], [0, 0, 0, 0], [3, 0, 3, 1], [1, 0, 1, 1]], np.int64)
    ovl = np.array([[9, 0, 5, 5], [0, 0, 0, 0], [5, 0, 6, 4], [5, 0, 4, 6]], np.int64)
    nd = np.array([[4, 0, 1, 2], [3, 0, 2, 2], [2, 0, 3, 2]], np.int64)
    prd = nd.T @ nd
    assert prd[3, 3] * D == tok[3] ** 2                       # no variance in topic 3
    pmi = tm.topic_correlation_finish("pmi", D, tok, pre, cod)
    npmi = tm.topic_correlation_finish("npmi", D, tok, pre, cod)
    for mat in (pmi, npmi):
        assert np.all(np.isnan(mat[1, :])) and np.all(np.isnan(mat[:, 1]))
        assert np.isfinite(np.delete(np.delete(mat, 1, 0), 1, 1)).all()
    assert npmi[0, 2] == 1.0 and npmi[0, 0] == 1.0 and npmi[2, 0] == 1.0      # C_kl = D'
    assert pmi[0, 2] == 0.0 and pmi[0, 3] == math.log(3 * 1 / (3 * 1))
    assert npmi[3, 3] == 1.0                                                   # pmi / -log(C_kk / D') at C_kk < D'
    jac = tm.topic_correlation_finish("jaccard", D, tok, pre, cod)
    assert math.isnan(jac[1, 1]) and jac[0, 1] == 0.0 and jac[0, 3] == 1 / 3
    ov = tm.topic_correlation_finish("overlap", D, tok, pre, ovl)
    assert math.isnan(ov[1, 1]) and ov[0, 1] == 0.0 and ov[0, 2] == 5 / 10
    cos = tm.topic_correlation_finish("cosine", D, tok, pre, prd)
    assert np.all(np.isnan(cos[1, :])) and np.all(np.isnan(cos[:, 1])) and np.isfinite(cos[0, 3])
    pea = tm.topic_correlation_finish("pearson", D, tok, pre, prd)
    for k in (1, 3):
        assert np.all(np.isnan(pea[k, :])) and np.all(np.isnan(pea[:, k]))
    assert pea[0, 2] == -1.0 and pea[0, 0] == 1.0
    for measure, tab in (("pmi", cod), ("npmi", cod), ("jaccard", cod), ("overlap", ovl), ("cosine", prd),
                         ("pearson", prd)):
        assert N.same_floats(tm.topic_correlation_finish(measure, D, tok, pre, tab),
                             N.finish(measure, D, tok, pre, tab)), measure
    # no used document at all: everything is NaN
    z4, z44 = np.zeros(4, np.int64), np.zeros((4, 4), np.int64)
    for measure in tm.CORR_MEASURES:
        assert np.all(np.isnan(tm.topic_correlation_finish(measure, 0, z4, z4, z44)))


def test_finish_pearson_has_no_cancellation_error(libs):
    """Counts near 2^20 in about 10^6 documents with a spread of 2: D' S_kl and
    N_k N_l are near 2^80 and differ by 2^40, past what a double holds; the
    terms are formed in 128-bit integers, so the correlations are exactly +-1."""
    D = 2 * 499979
    base = (1 << 20) + 7
    # topic 0: D/2 documents at base, D/2 at base + 2; topic 1 the reverse; topic 2 = topic 0
    half = D // 2
    n0 = half * base + half * (base + 2)
    s00 = half * base * base + half * (base + 2) ** 2
    s01 = D * base * (base + 2)
    assert s00 < 2 ** 63
    tok = np.array([n0, n0, n0], np.int64)
    prd = np.array([[s00, s01, s00], [s01, s00, s01], [s00, s01, s00]], np.int64)
    pea = tm.topic_correlation_finish("pearson", D, tok, np.zeros(3, np.int64), prd)
    assert pea.tolist() == [[1.0, -1.0, 1.0], [-1.0, 1.0, -1.0], [1.0, -1.0, 1.0]]
    # what doubles alone would have lost: neither product is a double
    assert int(float(D) * float(s01)) != D * s01 and int(float(n0) * float(n0)) != n0 * n0


def test_finish_rejects_a_wrong_table_and_an_unknown_measure(libs):
    _, T = libs
    D, tok, pre, tabs = _ints()
    out = np.zeros((4, 4))
    t, p, o = tok.ctypes.data, pre.ctypes.data, out.ctypes.data
    call = T.ldatm_topic_correlation_finish
    for name, m in tm.CORR_MEASURES.items():
        for kind, kv in tm.COOC_TABLES.items():
            st = call(m, 4, D, t, p, kv, tabs[kind].ctypes.data, o)
            if kind == tm.MEASURE_TABLE[name]:
                assert st == 0
            else:
                assert st == -1 and b"wrong table for the measure" in T.ldatm_last_error()
                with pytest.raises(capi.LdaError, match="wrong table"):
                    tm.topic_correlation_finish(name, D, tok, pre, tabs[kind], kind=kind)
    for m in (-1, 6):
        assert call(m, 4, D, t, p, 0, tabs["codocs"].ctypes.data, o) == -1 and b"measure" in T.ldatm_last_error()
    assert call(1, 0, D, t, p, 0, tabs["codocs"].ctypes.data, o) == -1 and b"K must" in T.ldatm_last_error()
    assert call(1, 4, -1, t, p, 0, tabs["codocs"].ctypes.data, o) == -1 and b"docs_used" in T.ldatm_last_error()
    assert call(1, 4, D, None, p, 0, tabs["codocs"].ctypes.data, o) == -1 and b"null input" in T.ldatm_last_error()
    assert call(1, 4, D, t, p, 0, None, o) == -1 and b"null input" in T.ldatm_last_error()
    assert call(1, 4, D, t, p, 0, tabs["codocs"].ctypes.data, None) == -1 and b"null output" in T.ldatm_last_error()
    with pytest.raises(ValueError, match="unknown measure"):
        tm.topic_correlation_finish("spearman", D, tok, pre, tabs["codocs"])
    with pytest.raises(ValueError, match="unknown table"):
        tm.topic_correlation_finish("npmi", D, tok, pre, tabs["codocs"], kind="cooc")
    with pytest.raises(ValueError, match=r"\[K, K\]"):
        tm.topic_correlation_finish("npmi", D, tok, pre, tabs["codocs"][:3])


# ------------------------------------------------------------- the partners
def test_partners_tie_order_non_finite_values_and_padding(libs):
    nan, inf = math.nan, math.inf
    mat = np.array([[9.0, 0.5, 0.5, nan, 0.5],
                    [0.5, 9.0, -inf, 0.25, inf],
                    [-1.0, -1.0, 9.0, -1.0, 0.0],
                    [nan, nan, nan, nan, nan],
                    [0.1, 0.3, 0.2, 0.3, 9.0]])
    ids, values = tm.topic_partners_select(mat, 3)
    assert ids.dtype == np.int32 and values.dtype == np.float64
    # equal values by smaller id; the diagonal, NaN and the infinities are left out
    assert ids.tolist() == [[1, 2, 4], [0, 3, -1], [4, 0, 1], [-1, -1, -1], [1, 3, 2]]
    assert N.same_floats(values, [[0.5, 0.5, 0.5], [0.5, 0.25, nan], [0.0, -1.0, -1.0], [nan] * 3, [0.3, 0.3, 0.2]])
    # n > K - 1: every row ends in -1 / NaN
    ids, values = tm.topic_partners_select(mat, 7)
    assert ids.shape == (5, 7) and np.all(ids[:, 4:] == -1) and np.all(np.isnan(values[:, 4:]))
    assert ids[2].tolist() == [4, 0, 1, 3, -1, -1, -1] and ids[0, :4].tolist() == [1, 2, 4, -1]
    for n in (1, 3, 4, 7):
        got, want = tm.topic_partners_select(mat, n), N.partners(mat, n)
        assert np.array_equal(got[0], want[0]) and N.same_floats(got[1], want[1])
    # a single topic has no partner
    ids, values = tm.topic_partners_select(np.ones((1, 1)), 2)
    assert ids.tolist() == [[-1, -1]] and np.all(np.isnan(values))
    with pytest.raises(ValueError, match="n must be"):
        tm.topic_partners_select(mat, 0)
    with pytest.raises(ValueError, match=r"\[K, K\]"):
        tm.topic_partners_select(mat[:, :3], 2)
    _, T = libs
    out_i, out_v = np.zeros(10, np.int32), np.zeros(10)
    assert T.ldatm_topic_partners_select(5, 2, None, out_i.ctypes.data, out_v.ctypes.data) == -1
    assert b"null matrix" in T.ldatm_last_error()
    assert T.ldatm_topic_partners_select(5, 0, mat.ctypes.data, out_i.ctypes.data, out_v.ctypes.data) == -1
    assert b"n must be" in T.ldatm_last_error()
    assert T.ldatm_topic_partners_select(5, 2, mat.ctypes.data, None, out_v.ctypes.data) == -1
    assert b"null output" in T.ldatm_last_error()


# ------------------------------------------------------------------ the text
def test_topic_correlations_text_from_given_arrays(libs):
    ids = np.array([[2, 1, -1], [0, -1, -1], [-1, -1, -1]], np.int32)
    values = np.array([[0.75, -0.125, math.nan], [1e-5, math.nan, math.nan], [math.nan] * 3])
    text = tm.format_topic_correlations(ids, values)
    assert text == ("#topic partner value\n"
                    "0 2 0.75\n"
                    "0 1 -0.125\n"
                    f"1 0 {tm.format_double(1e-5)}\n")
    assert tm.format_double(1e-5) == "1.0E-5"
    third = np.array([[1], [0]], np.int32), np.array([[1 / 3], [-1.0]])
    assert tm.format_topic_correlations(*third) == \
        f"#topic partner value\n0 1 {tm.format_double(1 / 3)}\n1 0 -1.0\n"
    assert float(tm.format_double(1 / 3)) == 1 / 3
    assert tm.format_topic_correlations(np.full((3, 2), -1, np.int32), np.full((3, 2), math.nan)) == \
        "#topic partner value\n"
    with pytest.raises(ValueError, match="one shape"):
        tm.format_topic_correlations(ids, values[:, :2])
    # from the hand-worked integers to the text in one go
    D, tok, pre, tabs = _ints()
    mat = tm.topic_correlation_finish("jaccard", D, tok, pre, tabs["codocs"])
    pi, pv = tm.topic_partners_select(mat, 2)
    assert pi.tolist() == [[3, 1], [2, 0], [1, 0], [0, 1]]
    assert tm.format_topic_correlations(pi, pv).splitlines()[1:3] == \
        ["0 3 0.5", f"0 1 {tm.format_double(1 / 4)}"]
