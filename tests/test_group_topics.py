"""CPU-side checks of the topics-by-group readout (no device needed):
lda_group_topics, lda_subcorpus_*, the helpers and the ldatm_ calls are
declared, bound and exported and the ABI stays 8; bad arguments fail with a
status and a message naming the argument before any device work; the numpy
restatement every GPU expectation comes from (group_topics_numpy) is checked
against an example worked by hand; group_prevalence_finish (the C call through
its Python twin) is checked against direct numpy formulas on those integers at
rtol 1e-12, the project's fp64 bar, and its NaN / -inf cases by kind; the
selection and the text are checked from given arrays; the Python faces run
against a stand-in library.  The GPU behaviour is in test_group_topics_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

import group_topics_numpy as N

SAMPLER_CALLS = ["lda_group_topics", "lda_group_topics_path", "lda_debug_group_topics_global", "lda_subcorpus_count",
                 "lda_subcorpus_merge", "lda_subcorpus_top_words", "lda_subcorpus_release"]
MODEL_CALLS = ["ldatm_group_topics", "ldatm_group_prevalence_finish", "ldatm_group_prevalence",
               "ldatm_group_top_topics_select", "ldatm_group_topics_text", "ldatm_print_group_topics",
               "ldatm_group_topics_format", "ldatm_subcorpus_top_words"]
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
    assert "#define LDA_GROUP_TOPICS_MAX_CELLS (1 << 28)\n" in text and capi.GROUP_TOPICS_MAX_CELLS == 1 << 28
    assert "#define LDA_ABI_VERSION 8" in text and L.lda_abi_version() == 8
    tm_text = open(TM_HEADER).read()
    for name, v in tm.GROUP_KINDS.items():
        assert "#define LDATM_GROUP_%s %d\n" % (name.upper(), v) in tm_text
    assert tuple(tm.GROUP_KINDS) == N.KINDS and set(tm.GROUP_KIND_TABLE) == set(tm.GROUP_KINDS)
    assert capi.GROUP_TOPICS_STATS == N.STATS
    assert {v for v in tm.GROUP_KIND_TABLE.values() if v} == set(N.STATS)


def test_sampler_calls_reject_a_null_context_and_the_helpers_need_none(libs):
    L, _ = libs
    out = np.zeros(16, np.int64)
    p = out.ctypes.data
    assert L.lda_group_topics(None, p, 3, 10, 2, 0.05, p, p, p, p, p) == -1 and b"null ctx" in L.lda_last_error()
    assert L.lda_subcorpus_count(None, p, 0) == -1 and b"null ctx" in L.lda_last_error()
    assert L.lda_subcorpus_merge(None, None) == -1 and b"null ctx" in L.lda_last_error()
    assert L.lda_subcorpus_top_words(None, 3, p, p, p) == -1 and b"null ctx" in L.lda_last_error()
    assert L.lda_subcorpus_release(None) == -1 and b"null ctx" in L.lda_last_error()
    assert not out.any()
    L.lda_debug_group_topics_global(1)
    L.lda_debug_group_topics_global(0)


def test_group_topics_path_is_the_lds_budget(libs):
    """The path helper, from the header's words alone: 24 Kp bytes of wave
    histograms and lists, 8 bytes per cell of the two [G] vectors and the
    tables, 64 KiB in all."""
    L, _ = libs
    lds = C.c_int32()
    for K in (1, 4, 20, 64, 65, 300, 512, 2048, 4096):
        Kp = L.lda_padded_topics(K)
        for tables in (1, 2, 3):
            for G in (1, 2, 3, 20, 37, 100, 1000, 5000):
                need = 24 * Kp + 8 * (2 * G + tables * G * K)
                path = L.lda_group_topics_path(G, K, tables, C.byref(lds))
                assert path == (1 if need <= 65536 else 0), (G, K, tables)
                assert lds.value == (need if path else 24 * Kp)
    assert L.lda_group_topics_path(3, 4, 3, None) == 1
    assert L.lda_group_topics_path(1, 4096, 1, None) == 0            # the histograms alone pass 64 KiB
    for bad in ((0, 4, 1), (3, 0, 1), (3, 4097, 1), (3, 4, 0), (3, 4, 4)):
        assert L.lda_group_topics_path(*bad, C.byref(lds)) == -1 and lds.value == 0


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
    gt = T.ldatm_group_topics
    assert gt(None, ip, 3, 10, 2, 0.05, p, p, p, p, p) == -1 and b"null" in err()
    for G in (0, -2):
        assert gt(handle, ip, G, 10, 2, 0.05, p, p, p, p, p) == -1 and b"G must be" in err()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert gt(handle, ip, 3, 10, 2, 0.05, *args, None, None) == -1 and b"null output" in err()
    for mt in (0, -3):
        assert gt(handle, ip, 3, mt, 2, 0.05, p, p, p, p, p) == -1 and b"min_tokens" in err()
    for mc in (0, -1):
        assert gt(handle, ip, 3, 10, mc, 0.05, p, p, p, p, p) == -1 and b"min_count" in err()
    for mp in BAD_PROPS:
        assert gt(handle, ip, 3, 10, 2, mp, p, p, p, p, p) == -1 and b"min_prop" in err()
    assert gt(handle, ip, (1 << 26) + 1, 10, 2, 0.05, p, p, p, None, None) == -5 and b"MAX_CELLS" in err()
    prev, text, prnt = T.ldatm_group_prevalence, T.ldatm_group_topics_text, T.ldatm_print_group_topics
    size = C.c_size_t()
    assert prev(None, ip, 3, 2, 10, 2, 0.05, fp) == -1 and b"null" in err()
    for kind in (-1, 4, 99):
        assert prev(handle, ip, 3, kind, 10, 2, 0.05, fp) == -1 and b"kind" in err()
        assert text(handle, ip, 3, kind, 3, 10, 2, 0.05, None, 0, C.byref(size)) == -1 and b"kind" in err()
        assert prnt(handle, b"/nonexistent/x", ip, 3, kind, 3, 10, 2, 0.05) == -1 and b"kind" in err()
    assert prev(handle, ip, 0, 2, 10, 2, 0.05, fp) == -1 and b"G must be" in err()
    assert prev(handle, ip, 3, 2, 0, 2, 0.05, fp) == -1 and b"min_tokens" in err()
    assert prev(handle, ip, 3, 2, 10, 0, 0.05, fp) == -1 and b"min_count" in err()
    for mp in BAD_PROPS:
        assert prev(handle, ip, 3, 2, 10, 2, mp, fp) == -1 and b"min_prop" in err()
    assert prev(handle, ip, 3, 2, 10, 2, 0.05, None) == -1 and b"null output" in err()
    assert text(None, ip, 3, 2, 3, 10, 2, 0.05, None, 0, C.byref(size)) == -1
    assert text(handle, ip, 3, 2, 0, 10, 2, 0.05, None, 0, C.byref(size)) == -1 and b"n must be" in err()
    assert text(handle, ip, 0, 2, 3, 10, 2, 0.05, None, 0, C.byref(size)) == -1 and b"G must be" in err()
    assert prnt(handle, b"/nonexistent/x", ip, 3, 2, 3, 0, 2, 0.05) == -1 and b"min_tokens" in err()
    assert prnt(handle, b"/nonexistent/x", ip, 3, 2, 3, 10, 0, 0.05) == -1 and b"min_count" in err()
    assert prnt(handle, b"/nonexistent/x", ip, 3, 2, 3, 10, 2, math.nan) == -1 and b"min_prop" in err()
    assert prnt(None, b"/nonexistent/x", ip, 3, 2, 3, 10, 2, 0.05) == -1
    sub = T.ldatm_subcorpus_top_words
    assert sub(None, p, 3, ip, ip, p) == -1 and b"null" in err()
    for n in (0, -1, capi.TOP_WORDS_MAX + 1):
        assert sub(handle, p, n, ip, ip, p) == -1 and b"n must be" in err()
    for args in ((None, ip, p), (ip, None, p), (ip, ip, None)):
        assert sub(handle, p, 3, *args) == -1 and b"null output" in err()
    # every argument is good: the model has no documents to build a shard from
    assert gt(handle, None, 3, 10, 2, 0.05, p, p, p, p, p) == -4 and b"addInstances" in err()
    assert sub(handle, None, 3, ip, ip, p) == -4 and b"addInstances" in err()
    assert not a.any() and not f.any() and not ids.any()          # nothing was written


# ------------------------------------------------- the restatement, by hand
# K = 4, G = 3, min_tokens 3, min_count 2, min_prop 0.25:
#   d0 g0 []                       empty: under min_tokens
#   d1 g-1 [0 0 1 1 1 1]           left out
#   d2 g0 [0 0]                    L 2: under min_tokens, counts nowhere
#   d3 g0 [3 3 0 0 0 0 0 0]        L 8,  n (6 0 0 2), 0.25 L = 2.0: topic 3 exactly at min_count and at min_prop L
#                                  shares 6 2^32 / 8 = 3 2^30, 2 2^32 / 8 = 2^30
#   d4 g1 [1 2 2]                  L 3,  n (0 1 2 0): topic 1 under min_count; shares floor(2^32 / 3),
#                                  floor(2^33 / 3)
#   d5 g0 [1 1 1 2 x 9]            L 12, n (0 3 9 0), 0.25 L = 3.0: topic 1 exactly at min_prop L
#                                  shares 2^30, 3 2^30
#   d6 g1 [0 0 1 x 10]             L 12, n (2 10 0 0): topic 0 at min_count but under 3.0: absent
#                                  shares floor(2^32 / 6), floor(10 2^32 / 12)
#   group 2: nobody
DOC_OFF = np.array([0, 0, 6, 8, 16, 19, 31, 43], np.int64)
Z = np.array([0, 0, 1, 1, 1, 1] + [0, 0] + [3, 3, 0, 0, 0, 0, 0, 0] + [1, 2, 2] + [1, 1, 1] + [2] * 9 + [0, 0] +
             [1] * 10, np.int32)
GROUPS = np.array([0, -1, 0, 0, 1, 0, 1], np.int32)
GROUP_DOCS = [2, 2, 0]
GROUP_TOKENS = [20, 15, 0]
TOKENS = [[6, 3, 9, 2], [2, 11, 2, 0], [0, 0, 0, 0]]
PRESENT = [[1, 1, 1, 1], [0, 1, 1, 0], [0, 0, 0, 0]]
SHARES = [[3 << 30, 1 << 30, 3 << 30, 1 << 30],
          [715827882, 1431655765 + 3579139413, 2863311530, 0],
          [0, 0, 0, 0]]
THR = dict(min_tokens=3, min_count=2, min_prop=0.25)


def test_restatement_against_the_hand_worked_example():
    assert len(Z) == DOC_OFF[-1] and len(GROUPS) == len(DOC_OFF) - 1 == 7
    assert (1 << 32) // 3 == 1431655765 and (2 << 32) // 3 == 2863311530
    assert (2 << 32) // 12 == 715827882 and (10 << 32) // 12 == 3579139413
    e = N.expected_group_topics(Z, DOC_OFF, 4, GROUPS, 3, **THR)
    assert e["group_docs"].tolist() == GROUP_DOCS and e["group_tokens"].tolist() == GROUP_TOKENS
    assert e["tokens"].tolist() == TOKENS and e["present"].tolist() == PRESENT and e["shares"].tolist() == SHARES
    assert e["shares"].dtype == np.uint64 and e["shares"][1, 1] > 2 ** 32
    for name in ("group_docs", "group_tokens", "tokens", "present"):
        assert e[name].dtype == np.int64
    assert e["tokens"].sum(axis=1).tolist() == GROUP_TOKENS
    # only the requested tables exist, and the others do not change
    one = N.expected_group_topics(Z, DOC_OFF, 4, GROUPS, 3, **THR, stats=("shares",))
    assert set(one) == {"group_docs", "group_tokens", "tokens", "shares"} and one["shares"].tolist() == SHARES
    none = N.expected_group_topics(Z, DOC_OFF, 4, GROUPS, 3, **THR, stats=())
    assert set(none) == {"group_docs", "group_tokens", "tokens"} and none["tokens"].tolist() == TOKENS


def test_restatement_thresholds_and_groups():
    # a hair above 0.25 drops the two topics that sat exactly on min_prop L; nothing else moves
    e = N.expected_group_topics(Z, DOC_OFF, 4, GROUPS, 3, 3, 2, np.nextafter(0.25, 1.0))
    assert e["present"].tolist() == [[1, 0, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
    assert e["tokens"].tolist() == TOKENS and e["shares"].tolist() == SHARES
    # min_tokens 1 takes d2 in, min_tokens 4 drops d4
    e = N.expected_group_topics(Z, DOC_OFF, 4, GROUPS, 3, 1, 1, 0.0)
    assert e["group_docs"].tolist() == [3, 2, 0] and e["tokens"][0].tolist() == [8, 3, 9, 2]
    assert e["shares"][0, 0] == (3 << 30) + (1 << 32) and e["present"][1].tolist() == [1, 2, 1, 0]
    e = N.expected_group_topics(Z, DOC_OFF, 4, GROUPS, 3, 4, 2, 0.25)
    assert e["group_docs"].tolist() == [2, 1, 0] and e["tokens"][1].tolist() == [2, 10, 0, 0]
    # everybody in one group, d1 included
    e = N.expected_group_topics(Z, DOC_OFF, 4, np.zeros(7, np.int32), 1, 3, 2, 0.25)
    assert e["group_docs"].tolist() == [5] and e["group_tokens"].tolist() == [41]
    e = N.expected_group_topics(Z, DOC_OFF, 4, np.full(7, -1), 2, 1, 1, 0.0)
    assert not any(v.any() for v in e.values())


def test_restatement_of_the_subcorpus_words_by_hand():
    words = np.array([0, 1, 0, 2, 2, 1] + [1, 1] + [4, 4, 0, 0, 3, 3, 3, 1] + [2, 2, 0] + [0] * 12 + [1] * 12, np.int32)
    assert len(words) == len(Z)
    mask = np.array([1, 0, 1, 1, 0, 0, 0], np.uint8)                 # d0 (empty), d2, d3
    sub = N.subcorpus_table(Z, words, DOC_OFF, 5, 4, mask)
    #        d2: (1,0) x 2;  d3: (4,3) x 2, (0,0) x 2, (3,0) x 3, (1,0)
    want = np.zeros((5, 4), np.int64)
    want[1, 0], want[4, 3], want[0, 0], want[3, 0] = 3, 2, 2, 3
    assert sub.tolist() == want.tolist()
    ids, cnt, tot = N.table_top_words(sub, 3)
    assert ids.tolist() == [[1, 3, 0], [-1, -1, -1], [-1, -1, -1], [4, -1, -1]]     # 1 before 3: equal counts by word
    assert cnt.tolist() == [[3, 3, 2], [0, 0, 0], [0, 0, 0], [2, 0, 0]] and tot.tolist() == [8, 0, 0, 2]
    assert ids.dtype == np.int32 and cnt.dtype == np.int32 and tot.dtype == np.int64
    assert not N.subcorpus_table(Z, words, DOC_OFF, 5, 4, np.zeros(7)).any()
    assert N.subcorpus_table(Z, words, DOC_OFF, 5, 4, np.ones(7)).sum() == len(Z)


# ------------------------------------------------------------- the kinds
def _ints():
    return (np.array(GROUP_DOCS, np.int64), np.array(GROUP_TOKENS, np.int64), np.array(TOKENS, np.int64),
            np.array(PRESENT, np.int64), np.array(SHARES, np.uint64))


def test_finish_against_direct_numpy_formulas(libs):
    gd, gt, tok, pre, shr = _ints()
    with np.errstate(divide="ignore", invalid="ignore"):
        share = tok / gt[:, None].astype(np.float64)
        direct = {
            "tokens": share,
            "documents": pre / gd[:, None].astype(np.float64),
            "mean": shr.astype(np.float64) / 2.0 ** 32 / gd[:, None],
            "lift": np.log(share / (tok.sum(axis=0) / gt.sum())),
        }
    for kind, want in direct.items():
        got = tm.group_prevalence_finish(kind, gd, gt, tok, pre, shr)
        assert got.shape == (3, 4) and got.dtype == np.float64
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), kind
        fin = np.isfinite(want)
        np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=0, err_msg=kind)
        assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), kind      # lift's -inf
        assert np.all(np.isnan(got[2])), kind                                  # the group nobody belongs to
        # the Python restatement cell by cell gives the same bits
        assert N.same_floats(got, N.finish(kind, gd, gt, tok, pre, shr)), kind
    got = tm.group_prevalence_finish("tokens", gd, gt, tok)
    assert got[0].tolist() == [6 / 20, 3 / 20, 9 / 20, 2 / 20] and got[1, 3] == 0.0
    got = tm.group_prevalence_finish("documents", gd, gt, tok, present=pre)
    assert got[:2].tolist() == [[0.5, 0.5, 0.5, 0.5], [0.0, 0.5, 0.5, 0.0]]
    got = tm.group_prevalence_finish("mean", gd, gt, tok, shares=shr)
    assert got[0].tolist() == [0.375, 0.125, 0.375, 0.125]                     # (6/8 + 0) / 2, (0 + 3/12) / 2, ...
    assert abs(got[1, 1] - (1 / 3 + 10 / 12) / 2) < 2 * 2.0 ** -32 and got[1, 1] <= (1 / 3 + 10 / 12) / 2
    got = tm.group_prevalence_finish("lift", gd, gt, tok)
    assert got[1, 3] == -math.inf and got[0, 3] == math.log((2 / 20) / (2 / 35))


def test_finish_nan_and_inf_cases_by_kind(libs):
    """Group 1 has no used document; topic 2 has no token in any group."""
    gd = np.array([3, 0, 2], np.int64)
    gt = np.array([30, 0, 10], np.int64)
    tok = np.array([[10, 20, 0, 0], [0, 0, 0, 0], [5, 0, 0, 5]], np.int64)
    pre = np.array([[3, 2, 0, 0], [0, 0, 0, 0], [2, 0, 0, 1]], np.int64)
    shr = np.array([[1 << 32, 2 << 32, 0, 0], [0, 0, 0, 0], [1 << 32, 0, 0, 1 << 32]], np.uint64)
    for kind in N.KINDS:
        got = tm.group_prevalence_finish(kind, gd, gt, tok, pre, shr)
        assert np.all(np.isnan(got[1])), kind
        assert N.same_floats(got, N.finish(kind, gd, gt, tok, pre, shr)), kind
    for kind in ("tokens", "documents", "mean"):
        got = tm.group_prevalence_finish(kind, gd, gt, tok, pre, shr)
        assert np.isfinite(got[[0, 2]]).all() and got[0, 2] == 0.0, kind
    assert tm.group_prevalence_finish("mean", gd, gt, tok, shares=shr)[0].tolist() == [1 / 3, 2 / 3, 0.0, 0.0]
    lift = tm.group_prevalence_finish("lift", gd, gt, tok)
    assert np.all(np.isnan(lift[:, 2]))                                   # N_k = 0: NaN, not -inf
    assert lift[0, 3] == -math.inf and lift[2, 1] == -math.inf
    assert lift[2, 3] == math.log((5 / 10) / (5 / 40)) and lift[0, 0] == math.log((10 / 30) / (15 / 40))
    # no used document at all: everything is NaN
    z3, z34 = np.zeros(3, np.int64), np.zeros((3, 4), np.int64)
    for kind in N.KINDS:
        assert np.all(np.isnan(tm.group_prevalence_finish(kind, z3, z3, z34, z34, z34.astype(np.uint64))))
    # a share sum above 2^63 is an unsigned value, not a negative one
    big = np.array([[(1 << 63) + (1 << 40)]], np.uint64)
    got = tm.group_prevalence_finish("mean", [1 << 31], [1 << 40], [[1 << 40]], shares=big)
    assert got[0, 0] == float((1 << 63) + (1 << 40)) / (4294967296.0 * float(1 << 31)) > 0


def test_finish_rejects_a_missing_table_and_an_unknown_kind(libs):
    _, T = libs
    gd, gt, tok, pre, shr = _ints()
    out = np.zeros((3, 4))
    g, t, k, p, s, o = (x.ctypes.data for x in (gd, gt, tok, pre, shr, out))
    call, err = T.ldatm_group_prevalence_finish, T.ldatm_last_error
    for kind in range(4):
        assert call(kind, 3, 4, g, t, k, p, s, o) == 0
    assert call(0, 3, 4, g, t, k, None, None, o) == 0 and call(3, 3, 4, g, t, k, None, None, o) == 0
    assert call(1, 3, 4, g, t, k, None, s, o) == -1 and b"documents takes present" in err()
    assert call(2, 3, 4, g, t, k, p, None, o) == -1 and b"mean takes shares" in err()
    for kind in (-1, 4):
        assert call(kind, 3, 4, g, t, k, p, s, o) == -1 and b"kind" in err()
    assert call(0, 0, 4, g, t, k, p, s, o) == -1 and b"G must" in err()
    assert call(0, 3, 0, g, t, k, p, s, o) == -1 and b"K must" in err()
    for args in ((None, t, k), (g, None, k), (g, t, None)):
        assert call(0, 3, 4, *args, p, s, o) == -1 and b"null input" in err()
    assert call(0, 3, 4, g, t, k, p, s, None) == -1 and b"null output" in err()
    with pytest.raises(capi.LdaError, match="documents takes present"):
        tm.group_prevalence_finish("documents", gd, gt, tok, shares=shr)
    with pytest.raises(capi.LdaError, match="mean takes shares"):
        tm.group_prevalence_finish("mean", gd, gt, tok, present=pre)
    with pytest.raises(ValueError, match="unknown kind"):
        tm.group_prevalence_finish("median", gd, gt, tok)
    with pytest.raises(ValueError, match=r"\[G, K\]"):
        tm.group_prevalence_finish("tokens", gd[:2], gt, tok)
    with pytest.raises(ValueError, match="as tokens"):
        tm.group_prevalence_finish("mean", gd, gt, tok, shares=shr[:, :3])


# ------------------------------------------------------------ the selection
def test_top_topics_tie_order_non_finite_values_and_padding(libs):
    nan, inf = math.nan, math.inf
    mat = np.array([[0.5, 0.25, 0.5, nan, 0.5],
                    [0.5, 9.0, -inf, 0.25, inf],
                    [nan, nan, nan, nan, nan],
                    [0.1, 0.3, 0.2, 0.3, -1.0]])
    ids, values = tm.group_top_topics_select(mat, 3)
    assert ids.dtype == np.int32 and values.dtype == np.float64
    # equal values by smaller id; NaN and the infinities are left out; a row has no diagonal to skip
    assert ids.tolist() == [[0, 2, 4], [1, 0, 3], [-1, -1, -1], [1, 3, 2]]
    assert N.same_floats(values, [[0.5, 0.5, 0.5], [9.0, 0.5, 0.25], [nan] * 3, [0.3, 0.3, 0.2]])
    ids, values = tm.group_top_topics_select(mat, 7)                    # n > K: every row ends in -1 / NaN
    assert ids.shape == (4, 7) and np.all(ids[:, 5:] == -1) and np.all(np.isnan(values[:, 5:]))
    assert ids[3].tolist() == [1, 3, 2, 0, 4, -1, -1] and ids[0].tolist() == [0, 2, 4, 1, -1, -1, -1]
    for n in (1, 3, 5, 7):
        got, want = tm.group_top_topics_select(mat, n), N.top_topics(mat, n)
        assert np.array_equal(got[0], want[0]) and N.same_floats(got[1], want[1])
    ids, values = tm.group_top_topics_select(np.ones((1, 1)), 2)
    assert ids.tolist() == [[0, -1]] and values[0, 0] == 1.0 and math.isnan(values[0, 1])
    with pytest.raises(ValueError, match="n must be"):
        tm.group_top_topics_select(mat, 0)
    with pytest.raises(ValueError, match=r"\[G, K\]"):
        tm.group_top_topics_select(mat[0], 2)
    _, T = libs
    out_i, out_v = np.zeros(8, np.int32), np.zeros(8)
    call, err = T.ldatm_group_top_topics_select, T.ldatm_last_error
    assert call(4, 5, 2, None, out_i.ctypes.data, out_v.ctypes.data) == -1 and b"null matrix" in err()
    assert call(4, 5, 0, mat.ctypes.data, out_i.ctypes.data, out_v.ctypes.data) == -1 and b"n must be" in err()
    assert call(0, 5, 2, mat.ctypes.data, out_i.ctypes.data, out_v.ctypes.data) == -1 and b"G must be" in err()
    assert call(4, 0, 2, mat.ctypes.data, out_i.ctypes.data, out_v.ctypes.data) == -1 and b"K must be" in err()
    assert call(4, 5, 2, mat.ctypes.data, None, out_v.ctypes.data) == -1 and b"null output" in err()
    assert not out_i.any() and not out_v.any()


# ------------------------------------------------------------------ the text
def test_group_topics_text_from_given_arrays(libs):
    ids = np.array([[2, 1, -1], [0, -1, -1], [-1, -1, -1]], np.int32)
    values = np.array([[0.75, -0.125, math.nan], [1e-5, math.nan, math.nan], [math.nan] * 3])
    assert tm.format_group_topics(ids, values) == ("#group topic value\n"
                                                   "0 2 0.75\n"
                                                   "0 1 -0.125\n"
                                                   f"1 0 {tm.format_double(1e-5)}\n")
    assert tm.format_double(1e-5) == "1.0E-5"
    assert tm.format_group_topics(np.full((3, 2), -1, np.int32), np.full((3, 2), math.nan)) == "#group topic value\n"
    with pytest.raises(ValueError, match="one shape"):
        tm.format_group_topics(ids, values[:, :2])
    # from the hand-worked integers to the text in one go
    gd, gt, tok, pre, shr = _ints()
    mat = tm.group_prevalence_finish("mean", gd, gt, tok, shares=shr)
    ti, tv = tm.group_top_topics_select(mat, 2)
    assert ti.tolist() == [[0, 2], [1, 2], [-1, -1]]
    lines = tm.format_group_topics(ti, tv).splitlines()
    assert lines[:3] == ["#group topic value", "0 0 0.375", "0 2 0.375"] and len(lines) == 5
    assert lines[3] == f"1 1 {tm.format_double(mat[1, 1])}" and float(lines[3].split()[2]) == mat[1, 1]


# ----------------------------------------------------------- Python faces
class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def _array(ptr, n, ctype):
    return np.ctypeslib.as_array((ctype * n).from_address(ptr))


class _CountsOnTheHost:
    """Stands where liblda_topic_model would for the one device call of
    topicsByGroup: ldatm_group_topics answers from the numpy restatement over
    the planted z; the host-only calls go to the real library."""

    def __init__(self, real, z, doc_off, K):
        self.real, self.z, self.doc_off, self.K, self.calls = real, z, doc_off, K, []

    def __getattr__(self, name):
        assert name in ("ldatm_group_prevalence_finish", "ldatm_group_top_topics_select"), name
        return getattr(self.real, name)

    def ldatm_group_topics(self, h, ids, G, mt, mc, mp, gd, gt, tok, pre, shr):
        D = len(self.doc_off) - 1
        groups = _array(ids, D, C.c_int32).copy()
        stats = tuple(s for s, p in (("present", pre), ("shares", shr)) if p)
        self.calls.append((groups.tolist(), G, stats))
        e = N.expected_group_topics(self.z, self.doc_off, self.K, groups, G, mt, mc, mp, stats)
        _array(gd, G, C.c_int64)[:] = e["group_docs"]
        _array(gt, G, C.c_int64)[:] = e["group_tokens"]
        _array(tok, G * self.K, C.c_int64)[:] = e["tokens"].ravel()
        if pre:
            _array(pre, G * self.K, C.c_int64)[:] = e["present"].ravel()
        if shr:
            _array(shr, G * self.K, C.c_uint64)[:] = e["shares"].ravel()
        return 0


def test_python_helpers_check_their_arguments():
    assert capi.group_topics_stats("shares") == ("shares",) and capi.group_topics_stats(()) == ()
    assert capi.group_topics_stats(["shares", "present"]) == ("present", "shares")
    with pytest.raises(ValueError, match="unknown statistic"):
        capi.group_topics_stats(("present", "tokens"))
    ids, G = capi.group_ids([0, -1, 2, 2], 4)
    assert ids.dtype == np.int32 and ids.tolist() == [0, -1, 2, 2] and G == 3
    assert capi.group_ids([-1, -1], 2)[1] == 1 and capi.group_ids([], 0)[1] == 1 and capi.group_ids([0], 1, 5)[1] == 5
    with pytest.raises(ValueError, match=r"doc_group\[2\] = 3 is outside"):
        capi.group_ids([0, 1, 3, 7], 4, 3)
    with pytest.raises(ValueError, match=r"doc_group\[1\] = -2 is outside"):
        capi.group_ids([0, -2], 2)
    with pytest.raises(ValueError, match="one group id per document"):
        capi.group_ids([0, 1], 3)
    with pytest.raises(ValueError, match="G must be"):
        capi.group_ids([-1], 1, 0)
    assert capi.doc_mask([0, 2, True, False], 4).tolist() == [0, 1, 1, 0]
    assert capi.doc_mask([0, 2], 2).dtype == np.uint8
    with pytest.raises(ValueError, match="one entry per document"):
        capi.doc_mask([1, 0], 3)
    labels, ids = tm.group_labels(["b", None, "a", "b", "c"])
    assert labels == ["a", "b", "c"] and ids.tolist() == [1, -1, 0, 1, 2] and ids.dtype == np.int32
    labels, ids = tm.group_labels([2007, 1999, 2007, None])
    assert labels == [1999, 2007] and ids.tolist() == [1, 0, 1, -1]
    labels, ids = tm.group_labels([1, "x", None])                    # labels that do not compare: still an order
    assert sorted(ids.tolist()) == [-1, 0, 1] and set(labels) == {1, "x"}


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    for name in ("group_topics", "subcorpus_count", "subcorpus_merge", "subcorpus_top_words", "subcorpus_release"):
        assert callable(getattr(GibbsSampler, name))
    for name in ("groupTopics", "topicsByGroup", "getGroupTopTopics", "subCorpusTopWords", "getSubCorpusTopWords",
                 "getGroupTopWords", "printGroupTopics", "groupTopicsText"):
        assert callable(getattr(tm.ParallelTopicModel, name))
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    with pytest.raises(ValueError, match="unknown statistic"):
        g.group_topics([0, 0, 0], stats=("present", "mean"))
    with pytest.raises(ValueError, match="min_tokens"):
        g.group_topics([0, 0, 0], min_tokens=0)
    with pytest.raises(ValueError, match="min_count"):
        g.group_topics([0, 0, 0], min_count=0)
    for bad in BAD_PROPS:
        with pytest.raises(ValueError, match="min_prop"):
            g.group_topics([0, 0, 0], min_prop=bad)
    with pytest.raises(ValueError, match="one group id per document"):
        g.group_topics([0, 0])
    with pytest.raises(ValueError, match=r"doc_group\[1\] = 2 is outside"):
        g.group_topics([0, 2, 0], G=2)
    with pytest.raises(ValueError, match="one entry per document"):
        g.subcorpus_count([1, 0])
    with pytest.raises(TypeError, match="GibbsSampler"):
        g.subcorpus_merge(object())
    for n in (0, capi.TOP_WORDS_MAX + 1):
        with pytest.raises(ValueError, match="n must be"):
            g.subcorpus_top_words(n)
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        m.data = [tm.Instance([0, 1], target=t) for t in ("b", "a", None)]
        for call in (m.topicsByGroup, lambda **kw: m.getGroupTopTopics(3, **kw), lambda **kw: m.groupTopicsText(3, **kw),
                     lambda **kw: m.printGroupTopics("/nonexistent/x", 3, **kw)):
            with pytest.raises(ValueError, match="unknown kind"):
                call(kind="median")
            with pytest.raises(ValueError, match="min_tokens"):
                call(minTokens=0)
            with pytest.raises(ValueError, match="one label per document"):
                call(groups=["a", "b"])
            with pytest.raises(ValueError, match="every label is None"):
                call(groups=[None, None, None])
        with pytest.raises(ValueError, match="unknown statistic"):
            m.topicsByGroup(stats=("tokens",))
        for call in (m.getGroupTopTopics, m.groupTopicsText):
            with pytest.raises(ValueError, match="n must be"):
                call(0)
        with pytest.raises(ValueError, match="n must be"):
            m.printGroupTopics("/nonexistent/x", 0)
        with pytest.raises(ValueError, match="n must be"):
            m.subCorpusTopWords([1, 1, 0], 0)
        with pytest.raises(ValueError, match="one entry per document"):
            m.getSubCorpusTopWords([1, 1], 3)
        with pytest.raises(ValueError, match="unknown label"):
            m.getGroupTopWords("z", 3)
        with pytest.raises(ValueError, match=r"doc_group\[0\] = 5"):
            m.groupTopics([5, 0, 0], G=2)
    finally:
        m._L = real
        m.data = []
        m.close()


def test_topics_by_group_from_targets_with_a_stand_in_library(libs):
    """groups=None takes each instance's target: the sorted distinct targets
    are the labels and a None target is left out.  The device call is answered
    by the numpy restatement on the hand-worked z; everything else is real."""
    _, T = libs
    targets = ["news", None, "news", "news", "blog", "news", "blog"]          # GROUPS with blog = 0, news = 1
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        fake = _CountsOnTheHost(real, Z, DOC_OFF, 4)
        m._L = fake
        m.data = [tm.Instance(np.zeros(int(n), np.int32), target=t) for n, t in zip(np.diff(DOC_OFF), targets)]
        r = m.topicsByGroup(minTokens=3, minCount=2, minProp=0.25)
        assert fake.calls == [([1, -1, 1, 1, 0, 1, 0], 2, ("shares",))]         # mean counts shares only
        assert r.kind == "mean" and r.labels == ["blog", "news"]
        assert r.groupDocs.tolist() == [2, 2] and r.groupTokens.tolist() == [15, 20]
        assert set(r.counts) == {"tokens", "shares"} and r.counts["tokens"].tolist() == [TOKENS[1], TOKENS[0]]
        assert r.values.shape == (2, 4) and r.values[1].tolist() == [0.375, 0.125, 0.375, 0.125]
        r = m.topicsByGroup(kind="documents", stats=("shares",), minTokens=3, minCount=2, minProp=0.25)
        assert fake.calls[-1][2] == ("present", "shares") and set(r.counts) == {"tokens", "present", "shares"}
        assert r.values.tolist() == [[0.0, 0.5, 0.5, 0.0], [0.5, 0.5, 0.5, 0.5]]
        r = m.topicsByGroup(kind="lift", minTokens=3, minCount=2, minProp=0.25)
        assert fake.calls[-1][2] == () and r.values[0, 3] == -math.inf
        # explicit labels, ints among them; the same numbers under other names
        years = [2001, 1999, 2001, 2001, 1999, 2001, 1999]
        r = m.topicsByGroup(years, "tokens", minTokens=3, minCount=2, minProp=0.25)
        assert r.labels == [1999, 2001] and fake.calls[-1][0] == [1, 0, 1, 1, 0, 1, 0]
        assert r.groupDocs.tolist() == [3, 2]                                   # d1 counts now
        top = m.getGroupTopTopics(2, kind="mean", minTokens=3, minCount=2, minProp=0.25)
        assert list(top) == ["blog", "news"] and top["news"] == [(0, 0.375), (2, 0.375)]
        assert [t for t, _ in top["blog"]] == [1, 2]
    finally:
        m._L = real
        m.data = []
        m.close()
