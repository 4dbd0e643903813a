"""GPU checks of the topics-by-group readout: lda_group_topics
(k_group_topics), the sub-corpus table (k_subcorpus_count, k_subcorpus_add,
k_subcorpus_totals and lda_top_words' selection kernels on it) and their ldatm_
mirrors.

Every expectation is the numpy restatement (group_topics_numpy) on the z that
the test planted with set_z, so nothing needs training.  Every output is an
integer and is compared byte for byte; no tolerance appears anywhere.

Geometry.  One wave takes a document; a block is four waves and the grid is
capped at 8 blocks per CU, P = 32 x CUs documents a trip: the second-trip tests
hold 2 P + 37 documents.  lda_group_topics accumulates in LDS when the two [G]
vectors, the requested tables and the block's histograms and lists fit 64 KiB,
with global atomics otherwise: lda_group_topics_path says which, the shape test
takes for every K the last G on the LDS side and the first on the global side
from it, and the hook lda_debug_group_topics_global runs the global path at
small shapes, where both must give the same bytes.  A document's distinct
topics go into a per-wave list that is walked 64 entries at a time: documents
with 1, 2, 20, 100, 299 and 2500 distinct topics cover a list shorter than,
equal to and (far) longer than a wave."""
import contextlib
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

import group_topics_numpy as N

pytestmark = pytest.mark.gpu

V = 50
HEAD = ("group_docs", "group_tokens", "tokens")


# ------------------------------------------------------------------ helpers
def _planted(docs, seed=1, num_types=V):
    """(Corpus, z) of documents given as their topic sequences."""
    lens = np.array([len(d) for d in docs], np.int64)
    off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    z = np.concatenate([np.asarray(d, np.int32) for d in docs] + [np.zeros(0, np.int32)]).astype(np.int32)
    words = np.random.default_rng(seed).integers(0, num_types, int(off[-1])).astype(np.int32)
    return Corpus(off, words, num_types), z


def _ragged_docs(K, D, seed, max_len=400):
    """D documents of 0 .. max_len tokens, each over a few topics of its own
    with skewed shares, so counts repeat, tie and straddle the thresholds."""
    rng = np.random.default_rng(seed)
    docs = []
    for _ in range(D):
        L = int(rng.integers(0, max_len + 1))
        m = int(rng.integers(1, min(K, 12) + 1))
        topics = rng.choice(K, m, replace=False)
        p = rng.dirichlet(np.full(m, 0.5))
        docs.append(topics[rng.choice(m, L, p=p)].astype(np.int32))
    return docs


def _shape_docs(K, seed):
    docs = _ragged_docs(K, 500, seed)
    docs[3] = np.zeros(0, np.int32)                                   # empty
    docs[4] = np.array([K - 1], np.int32)                             # one token
    docs[5] = np.full(64, K // 2, np.int32)                           # one topic, one wave's lanes
    docs[6] = (np.arange(65) % 2).astype(np.int32)                    # two topics, 65 tokens
    docs[7] = (np.arange(400) % min(K, 20)).astype(np.int32)          # every topic at K <= 20
    docs[-1] = np.full(11, K - 1, np.int32)                           # the last wave's document
    if K >= 300:
        docs[8] = (np.arange(400) % 100).astype(np.int32)             # 100 distinct: a list longer than a wave
        docs[9] = np.arange(299, dtype=np.int32)                      # an odd number of entries, all counts 1
        docs[10] = np.concatenate([np.arange(K - 129, K), np.arange(K - 60, K)]).astype(np.int32)   # the top ids
    if K >= 4096:
        # more than 2048 distinct topics, some of them three times
        docs[11] = np.concatenate([np.arange(2500), np.arange(150), np.arange(150)]).astype(np.int32)
    return docs


def _groups(D, G, seed):
    """One id in [-1, G) per document: some left out, group 1 empty (G >= 3),
    group G - 1 used by the last document only (G >= 2)."""
    g = np.random.default_rng(seed).integers(-1, G, D).astype(np.int32)
    if G >= 3:
        g[g == 1] = 0
    if G >= 2:
        g[g == G - 1] = 0
        g[-1] = G - 1
    g[:12] = np.where(g[:12] < 0, 0, g[:12])          # the planted documents count
    g[2] = -1
    return g


def _sampler_kind(K):
    return "sparse" if K > capi.MAX_TOPICS_DENSE else "dense"


@contextlib.contextmanager
def _planted_sampler(docs, K, seed=11, num_types=V, word_seed=1):
    from ldagibbssampling_amd.sampler import GibbsSampler
    c, z = _planted(docs, word_seed, num_types)
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=seed,
                      sampler=_sampler_kind(K)) as g:
        g.set_z(z)
        g.apply()
        yield g, c, z


@contextlib.contextmanager
def _global_atomics():
    L = capi.load()
    L.lda_debug_group_topics_global(1)
    try:
        yield
    finally:
        L.lda_debug_group_topics_global(0)


def _path(G, K, tables=3):
    return capi.load().lda_group_topics_path(G, K, tables, None)


def _last_lds_group_count(K, tables=3):
    """The largest G that lda_group_topics_path puts on the LDS side (0: none)."""
    G = 0
    while _path(G + 1, K, tables) == 1:
        G += 1
    return G


def _same(got, exp, G, K, stats=N.STATS):
    assert set(got) == {*HEAD, *stats}
    for name in HEAD + tuple(stats):
        a, e = got[name], exp[name]
        assert a.dtype == (np.uint64 if name == "shares" else np.int64), name
        assert a.shape == ((G,) if name.startswith("group_") else (G, K)), name
        assert a.tobytes() == e.tobytes(), (name, np.argwhere(a != e)[:5])


def _check(g, c, z, K, groups, G, min_tokens=10, min_count=2, min_prop=0.05, stats=N.STATS):
    got = g.group_topics(groups, G, stats, min_tokens, min_count, min_prop)
    exp = N.expected_group_topics(z, c.doc_off, K, groups, G, min_tokens, min_count, min_prop, stats)
    _same(got, exp, G, K, stats)
    return exp


# ------------------------------------------------------------------- shapes
@pytest.mark.parametrize("K", [4, 20, 64, 65, 300, 4096])
def test_group_topics_against_numpy(K):
    docs = _shape_docs(K, seed=K)
    distinct = max(len(np.unique(d)) for d in docs)
    assert distinct == (min(K, 20) if K < 300 else 299 if K < 4096 else 2500)
    edge = _last_lds_group_count(K)
    assert (edge == 0) == (K == 4096)                 # at Kp = 4096 the histograms alone pass 64 KiB
    Gs = sorted({1, 3, 37, edge, edge + 1} - {0})
    paths = {G: _path(G, K) for G in Gs}
    assert 0 in paths.values() and (1 in paths.values() or K == 4096)
    with _planted_sampler(docs, K) as (g, c, z):
        assert g.z().tobytes() == z.tobytes()
        for G in Gs:
            groups = _groups(len(docs), G, seed=G + K)
            exp = _check(g, c, z, K, groups, G)                        # jsLDA's thresholds
            assert 0 < exp["group_docs"].sum() < len(docs) and exp["present"].any()
            assert np.array_equal(exp["tokens"].sum(axis=1), exp["group_tokens"])
            if G >= 3:
                assert exp["group_docs"][1] == 0 and not exp["tokens"][1].any()
            if G >= 2:
                assert exp["group_docs"][G - 1] == 1 and exp["tokens"][G - 1, K - 1] == 11
                assert exp["shares"][G - 1, K - 1] == 1 << 32
        groups = _groups(len(docs), 3, seed=K)
        all_in = _check(g, c, z, K, groups, 3, 1, 1, 0.0)              # every nonzero topic is present
        assert np.array_equal(all_in["tokens"] > 0, all_in["present"] > 0)
        assert np.array_equal(all_in["tokens"] > 0, all_in["shares"] > 0)
        everybody = _check(g, c, z, K, np.zeros(len(docs), np.int32), 1, 1, 1, 0.0)
        assert everybody["group_tokens"][0] == len(z)
        assert everybody["group_docs"][0] == sum(len(d) > 0 for d in docs) < len(docs)


def test_group_topics_every_subset_of_tables_on_both_paths():
    """A NULL table is neither allocated nor accumulated, and the others do
    not change; the forced global path gives the same bytes."""
    K, G = 20, 3
    docs = _shape_docs(K, seed=3)
    groups = _groups(len(docs), G, seed=5)
    with _planted_sampler(docs, K) as (g, c, z):
        full = N.expected_group_topics(z, c.doc_off, K, groups, G)
        for r in range(3):
            for stats in itertools.combinations(N.STATS, r):
                assert _path(G, K, 1 + len(stats)) == 1
                for ctx in (contextlib.nullcontext(), _global_atomics()):
                    with ctx:
                        got = g.group_topics(groups, G, stats)
                    _same(got, {k: v for k, v in full.items() if k in (*HEAD, *stats)}, G, K, stats)
        got = g.group_topics(groups, G, "shares")                       # a single name
        assert set(got) == {*HEAD, "shares"}
        got = g.group_topics(groups)                                    # G from the ids
        _same(got, full, G, K)


@pytest.mark.parametrize("K,G", [(4, 1), (4, 37), (64, 3)])
def test_group_topics_lds_and_global_paths_agree(K, G):
    assert _path(G, K) == 1
    docs = _shape_docs(K, seed=5 + K)
    groups = _groups(len(docs), G, seed=K + G)
    with _planted_sampler(docs, K) as (g, c, z):
        for thr in ((10, 2, 0.05), (1, 1, 0.0)):
            exp = _check(g, c, z, K, groups, G, *thr)
            with _global_atomics():
                _same(g.group_topics(groups, G, N.STATS, *thr), exp, G, K)


# --------------------------------------------------------------- thresholds
def test_group_topics_thresholds():
    K, G = 20, 3
    docs = _ragged_docs(K, 150, seed=9, max_len=120)
    # counts exactly at min_count = 2, at shares on both sides of 0.05 and 0.25
    docs[0] = np.array([1] * 2 + [2] * 38)         # 2 / 40 = 0.05
    docs[1] = np.array([1] * 2 + [2] * 39)         # just under 0.05
    docs[2] = np.array([1] * 2 + [2] * 37)         # just over 0.05
    docs[3] = np.array([3] * 2 + [4] * 6)          # 2 / 8 = 0.25 exactly
    docs[4] = np.array([3] * 2 + [4] * 7)          # under 0.25
    docs[5] = np.array([3] * 2 + [4] * 5)          # over 0.25
    docs[6] = np.array([5] * 10)                   # share 1.0, ten tokens: at min_tokens = 10
    docs[7] = np.array([5] * 9)                    # nine tokens
    docs[8] = np.array([6] * 1 + [7] * 19)         # a count of 1: under min_count = 2
    docs[9] = np.array([8, 9, 9])                  # L = 3 with n = 1: the share is floor(2^32 / 3)
    longest = max(len(d) for d in docs)
    groups = np.random.default_rng(4).integers(0, 2, len(docs)).astype(np.int32)
    groups[:10] = 2                                # the planted documents are group 2, alone
    settings = 0
    with _planted_sampler(docs, K) as (g, c, z):
        biggest = max(int(np.bincount(d, minlength=K).max()) for d in docs if len(d))
        for min_prop in (0.0, 0.05, 0.25, 1.0):
            for min_count in (1, 2, biggest + 1):
                for min_tokens in (1, 10, longest + 1):
                    exp = _check(g, c, z, K, groups, G, min_tokens, min_count, min_prop)
                    settings += 1
                    if min_tokens > longest:
                        assert not any(v.any() for v in exp.values())
                    elif min_count > biggest:
                        assert exp["group_docs"].all() and not exp["present"].any() and exp["shares"].any()
        assert settings >= 12
        a = N.expected_group_topics(z, c.doc_off, K, groups, G, 1, 2, 0.05)
        b = N.expected_group_topics(z, c.doc_off, K, groups, G, 1, 2, 0.25)
        assert (a["present"][2, 1], a["present"][2, 3], b["present"][2, 1], b["present"][2, 3]) == (2, 3, 0, 2)
        assert a["shares"][2, 8] == (1 << 32) // 3 and a["shares"][2, 9] == (2 << 32) // 3
        # ten tokens or more: documents 0, 1, 2, 6 and 8
        assert a["group_docs"][2] == 10 and N.expected_group_topics(z, c.doc_off, K, groups, G)["group_docs"][2] == 5


# -------------------------------------------------------------- 64-bit cells
def test_group_topics_share_cells_above_2_to_the_32():
    """Two one-topic documents in one group: 2^32 each."""
    K = 4
    docs = [np.full(12, 1), np.full(30, 1), np.array([0, 0, 1] * 4), np.full(15, 3)]
    groups = np.array([0, 0, 0, 1], np.int32)
    with _planted_sampler(docs, K) as (g, c, z):
        exp = _check(g, c, z, K, groups, 2)
        assert exp["shares"][0, 1] == (2 << 32) + (4 << 32) // 12 > 2 ** 33 and exp["shares"][1, 3] == 1 << 32
        with _global_atomics():
            _same(g.group_topics(groups, 2), exp, 2, K)


# ---------------------------------------------------------------- second trip
def _second_trip_docs(K):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P = 32 * cus                                    # 8 blocks per CU, four one-document waves each
    D = 64 * cus + 37
    assert D == 2 * P + 37 and (D + 3) // 4 > 8 * cus          # the grid is capped: the waves loop
    rng = np.random.default_rng(8)
    docs = [rng.integers(0, K, int(n)).astype(np.int32) for n in rng.integers(1, 4, D)]
    long_doc = lambda: rng.integers(0, K, 150).astype(np.int32)
    # a long, an empty and a one-token document a trip apart: the first wave and
    # wave 36, the last one with a third trip; a middle wave has two trips
    for w in (0, 36):
        docs[w], docs[P + w], docs[2 * P + w] = long_doc(), np.zeros(0, np.int32), np.array([w % K], np.int32)
    docs[P // 2 + 1], docs[P + P // 2 + 1] = long_doc(), np.zeros(0, np.int32)
    docs[P - 1], docs[2 * P - 1] = np.array([3], np.int32), long_doc()      # the last wave of a trip
    for w in (1, 35):
        docs[w], docs[P + w], docs[2 * P + w] = np.zeros(0, np.int32), long_doc(), long_doc()
    return docs, P


def test_grid_cap_group_topics_second_trip():
    K, G = 4, 3
    docs, P = _second_trip_docs(K)
    D = len(docs)
    groups = np.random.default_rng(3).integers(-1, G, D).astype(np.int32)
    for w in (0, 1, 35, 36):
        groups[[w, P + w, 2 * P + w]] = (0, 1, 2)
    with _planted_sampler(docs, K) as (g, c, z):
        assert g.D == D
        exp = _check(g, c, z, K, groups, G, 1, 1, 0.0)
        _check(g, c, z, K, groups, G)
        # the third trip's documents alone change the result
        cut = groups.copy()
        cut[2 * P:] = -1
        short = N.expected_group_topics(z, c.doc_off, K, cut, G, 1, 1, 0.0)
        assert short["group_docs"].sum() < exp["group_docs"].sum()
        assert short["shares"].tobytes() != exp["shares"].tobytes()
        with _global_atomics():
            _same(g.group_topics(groups, G, N.STATS, 1, 1, 0.0), exp, G, K)


def test_grid_cap_subcorpus_count_second_trip():
    K = 4
    docs, P = _second_trip_docs(K)
    D = len(docs)
    mask = (np.random.default_rng(5).random(D) < 0.5).astype(np.uint8)
    mask[[0, 36, 2 * P, 2 * P + 1, 2 * P + 35, 2 * P + 36, D - 1]] = 1
    mask[[1, P + 36]] = 0
    with _planted_sampler(docs, K) as (g, c, z):
        g.subcorpus_count(mask)
        want = N.table_top_words(N.subcorpus_table(z, c.words, c.doc_off, V, K, mask), V)
        _same_words(g.subcorpus_top_words(V), want)
        cut = mask.copy()
        cut[2 * P:] = 0
        assert N.subcorpus_table(z, c.words, c.doc_off, V, K, cut).sum() < want[2].sum()


# -------------------------------------------------------------- sub-corpus
def _same_words(got, want):
    for a, e, dt in zip(got, want, (np.int32, np.int32, np.int64)):
        assert a.dtype == dt and a.shape == e.shape
        assert a.tobytes() == e.tobytes(), np.argwhere(a != e)[:5]


def test_subcorpus_whole_table_accumulate_and_release():
    """V = 50 with n = 50: every nonzero cell of the table is compared."""
    K = 20
    docs = _ragged_docs(K, 200, seed=2, max_len=80)
    docs[-1] = np.array([K - 1] * 7 + [0] * 3, np.int32)
    D = len(docs)
    rng = np.random.default_rng(6)
    A = (rng.random(D) < 0.3).astype(np.uint8)
    B = ((rng.random(D) < 0.4) & (A == 0)).astype(np.uint8)
    last = np.zeros(D, np.uint8)
    last[-1] = 1                                                       # the shard's last document alone
    with _planted_sampler(docs, K) as (g, c, z):
        table = lambda m: N.subcorpus_table(z, c.words, c.doc_off, V, K, m)
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*without a table") as e:
            g.subcorpus_top_words(5)                                   # before any count
        assert e.value.status == -4
        g.subcorpus_release()                                          # nothing to release
        g.subcorpus_count(A)
        _same_words(g.subcorpus_top_words(V), N.table_top_words(table(A), V))
        g.subcorpus_count(B, accumulate=True)                          # A then B = A | B for disjoint masks
        union = N.table_top_words(table(A | B), V)
        assert union[2].sum() == table(A).sum() + table(B).sum()
        _same_words(g.subcorpus_top_words(V), union)
        g.subcorpus_count(B)                                           # without accumulate the table starts over
        _same_words(g.subcorpus_top_words(V), N.table_top_words(table(B), V))
        g.subcorpus_count(last)
        ids, cnt, tot = g.subcorpus_top_words(3)
        _same_words((ids, cnt, tot), N.table_top_words(table(last), 3))
        assert tot[K - 1] == 7 and tot[0] == 3 and tot.sum() == 10
        # all ones equals top_words(n) of the same context: the new route against an existing readout
        g.subcorpus_count(np.ones(D, np.uint8))
        for n in (1, 10, capi.TOP_WORDS_MAX):
            ids, cnt, tot = g.subcorpus_top_words(n)
            tw_ids, tw_cnt = g.top_words(n)
            assert ids.tobytes() == tw_ids.tobytes() and cnt.tobytes() == tw_cnt.tobytes()
            assert tot.tolist() == np.bincount(z, minlength=K).tolist()
        # all zeros gives -1 / 0
        g.subcorpus_count(np.zeros(D, np.uint8))
        ids, cnt, tot = g.subcorpus_top_words(4)
        assert np.all(ids == -1) and not cnt.any() and not tot.any()
        # release, then accumulate into a fresh table: it starts from zero
        g.subcorpus_release()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*without a table"):
            g.subcorpus_top_words(5)
        g.subcorpus_count(A, accumulate=True)
        _same_words(g.subcorpus_top_words(V), N.table_top_words(table(A), V))


@pytest.mark.parametrize("K", [20, 300])
def test_subcorpus_top_words_with_ties(K):
    """V = 300, n = 10: few tokens per cell, so equal counts meet in every list."""
    nv = 300
    docs = _ragged_docs(K, 300, seed=12, max_len=60)
    mask = (np.random.default_rng(1).random(len(docs)) < 0.6).astype(np.uint8)
    with _planted_sampler(docs, K, num_types=nv, word_seed=3) as (g, c, z):
        g.subcorpus_count(mask)
        want = N.table_top_words(N.subcorpus_table(z, c.words, c.doc_off, nv, K, mask), 10)
        ties = (want[1][:, :-1] == want[1][:, 1:]) & (want[1][:, 1:] > 0)
        assert ties.sum() >= K                                          # the order by word id is exercised
        _same_words(g.subcorpus_top_words(10), want)


def _half_samplers(docs, K, cut):
    """Two contexts over documents [0, cut) and [cut, D) of one planted corpus."""
    from ldagibbssampling_amd.sampler import GibbsSampler
    c, z = _planted(docs)
    t = int(c.doc_off[cut])
    parts = [(c.doc_off[:cut + 1], c.words[:t], z[:t]), (c.doc_off[cut:] - t, c.words[t:], z[t:])]
    mk = lambda p, dev: GibbsSampler(K, V, p[0], p[1], np.full(K, 0.3), 0.05, seed=5, device=dev)
    return c, z, parts, mk


def _merge_check(dev_b):
    K = 20
    docs = _ragged_docs(K, 120, seed=7, max_len=70)
    cut = 70
    c, z, parts, mk = _half_samplers(docs, K, cut)
    mask = (np.random.default_rng(9).random(len(docs)) < 0.5).astype(np.uint8)
    with mk(parts[0], 0) as a, mk(parts[1], dev_b) as b:
        for s, p in ((a, parts[0]), (b, parts[1])):
            s.set_z(p[2])
            s.apply()
        a.subcorpus_count(mask[:cut])
        b.subcorpus_count(mask[cut:])
        own_b = b.subcorpus_top_words(V)
        a.subcorpus_merge(b)
        _same_words(a.subcorpus_top_words(V), N.table_top_words(N.subcorpus_table(z, c.words, c.doc_off, V, K, mask), V))
        _same_words(b.subcorpus_top_words(V), own_b)                   # from is unchanged
        _same_words(own_b, N.table_top_words(N.subcorpus_table(parts[1][2], parts[1][1], parts[1][0], V, K,
                                                               mask[cut:]), V))
        return a, b


def test_subcorpus_merge_of_two_shards_equals_one_table():
    _merge_check(0)
    K = 20
    docs = _ragged_docs(K, 30, seed=1, max_len=30)
    with _planted_sampler(docs, K) as (a, _, _), _planted_sampler(docs, K + 1) as (b, _, _), \
            _planted_sampler(docs, K) as (d, _, _):
        ones = np.ones(len(docs), np.uint8)
        a.subcorpus_count(ones)
        b.subcorpus_count(ones)
        with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*differ in V or K"):
            a.subcorpus_merge(b)
        with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*into itself"):
            a.subcorpus_merge(a)
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*without a table"):
            a.subcorpus_merge(d)                                        # from has no table
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*without a table"):
            d.subcorpus_merge(a)
        assert a._L.lda_subcorpus_merge(a._h, None) == -1 and b"null from" in a._L.lda_last_error()
        d.subcorpus_count(ones)
        a.subcorpus_merge(d)                                            # twice the table
        ids, cnt, tot = a.subcorpus_top_words(5)
        one = d.subcorpus_top_words(5)
        assert ids.tobytes() == one[0].tobytes() and np.array_equal(cnt, 2 * one[1]) and np.array_equal(tot, 2 * one[2])


def test_subcorpus_merge_between_two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible: the peer-copy merge needs two")
    _merge_check(1)


# -------------------------------------------------------------- model level
def _model(corpus, K, devices=None, iters=4):
    from ldagibbssampling_amd import topic_model as tm
    m = tm.ParallelTopicModel(K, 0.5 * K, 0.01)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(iters)
    m.setOptimizeInterval(0)
    if devices is not None:
        m.setDevices(devices)
    m.addInstances(tm.InstanceList.fromCorpus(corpus))
    m.estimate()
    return m


def test_model_group_topics_and_subcorpus_words_on_one_two_and_three_shards(tmp_path):
    from ldagibbssampling_amd import topic_model as tm
    K, G = 20, 4
    c, _ = _planted(_ragged_docs(K, 300, seed=4, max_len=60))
    D = c.num_docs
    rng = np.random.default_rng(2)
    labels = ["d", "a", None, "c"]                                      # "b" is nobody's: three groups, by name
    names = [labels[i] for i in rng.integers(0, 4, D)]
    groups = rng.integers(-1, G, D).astype(np.int32)
    groups[groups == 2] = 3                                             # an empty group
    mask = (rng.random(D) < 0.4).astype(np.uint8)
    for devices in ([0], [0, 0], [0, 0, 0]):
        m = _model(c, K, devices)
        assert m.numShards() == len(devices)
        z = m.topicAssignments()
        for thr in ((10, 2, 0.05), (1, 1, 0.0), (5, 3, 0.25)):
            exp = N.expected_group_topics(z, c.doc_off, K, groups, G, *thr)       # the whole corpus
            _same(m.groupTopics(groups, G, N.STATS, *thr), exp, G, K)
            _same(m.groupTopics(groups, G, ("shares",), *thr), {k: v for k, v in exp.items() if k != "present"},
                  G, K, ("shares",))
        lab, ids = tm.group_labels(names)
        assert lab == ["a", "c", "d"]
        exp = N.expected_group_topics(z, c.doc_off, K, ids, 3)
        for kind in N.KINDS:
            r = m.topicsByGroup(names, kind)
            want = N.finish(kind, exp["group_docs"], exp["group_tokens"], exp["tokens"], exp["present"], exp["shares"])
            assert r.labels == lab and N.same_floats(r.values, want), kind
            assert r.groupDocs.tobytes() == exp["group_docs"].tobytes()
            assert r.groupTokens.tobytes() == exp["group_tokens"].tobytes()
            assert r.counts["tokens"].tobytes() == exp["tokens"].tobytes()
            wi, wv = N.top_topics(want, 3)
            assert m.getGroupTopTopics(3, names, kind) == \
                {l: [(int(t), float(v)) for t, v in zip(wi[g], wv[g]) if t >= 0] for g, l in enumerate(lab)}
            text = tm.format_group_topics(wi, wv)
            assert m.groupTopicsText(3, kind, names) == text and text.startswith("#group topic value\n0 ")
            path = tmp_path / "group_topics.txt"
            m.printGroupTopics(path, 3, kind, names)
            assert path.read_text() == text
        want = N.table_top_words(N.subcorpus_table(z, c.words, c.doc_off, V, K, mask), 10)
        _same_words(m.subCorpusTopWords(mask, 10), want)
        name = m.alphabet.lookupObject
        assert m.getSubCorpusTopWords(mask, 10) == \
            [[(name(int(w)), int(n)) for w, n in zip(want[0][k], want[1][k]) if w >= 0] for k in range(K)]
        assert m.getGroupTopWords("c", 10, names) == m.getSubCorpusTopWords(ids == 1, 10)
        _same_words(m.subCorpusTopWords(np.ones(D), 10)[:2], m.topWords(10))      # everybody: the model's top words
        m.close()


# --------------------------------------------------------- state and errors
def test_group_topics_state_and_errors():
    K, G = 20, 3
    docs = _ragged_docs(K, 12, seed=1, max_len=40)
    from ldagibbssampling_amd.sampler import GibbsSampler
    c, z = _planted(docs)
    groups = np.array([0, 1, 2] * 4, np.int32)
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=3) as g:
        # lda_create leaves the shard's counts as the pending delta
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
            g.group_topics(groups)
        assert e.value.status == -4
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.subcorpus_count(np.ones(12))
        g.sweep(1)
        out = np.zeros(G * K, np.int64)
        p, gp = out.ctypes.data, groups.ctypes.data
        call, err = g._L.lda_group_topics, g._L.lda_last_error
        for bad in (0, -1):
            assert call(g._h, gp, bad, 10, 2, 0.05, p, p, p, p, p) == -1 and b"G must be" in err()
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            assert call(g._h, gp, G, 10, 2, 0.05, *args, p, p) == -1 and b"null output" in err()
        for mt in (0, -2):
            assert call(g._h, gp, G, mt, 2, 0.05, p, p, p, p, p) == -1 and b"min_tokens" in err()
        for mc in (0, -2):
            assert call(g._h, gp, G, 10, mc, 0.05, p, p, p, p, p) == -1 and b"min_count" in err()
        for mp in (-1e-9, 1.0 + 1e-9, math.nan, math.inf, -math.inf):
            assert call(g._h, gp, G, 10, 2, mp, p, p, p, p, p) == -1 and b"min_prop" in err()
        assert call(g._h, None, G, 10, 2, 0.05, p, p, p, p, p) == -1 and b"null doc_group" in err()
        for at, v in ((11, 3), (4, -2)):
            bad = groups.copy()
            bad[at] = v
            bad[11] = 3                                                 # the first offender is named
            assert call(g._h, bad.ctypes.data, G, 10, 2, 0.05, p, p, p, p, p) == -1
            assert (b"doc_group[%d] = %d is outside" % (at, v)) in err()
        big = (capi.GROUP_TOPICS_MAX_CELLS // K) + 1
        wide = np.zeros(12, np.int32)
        assert call(g._h, wide.ctypes.data, big, 10, 2, 0.05, p, p, p, None, None) == -5 and b"MAX_CELLS" in err()
        assert g._L.lda_subcorpus_count(g._h, None, 0) == -1 and b"null doc_mask" in err()
        ip = np.zeros(K * 3, np.int32).ctypes.data
        for n in (0, capi.TOP_WORDS_MAX + 1):
            assert g._L.lda_subcorpus_top_words(g._h, n, ip, ip, p) == -1 and b"n must be" in err()
        assert g._L.lda_subcorpus_top_words(g._h, 3, ip, ip, None) == -1 and b"null output" in err()
        assert not out.any()                                            # nothing was written
        g.subcorpus_count(np.ones(12))
        g.sample()                                                      # a pending delta again
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.group_topics(groups)
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.subcorpus_count(np.ones(12), accumulate=True)
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.subcorpus_top_words(3)
        with _planted_sampler(docs, K) as (other, _, _):
            other.subcorpus_count(np.ones(12))
            with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
                g.subcorpus_merge(other)
            with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
                other.subcorpus_merge(g)
        g.apply()
        _check(g, c, g.z(), K, groups, G)
        g.subcorpus_release()


@pytest.mark.parametrize("D", [0, 3])
def test_group_topics_without_documents_or_tokens(D):
    K, G = 20, 3
    with _planted_sampler([np.zeros(0, np.int32)] * D, K) as (g, _, _):
        got = g.group_topics(np.zeros(D, np.int32), G, min_tokens=1)
        assert not any(got[s].any() for s in HEAD + N.STATS) and got["shares"].shape == (G, K)
        g.subcorpus_count(np.ones(D, np.uint8))
        ids, cnt, tot = g.subcorpus_top_words(3)
        assert np.all(ids == -1) and not cnt.any() and not tot.any()


def test_group_topics_and_subcorpus_change_no_state():
    K, G = 100, 5
    from ldagibbssampling_amd.sampler import GibbsSampler
    c, _ = _planted(_ragged_docs(K, 300, seed=6, max_len=60))
    groups = _groups(c.num_docs, G, seed=2)
    mask = (groups >= 2).astype(np.uint8)
    mk = lambda: GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=21)
    with mk() as g, mk() as ref, mk() as other:
        for s in (g, ref, other):
            s.sweep(2)
        z, before, sweeps = g.z(), g.counts_checksum(), g.sweep_index
        assert before == ref.counts_checksum() and sweeps == ref.sweep_index
        a = g.group_topics(groups, G)
        b = g.group_topics(groups, G)
        with _global_atomics():
            g.group_topics(groups, G)
        _same(a, N.expected_group_topics(z, c.doc_off, K, groups, G), G, K)
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)
        g.subcorpus_count(mask)
        other.subcorpus_count(mask)
        g.subcorpus_merge(other)
        first = g.subcorpus_top_words(8)
        assert np.array_equal(first[2], 2 * other.subcorpus_top_words(8)[2])
        assert g.z().tobytes() == z.tobytes() and g.counts_checksum() == before and g.sweep_index == sweeps
        g.sweep(5)
        ref.sweep(5)
        assert g.z().tobytes() == ref.z().tobytes() and g.counts_checksum() == ref.counts_checksum()
        assert g.sweep_index == ref.sweep_index
        # the table is a snapshot: five sweeps later it still holds the old z's counts
        _same_words(g.subcorpus_top_words(8), first)
        g.subcorpus_release()
