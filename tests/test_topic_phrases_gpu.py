"""GPU checks of the topic phrases: lda_topic_phrases (k_phrase_scan,
k_phrase_insert, k_phrase_hist, k_phrase_thresh, k_phrase_scatter,
k_phrase_select, k_phrase_gather), lda_phrase_counts / lda_phrase_lookup
(k_phrase_lookup), the ldatm_ mirror and printTopicPhrases' text.

Every expectation is the brute-force restatement (topic_phrases_numpy) on z()
of the same context: a Python loop over the runs and a dictionary.  Everything
compared is an integer array and is compared exactly; no tolerance appears
anywhere.

Geometry.  Every pass over the runs gives a wave a document and a lane a token
and caps its grid at 8 blocks of 4 waves per CU, P = 32 x CUs documents a trip;
the second-trip test holds 2 P + 37 documents.  A document longer than 64
tokens takes several trips of its wave: the lengths 64, 65 and 150 are in every
shape.  The table has the smallest power of two of slots >= 2 N / min_len, at
least 1024; the test hook sets it, and a table of 64 slots takes at least
ceil(runs / 32) passes, since a pass inserts at most 32 runs (half the slots)
unless one of the 4096 hash parts alone holds more."""
import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

import topic_phrases_numpy as N

pytestmark = pytest.mark.gpu

LIMITS = [(2, 32), (2, 2), (3, 5)]


# ------------------------------------------------------------------ helpers
def _corpus(lengths, seed, num_types):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    words = rng.integers(0, num_types, int(off[-1])).astype(np.int32)
    return Corpus(off, words, num_types)


def _lengths(seed, n):
    """test_topic_docs_gpu's lengths: an empty document, a one-token one, one
    wave's 64 lanes, 65, several trips, among ordinary ones, shuffled (fewer
    than five documents: the first n of the ordinary ones)."""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 64, 65, 150] if n >= 5 else []
    lens = np.array(fixed + rng.integers(2, 40, n - len(fixed)).tolist(), np.int64)
    rng.shuffle(lens)
    return lens


def _sampler(c, K, seed=11):
    from ldagibbssampling_amd.sampler import GibbsSampler
    return GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=seed,
                        sampler="sparse" if K > capi.MAX_TOPICS_DENSE else "dense")


class _Expect:
    """The restatement of one (corpus, z), its tables kept per (min_len, max_len)."""

    def __init__(self, c, z, K):
        self.c, self.z, self.K, self.tables = c, np.array(z), K, {}

    def table(self, lo, hi):
        if (lo, hi) not in self.tables:
            self.tables[lo, hi] = N.phrase_table(self.c.words, self.z, self.c.doc_off, lo, hi)
        return self.tables[lo, hi]

    def arrays(self, n, lo, hi, min_count):
        table, skipped = self.table(lo, hi)
        w = np.full((self.K, n, hi), -1, np.int32)
        lens = np.zeros((self.K, n), np.int32)
        cnt = np.zeros((self.K, n), np.int64)
        first = np.full((self.K, n), -1, np.int64)
        runs = np.zeros(self.K, np.int64)
        distinct = np.zeros(self.K, np.int64)
        for (k, _), (c, _) in table.items():
            runs[k] += c
            distinct[k] += 1
        for k, lst in enumerate(N.ranked(table, self.K, min_count)):
            for i, (ph, c, f) in enumerate(lst[:n]):
                w[k, i, :len(ph)] = ph
                lens[k, i], cnt[k, i], first[k, i] = len(ph), c, f
        return w, lens, cnt, first, runs, distinct, skipped


def _same(got, exp):
    for a, e in zip(got[:6], exp[:6]):
        assert a.dtype == e.dtype and a.shape == e.shape
        np.testing.assert_array_equal(a, e)
    assert got[6] == exp[6]


def _check(g, ex, n, lo, hi, min_count):
    exp = ex.arrays(n, lo, hi, min_count)
    _same(g.topic_phrases(n, lo, hi, min_count), exp)
    return exp


def _bytes(res):
    return b"".join(a.tobytes() for a in res[:6]) + str(res[6]).encode()


def test_restatement_arrays_agree():
    """_Expect.arrays is topic_phrases_numpy.expected_topic_phrases with the table kept."""
    c = _corpus(_lengths(3, 40), 4, 5)
    z = np.random.default_rng(5).integers(0, 4, c.num_tokens).astype(np.int32)
    ex = _Expect(c, z, 4)
    for n, (lo, hi), mc in ((10, (2, 32), 1), (128, (3, 5), 2)):
        e = N.expected_topic_phrases(c.words, z, c.doc_off, 4, n, lo, hi, mc)
        assert _bytes(ex.arrays(n, lo, hi, mc)) == _bytes(e)


# ------------------------------------------------------------------- shapes
@pytest.mark.parametrize("V", [5, 50])
@pytest.mark.parametrize("D", [1, 7, 300, 3001])
@pytest.mark.parametrize("K", [4, 20, 500, 4096])
def test_topic_phrases_against_the_restatement(K, D, V):
    c = _corpus(_lengths(K + D, D), 5 + V, V)
    seen = dict(counted=False, tie=False, padded=False, skipped=False)
    with _sampler(c, K, seed=K * 7 + D) as g:
        g.apply()                               # lda_create leaves the counts pending: the random start
        ex = _Expect(c, g.z(), K)
        for lo, hi in LIMITS:
            for mc in (1, 2):
                _check(g, ex, 10, lo, hi, mc)
        g.sweep(3)
        ex = _Expect(c, g.z(), K)
        for n in (1, 10, 128):
            for lo, hi in LIMITS:
                for mc in (1, 2):
                    w, lens, cnt, first, runs, distinct, skipped = _check(g, ex, n, lo, hi, mc)
                    seen["counted"] |= bool(np.any(cnt > 1))
                    seen["tie"] |= N.content_tie(lens, cnt)
                    seen["padded"] |= bool(np.any(lens == 0))
                    seen["skipped"] |= skipped > 0
                    assert np.all(w[lens == 0] == -1) and np.all(first[lens == 0] == -1)
        again = g.topic_phrases(128, 3, 5, 2)
        assert _bytes(again) == _bytes(ex.arrays(128, 3, 5, 2))
    # a case that loses its point fails loudly
    assert seen["padded"], "no padded slot was compared"
    if D >= 300 and K <= 20:
        assert seen["tie"], "no two neighbours of a list share a count: the content order decided nothing"
    if D >= 300 and V == 5 and K <= 20:
        assert seen["counted"], "no phrase was counted more than once"
        assert seen["skipped"], "no run was longer than max_len"


# ------------------------------------------------------------ crafted z
def _crafted(K, lens, words, z, num_types, cases):
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    c = Corpus(off, np.asarray(words, np.int32), num_types)
    z = np.asarray(z, np.int32)
    out = []
    with _sampler(c, K) as g:
        g.set_z(z)
        g.apply()
        assert g.z().tobytes() == z.tobytes()
        ex = _Expect(c, z, K)
        for n, lo, hi, mc in cases:
            out.append(_check(g, ex, n, lo, hi, mc))
    return out


def test_one_topic_through_documents_of_64_65_and_150_tokens():
    """Every document is one run longer than max_len, across the wave's trips:
    three skipped_long, no phrase, no run."""
    lens = [64, 65, 150]
    words = np.arange(sum(lens)) % 7
    for lo, hi in LIMITS:
        (res,) = _crafted(4, lens, words, np.full(sum(lens), 2), 7, [(10, lo, hi, 1)])
        assert res[6] == 3 and not res[1].any() and not res[4].any() and not res[5].any()


def test_runs_that_straddle_the_wave_trip():
    """A 150-token document of alternating topics 2 3 2 3 ... with topic 1 on
    tokens [60, 68) and [126, 130): both runs cross a multiple of 64."""
    z = np.tile([2, 3], 75)
    z[60:68] = 1
    z[126:130] = 1
    words = np.arange(150) % 11
    (res,) = _crafted(4, [150], words, z, 11, [(10, 2, 32, 1)])
    w, lens, cnt, first, runs, distinct, skipped = res
    assert runs.tolist() == [0, 2, 0, 0] and distinct.tolist() == [0, 2, 0, 0] and skipped == 0
    assert sorted(zip(first[1, :2].tolist(), lens[1, :2].tolist())) == [(60, 8), (126, 4)]
    assert w[1][lens[1] == 8][0, :8].tolist() == words[60:68].tolist()


def test_a_document_of_exactly_max_len_tokens_counts():
    for hi in (32, 5, 2):
        lens = [hi, hi + 1, hi]
        words = np.concatenate([np.arange(hi), np.arange(hi + 1), np.arange(hi)])
        (res,) = _crafted(4, lens, words, np.full(3 * hi + 1, 3), 40, [(10, 2, hi, 1)])
        w, plens, cnt, first, runs, distinct, skipped = res
        assert plens[3, 0] == hi and cnt[3, 0] == 2 and first[3, 0] == 0 and skipped == 1
        assert runs.tolist() == [0, 0, 0, 2] and distinct.tolist() == [0, 0, 0, 1]
        assert w[3, 0].tolist() == list(range(hi))


def test_alternating_topics_give_no_run():
    lens = [1, 64, 0, 65, 150, 7]
    n = sum(lens)
    for res in _crafted(4, lens, np.arange(n) % 3, np.arange(n) % 2, 3, [(10, 2, 32, 1), (128, 2, 2, 1)]):
        assert not res[1].any() and not res[2].any() and np.all(res[3] == -1) and np.all(res[0] == -1)
        assert not res[4].any() and not res[5].any() and res[6] == 0


def test_runs_do_not_join_across_a_document_boundary():
    """d0 ends and d1 starts in topic 1 with the words 1 2 | 1 2: two runs of
    (1 2), never one of (1 2 1 2); an empty document between d1 and d2 changes
    nothing; d2's single token of topic 1 next to d1's last run joins nothing."""
    lens = [5, 6, 0, 1, 3]
    words = [1, 2, 3, 1, 2, 1, 2, 4, 4, 1, 2, 1, 1, 2, 3]
    z = [0, 0, 0, 1, 1, 1, 1, 2, 2, 1, 1, 1, 0, 0, 0]
    (res,) = _crafted(4, lens, words, z, 6, [(10, 2, 32, 1)])
    w, plens, cnt, first, runs, distinct, skipped = res
    assert w[1, 0, :3].tolist() == [1, 2, -1] and cnt[1, 0] == 3 and first[1, 0] == 3 and plens[1, 1] == 0
    assert w[0, 0, :4].tolist() == [1, 2, 3, -1] and cnt[0, 0] == 2 and first[0, 0] == 0
    assert runs.tolist() == [2, 3, 1, 0]


def test_topic_k_minus_1_at_k_4096_with_the_longest_phrase():
    """Topic 4095 and length 32 are all ones in the key's topic and length
    fields: only the start tells such a key from an empty slot."""
    K = 4096
    lens = [32, 32, 3, 40]
    words = np.concatenate([np.arange(32), np.arange(32), [5, 6, 7], np.arange(40)])
    z = np.concatenate([np.full(67, K - 1), np.tile([0, K - 1], 20)])
    res = _crafted(K, lens, words, z, 64, [(10, 2, 32, 1), (128, 2, 32, 2), (1, 3, 5, 1)])
    w, plens, cnt, first, runs, distinct, skipped = res[0]
    assert plens[K - 1, :3].tolist() == [32, 3, 0] and cnt[K - 1, :2].tolist() == [2, 1]
    assert first[K - 1, :2].tolist() == [0, 64] and runs[K - 1] == 3 and not runs[:K - 1].any()
    assert res[1][2][K - 1].tolist() == [2] + [0] * 127
    assert res[2][1][K - 1, 0] == 3 and res[2][6] == 2      # (3, 5): the two 32-runs are too long


# ----------------------------------------------------------- contention
def test_three_thousand_identical_documents_meet_in_one_slot():
    """One phrase, count 3000, first 0: the claim, the add and the minimum on
    one slot from every wave of the grid."""
    D = 3000
    words = np.tile([3, 1, 4, 1], D)
    z = np.tile([1, 1, 1, 1], D)
    res = _crafted(4, [4] * D, words, z, 5, [(10, 2, 32, 1), (1, 2, 32, 2), (10, 3, 5, 3000), (10, 3, 5, 3001)])
    for r in res[:3]:
        assert r[0][1, 0, :4].tolist() == [3, 1, 4, 1] and r[1][1, 0] == 4 and r[2][1, 0] == D and r[3][1, 0] == 0
        assert r[4].tolist() == [0, D, 0, 0] and r[5].tolist() == [0, 1, 0, 0] and r[2].sum() == D
    assert not res[3][2].any() and res[3][4][1] == D


# --------------------------------------------------------------- passes
def test_small_tables_take_many_passes_and_give_the_default_arrays():
    K, D = 4, 300                               # few topics: many runs at every pair of limits
    c = _corpus(_lengths(K + D, D), 55, 50)
    L = capi.load()
    with _sampler(c, K) as g:
        g.sweep(3)
        ex = _Expect(c, g.z(), K)
        cases = ((10, 2, 32, 1), (128, 2, 32, 1), (128, 3, 5, 1), (10, 2, 2, 2))
        base = [_check(g, ex, *case) for case in cases]
        # a pass inserts at most 32 of these runs into 64 slots: at least 8 passes
        for b in base:
            assert -(-int(b[4].sum()) // 32) >= 8, "too few runs for 8 passes of a 64-slot table"
        assert max(len(ph) for _, ph in ex.table(2, 32)[0]) <= 32 < int(base[0][5].sum())
        queries = [(k, ph) for (k, ph) in list(ex.table(2, 32)[0])[:200]]
        qt, qp = [k for k, _ in queries], [ph for _, ph in queries]
        counts = g.phrase_counts(qt, qp, with_first=True)
        assert counts[0].tolist() == [ex.table(2, 32)[0][q][0] for q in queries]
        assert counts[1].tolist() == [ex.table(2, 32)[0][q][1] for q in queries]
        try:
            # 2^21 slots: the table passes (hist, scatter) take four trips of their capped grid
            for slots in (64, 256, 4096, 1 << 21):
                L.lda_debug_phrase_table_slots(slots)
                for case, exp in zip(cases, base):
                    got = g.topic_phrases(*case)
                    assert _bytes(got) == _bytes(exp), (slots, case)
                    assert _bytes(g.topic_phrases(*case)) == _bytes(got), (slots, case)
                again = g.phrase_counts(qt, qp, with_first=True)
                assert again[0].tobytes() == counts[0].tobytes() and again[1].tobytes() == counts[1].tobytes()
        finally:
            L.lda_debug_phrase_table_slots(0)
        for case, exp in zip(cases, base):
            assert _bytes(g.topic_phrases(*case)) == _bytes(exp)


# ------------------------------------------------------------- grid cap
def test_grid_cap_phrase_scan_second_trip():
    import torch
    P = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    K, D = 4, 2 * P + 37
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 4, D).astype(np.int64)
    lens[[5, P + 5, 2 * P + 5]] = (150, 0, 1)           # a long, an empty and a one-token document a trip apart
    lens[[6, P + 6, 2 * P + 6]] = 12
    c = _corpus(lens, 9, 5)
    z = rng.integers(0, K, c.num_tokens).astype(np.int32)
    marks = []
    for d, k in ((6, 1), (P + 6, 2), (2 * P + 6, 3)):        # one 12-token run of its own in each trip
        s = int(c.doc_off[d])
        z[s:s + 12] = k
        c.words[s:s + 12] = [4, 4, 4, 4, 0, 4, 4, 4, 4, 1, 4, 4]
        marks.append((k, s))
    with _sampler(c, K) as g:
        g.set_z(z)
        g.apply()
        ex = _Expect(c, z, K)
        for n, lo, hi, mc in ((10, 2, 32, 1), (128, 2, 2, 1), (128, 3, 5, 2)):
            _check(g, ex, n, lo, hi, mc)
        ph = [4, 4, 4, 4, 0, 4, 4, 4, 4, 1, 4, 4]
        cnt, first = g.phrase_counts([k for k, _ in marks], [ph] * 3, with_first=True)
        assert cnt.tolist() == [1, 1, 1] and first.tolist() == [s for _, s in marks]
        assert marks[1][1] >= c.doc_off[P] and marks[2][1] >= c.doc_off[2 * P]


# --------------------------------------------------------------- lookup
def test_phrase_counts_of_reported_absent_wrong_topic_and_too_long_queries():
    K, D = 20, 300
    c = _corpus(_lengths(K + D, D), 10, 5)
    with _sampler(c, K) as g:
        g.sweep(3)
        ex = _Expect(c, g.z(), K)
        for lo, hi in LIMITS:
            table, _ = ex.table(lo, hi)
            w, lens, cnt, first, *_ = _check(g, ex, 128, lo, hi, 1)
            topics = [k for k in range(K) for i in range(128) if lens[k, i] > 0]
            phrases = [tuple(w[k, i, :lens[k, i]].tolist()) for k in range(K) for i in range(128) if lens[k, i] > 0]
            assert len(topics) > 100
            got, gfirst = g.phrase_counts(topics, phrases, lo, hi, with_first=True)
            assert got.tolist() == cnt[lens > 0].tolist() and gfirst.tolist() == first[lens > 0].tolist()
            assert g.phrase_counts(topics, phrases, lo, hi).tobytes() == got.tobytes()
            # the same words under the next topic, and with the last word changed
            wrong = [(k + 1) % K for k in topics]
            other = [ph[:-1] + ((ph[-1] + 1) % 5,) for ph in phrases]
            for qt, qp in ((wrong, phrases), (topics, other)):
                e = [table.get((k, ph), [0, -1]) for k, ph in zip(qt, qp)]
                got, gfirst = g.phrase_counts(qt, qp, lo, hi, with_first=True)
                assert got.tolist() == [x[0] for x in e] and gfirst.tolist() == [x[1] for x in e]
                if hi > 2:      # (2, 2) at V = 5 has 25 word pairs: a changed one may well exist
                    assert 0 in got.tolist(), "every changed query is still a phrase of the corpus"
        # lengths outside the limits count 0 whatever the corpus holds
        table, _ = ex.table(2, 32)
        (k2, p2), = [(k, ph) for (k, ph) in table if len(ph) == 2][:1]
        (k4, p4), = [(k, ph) for (k, ph) in table if len(ph) == 4][:1]
        got = g.phrase_counts([k2, k4, k4, 0, 0], [p2, p4, p4 + p4 * 8, (), (1,)], 3, 5)
        assert got.tolist() == [0, table[k4, p4][0], 0, 0, 0]
        got = g.phrase_counts([k2, k4, 1], [p2, p4, tuple([1] * 33)], 2, 32)
        assert got.tolist() == [table[k2, p2][0], table[k4, p4][0], 0]
        assert g.phrase_counts([], []).shape == (0,)


def test_phrase_counts_past_two_trips_of_the_lookup_grid():
    """The lookup gives a thread a query and caps its grid at 2048 blocks of
    256: 2 x 524288 + 37 queries, the corpus' own phrases in turn."""
    K, D, P = 4, 300, 2048 * 256
    c = _corpus(_lengths(K + D, D), 12, 5)
    with _sampler(c, K) as g:
        g.sweep(2)
        table, _ = N.phrase_table(c.words, g.z(), c.doc_off, 2, 2)
        keys = sorted(table)
        Q, m = 2 * P + 37, len(keys)
        pick = np.arange(Q) % m
        topics = np.array([k for k, _ in keys], np.int32)[pick]
        words = np.ascontiguousarray(np.array([ph for _, ph in keys], np.int32)[pick].reshape(-1))
        topics[P + 5] = (topics[P + 5] + 1) % K                 # whatever that is, it is in the table or 0
        off = np.arange(Q + 1, dtype=np.int64) * 2
        cnt = np.full(Q, -5, np.int64)
        first = np.full(Q, -5, np.int64)
        capi.check(g._L.lda_phrase_lookup(g._h, 2, 2, Q, topics.ctypes.data, off.ctypes.data, words.ctypes.data,
                                          cnt.ctypes.data, first.ctypes.data), "lda_phrase_lookup")
        e = np.array([table[k] for k in keys], np.int64)[pick]
        e[P + 5] = table.get((int(topics[P + 5]), tuple(words[2 * (P + 5):2 * (P + 5) + 2].tolist())), [0, -1])
        np.testing.assert_array_equal(cnt, e[:, 0])
        np.testing.assert_array_equal(first, e[:, 1])
        assert m > 37 and cnt[2 * P:].all()


# -------------------------------------------------------------- model level
def _model(corpus, K, devices=None, iters=4):
    from ldagibbssampling_amd import topic_model as tm
    il = tm.InstanceList.fromCorpus(corpus)
    m = tm.ParallelTopicModel(K, 0.5 * K, 0.01)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(iters)
    m.setOptimizeInterval(0)
    if devices is not None:
        m.setDevices(devices)
    m.addInstances(il)
    m.estimate()
    return m


def _shard_counts(c, z, K, G, lo, hi):
    """The shards' listed counts [G, K, 128]: the shards are the token-balanced
    contiguous document ranges the model cuts (lower bound of N g / G in
    doc_off)."""
    M = capi.PHRASES_MAX
    Ntok = int(c.doc_off[-1])
    begin = [0] + [int(np.searchsorted(c.doc_off, Ntok * g // G, side="left")) for g in range(1, G)] + \
        [len(c.doc_off) - 1]
    sc = np.zeros((G, K, M), np.int64)
    for g in range(G):
        off = c.doc_off[begin[g]:begin[g + 1] + 1]
        s, e = int(off[0]), int(off[-1])
        table, _ = N.phrase_table(c.words[s:e], z[s:e], off - s, lo, hi)
        for k, lst in enumerate(N.ranked(table, K)):
            cs = [x[1] for x in lst[:M]]
            sc[g, k, :len(cs)] = cs
    return sc


def test_model_topic_phrases_on_one_and_three_shards(tmp_path):
    from ldagibbssampling_amd import topic_model as tm
    K, D = 20, 300
    c = _corpus(_lengths(3, D), 8, 5)
    m1, m3 = _model(c, K), _model(c, K, devices=[0, 0, 0])
    assert m1.numShards() == 1 and m3.numShards() == 3
    # the shards sample the same chain
    z = m1.topicAssignments()
    assert z.tobytes() == m3.topicAssignments().tobytes()
    ex = _Expect(c, z, K)
    for n, lo, hi, mc in ((10, 2, 32, 1), (10, 3, 5, 2), (128, 2, 2, 1), (1, 2, 32, 1)):
        exp = ex.arrays(n, lo, hi, mc)
        r1 = m1.topicPhrases(n, lo, hi, mc)
        _same(r1[:7], exp)
        assert r1[7].tolist() == [n] * K
        r3 = m3.topicPhrases(n, lo, hi, mc)
        # runs and skipped_long are sums; distinct is not one with several shards
        np.testing.assert_array_equal(r3[4], exp[4])
        assert r3[5].tolist() == [-1] * K and r3[6] == exp[6]
        # proven against the bound recomputed here from the shards' own lists
        sc = _shard_counts(c, z, K, 3, lo, hi)
        B, proven = N.bound_and_proven(sc, r3[2])
        assert r3[7].tolist() == proven.tolist()
        for k in range(K):
            # the proven entries are the true leading phrases, in order
            p = int(min(proven[k], np.count_nonzero(exp[1][k])))
            for a, e in zip(r3[:4], exp[:4]):
                np.testing.assert_array_equal(a[k, :p], e[k, :p])
        if n <= 10:
            # here every entry is proven: the three shards give the one shard's arrays
            assert np.all(proven == n), "the corpus no longer proves its best %d" % n
            for a, b in zip(r1[:4], r3[:4]):
                assert a.tobytes() == b.tobytes()
        # every reported total is exact, proven or not
        table, _ = ex.table(lo, hi)
        for k in range(K):
            for i in range(n):
                if r3[1][k, i] > 0:
                    ph = tuple(r3[0][k, i, :r3[1][k, i]].tolist())
                    assert table[k, ph] == [int(r3[2][k, i]), int(r3[3][k, i])]
        for m, r in ((m1, r1), (m3, r3)):
            text = tm.format_topic_phrases(r[0], r[1], r[2], [str(w) for w in range(5)])
            assert m.topicPhrasesText(n, lo, hi, mc) == text
            path = tmp_path / "topic_phrases.txt"
            m.printTopicPhrases(path, n, lo, hi, mc)
            k0 = int(np.flatnonzero(r[1][:, 0])[0])     # the first topic with a phrase
            assert path.read_text() == text and text.startswith("#topic rank count phrase\n%d 0 " % k0)
            assert text.count("\n") == 1 + np.count_nonzero(r[1])
            got = m.getTopicPhrases(n, lo, hi, mc)
            assert got.phrases[k0][0] == (" ".join(str(w) for w in got.wordIds[k0][0]), int(r[2][k0, 0]))
            assert got.wordIds[k0][0] == tuple(r[0][k0, 0, :r[1][k0, 0]].tolist())
            assert got.counts.tobytes() == r[2].tobytes() and got.first.tobytes() == r[3].tobytes()
            assert got.runs.tobytes() == r[4].tobytes() and got.distinct.tobytes() == r[5].tobytes()
            assert got.skippedLong == r[6] and got.proven.tobytes() == r[7].tobytes()
            assert [len(p) for p in got.phrases] == np.count_nonzero(r[1], axis=1).tolist()
    m1.close()
    m3.close()


def test_model_topic_phrases_where_the_bound_cuts_the_proof():
    """K = 4 over 3001 documents at V = 50: every shard holds far more than 128
    phrases of each topic, nearly all of count 1, so B_k > 0 and only the
    entries above it are proven; those are the restatement's, in order, and
    every reported total is exact."""
    K, D, n = 4, 3001, 128
    c = _corpus(_lengths(4, D), 9, 50)
    m3 = _model(c, K, devices=[0, 0, 0], iters=3)
    z = m3.topicAssignments()
    ex = _Expect(c, z, K)
    for lo, hi, mc in ((2, 32, 1), (3, 5, 2)):
        exp = ex.arrays(n, lo, hi, mc)
        r3 = m3.topicPhrases(n, lo, hi, mc)
        sc = _shard_counts(c, z, K, 3, lo, hi)
        assert np.all(sc[:, :, -1] > 0), "a shard's list is not full"
        B, proven = N.bound_and_proven(sc, r3[2])
        assert r3[7].tolist() == proven.tolist() and np.all(B >= 3)
        assert np.any(proven < n), "no list was cut by the bound"
        for k in range(K):
            p = int(min(proven[k], np.count_nonzero(exp[1][k])))
            for a, e in zip(r3[:4], exp[:4]):
                np.testing.assert_array_equal(a[k, :p], e[k, :p])
        table, _ = ex.table(lo, hi)
        for k in range(K):
            for i in range(n):
                if r3[1][k, i] > 0:
                    ph = tuple(r3[0][k, i, :r3[1][k, i]].tolist())
                    assert table[k, ph] == [int(r3[2][k, i]), int(r3[3][k, i])]
                    assert r3[2][k, i] >= mc
        np.testing.assert_array_equal(r3[4], exp[4])
        assert r3[6] == exp[6]
    m3.close()


def test_topic_phrases_between_two_sweeps_changes_nothing():
    K = 100
    c = _corpus(_lengths(9, 300), 4, 5)
    with _sampler(c, K, seed=21) as g, _sampler(c, K, seed=21) as ref:
        g.sweep(2)
        ref.sweep(2)
        before = g.counts_checksum()
        assert before == ref.counts_checksum()
        ex = _Expect(c, g.z(), K)
        w, lens, *_ = _check(g, ex, 64, 2, 32, 1)
        g.phrase_counts([0], [tuple(w[0, 0, :max(lens[0, 0], 2)].clip(0).tolist())])
        assert g.counts_checksum() == before
        g.sweep(1)
        ref.sweep(1)
        assert g.z().tobytes() == ref.z().tobytes() and g.counts_checksum() == ref.counts_checksum()


# --------------------------------------------------------- state and errors
def test_topic_phrases_state_and_errors():
    K = 20
    c = _corpus(_lengths(1, 12), 2, 5)
    with _sampler(c, K) as g:
        # lda_create leaves the shard's counts as the pending delta
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
            g.topic_phrases(3)
        assert e.value.status == -4
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.phrase_counts([0], [(1, 2)])
        g.sweep(1)
        w = np.zeros(K * 129 * 32, np.int32)
        o = np.zeros(K * 129, np.int64)
        p, q = w.ctypes.data, o.ctypes.data
        outs = (p, p, q, q, q, q, q)
        call, err = g._L.lda_topic_phrases, g._L.lda_last_error
        for n in (0, -1, capi.PHRASES_MAX + 1):
            assert call(g._h, n, 2, 32, 1, *outs) == -1 and b"LDA_PHRASES_MAX" in err()
        for lo, hi in ((1, 32), (5, 4), (2, 33)):
            assert call(g._h, 3, lo, hi, 1, *outs) == -1 and b"LDA_PHRASE_LEN_MAX" in err()
        for mc in (0, -2):
            assert call(g._h, 3, 2, 32, mc, *outs) == -1 and b"min_count" in err()
        for i in range(len(outs)):
            args = list(outs)
            args[i] = None
            assert call(g._h, 3, 2, 32, 1, *args) == -1 and b"null output" in err()
        assert not w.any() and not o.any()              # nothing was written
        # the queries: a topic, a word id and the offsets
        look = g._L.lda_phrase_counts
        t = np.array([0, K], np.int32)
        off = np.array([0, 2, 4], np.int64)
        ph = np.array([1, 2, 3, 4], np.int32)
        cnt = np.full(2, 77, np.int64)
        a = (t.ctypes.data, off.ctypes.data, ph.ctypes.data, cnt.ctypes.data)
        assert look(g._h, 2, 32, 2, *a) == -1 and b"topic" in err()
        t[1] = -1
        assert look(g._h, 2, 32, 2, *a) == -1 and b"topic" in err()
        t[1] = K - 1
        ph[3] = 5                                       # V = 5
        assert look(g._h, 2, 32, 2, *a) == -1 and b"word id" in err()
        ph[3] = -1
        assert look(g._h, 2, 32, 2, *a) == -1 and b"word id" in err()
        ph[3] = 4
        off[:] = [0, 3, 2]
        assert look(g._h, 2, 32, 2, *a) == -1 and b"phrase_off" in err()
        off[:] = [1, 2, 4]
        assert look(g._h, 2, 32, 2, *a) == -1 and b"phrase_off" in err()
        off[:] = [0, 2, 4]
        assert look(g._h, 1, 32, 2, *a) == -1 and b"LDA_PHRASE_LEN_MAX" in err()
        assert look(g._h, 2, 32, -1, *a) == -1 and b"Q" in err()
        assert look(g._h, 2, 32, 2, a[0], a[1], a[2], None) == -1 and b"null" in err()
        assert cnt.tolist() == [77, 77]                 # nothing was written
        assert look(g._h, 2, 32, 2, *a) == 0
        # a pending delta again: sample() without apply()
        g.sample()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.topic_phrases(3)
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.phrase_counts([0], [(1, 2)])
        g.apply()
        ex = _Expect(c, g.z(), K)
        _check(g, ex, 128, 2, 32, 1)
        assert _bytes(g.topic_phrases(128, 2, 32, 1)) == _bytes(g.topic_phrases(128, 2, 32, 1))


@pytest.mark.parametrize("D", [0, 3])
def test_topic_phrases_without_documents_or_tokens(D):
    K = 20
    c = _corpus(np.zeros(D, np.int64), 1, 5)
    with _sampler(c, K) as g:
        g.sweep(1)
        w, lens, cnt, first, runs, distinct, skipped = g.topic_phrases(7, 2, 5, 1)
        assert w.shape == (K, 7, 5) and np.all(w == -1) and not lens.any() and not cnt.any() and np.all(first == -1)
        assert not runs.any() and not distinct.any() and skipped == 0
        assert g.phrase_counts([1, 2], [(1, 2), (3, 3, 3)]).tolist() == [0, 0]
