"""GPU checks of the topic diagnostics: lda_topic_codocuments (k_codoc,
k_doc_diag), lda_topic_word_stats (k_word_stats, k_sumsq), their ldatm_
mirrors and ParallelTopicModel.getDiagnostics.

Every expectation is numpy on z(), the corpus and counts().  The integer
outputs are compared with array_equal; share_sums at rtol 1e-13 (at most 2048
fp64 addends of one sign, each good to an ulp of 1.1e-16, added in another
order); the eleven columns against test_diagnostics.restate at its derived
rtol = atol = 1e-12.

Geometry the shapes reach: a block of k_codoc holds min(K, 65536 / (128 +
2 n (n + 1))) topics, so n = 1 (132 bytes a topic, 496 topics) is one group up
to K = 100, two at K = 512 and five at K = 2048; n = 7 (240 bytes, 273 topics)
two groups at K = 512 and eight at 2048; n = 64 (8448 bytes, 7 topics) three
groups at K = 20 and 293 at K = 2048, the last group partial everywhere.  A
block has 16 waves and there are at most 2 x CUs / groups document slabs, so
with one group 19 slabs take the 300 documents (a wave one document or none)
and with 293 groups one slab does (a wave 18 or 19 documents in turn).
k_doc_diag counts through per-block LDS counters while 16 Kp + 4 K (2 + P)
<= 65536 (every K here up to 512) and straight to global memory at K = 2048.
"""
import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu

MALLET_PROPS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
BETA = 0.05
V300 = 300


# ------------------------------------------------------------------ helpers
def _lengths(seed, n):
    """test_readout_gpu._lengths: an empty document, a one-token one, one
    wave's 64 lanes, 65, several passes, among ordinary ones, shuffled."""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 64, 65, 150]
    lens = np.array(fixed + rng.integers(2, 40, n - len(fixed)).tolist(), np.int64)
    rng.shuffle(lens)
    return lens


def _corpus(lengths, V, seed):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    return Corpus(off, words, V)


def _sampler_kind(K):
    return "sparse" if K > capi.MAX_TOPICS_DENSE else "dense"


def _seq_sum(alpha):
    s = 0.0
    for a in alpha:          # added in index order, as the library adds them
        s += float(a)
    return s


def shape_alpha(K):
    """Topic 3 is heavy (a third of every document after two sweeps), so that
    at every K some topic holds more than 32 different words."""
    a = np.full(K, 0.3)
    a[3] = 40.0
    return a


def doc_counts(doc_off, z, K):
    D = len(doc_off) - 1
    doc = np.repeat(np.arange(D), np.diff(doc_off))
    nd = np.zeros((D, K), np.int64)
    np.add.at(nd, (doc, z), 1)
    return nd


def presence(doc_off, words, z, ids, V):
    """pres[k, i, d]: document d holds a token of word ids[k, i] assigned to k."""
    K, n = ids.shape
    D = len(doc_off) - 1
    slot = np.full((K, V), -1, np.int64)
    kk, ii = np.nonzero(ids >= 0)
    slot[kk, ids[kk, ii]] = ii
    doc = np.repeat(np.arange(D), np.diff(doc_off))
    s = slot[z, words]
    sel = s >= 0
    pres = np.zeros((K, n, D), bool)
    pres[z[sel], s[sel], doc[sel]] = True
    return pres


def expected_codoc(pres):
    """The packed lower triangles [K, n (n + 1) / 2] (int32) of pres."""
    K, n, D = pres.shape
    assert D < 2 ** 24                       # float32 products of 0 / 1 add exactly
    p = pres.astype(np.float32)
    full = np.matmul(p, p.transpose(0, 2, 1)).astype(np.int32)
    i, j = np.tril_indices(n)
    return np.ascontiguousarray(full[:, i, j])


def expected_doc_stats(nd, alpha, props):
    D, K = nd.shape
    lens = nd.sum(1)
    out = np.zeros((K, 2 + len(props)), np.int64)
    out[:, 0] = (nd > 0).sum(0)
    full = lens > 0
    out[:, 1] = np.bincount(np.argmax(nd[full], axis=1), minlength=K)   # the first maximum: the smallest id
    w = (alpha[None, :] + nd.astype(np.float64)) / (lens.astype(np.float64)[:, None] + _seq_sum(alpha))
    for i, p in enumerate(props):
        out[:, 2 + i] = ((nd > 0) & (w >= p)).sum(0)
    return out


def expected_word_stats(nw, nwsum, ids, beta):
    V, K = nw.shape
    live = ids >= 0
    w = np.where(live, ids, 0)
    k = np.arange(K)[:, None]
    counts = np.where(live, nw[w, k], 0).astype(np.int32)
    totals = np.where(live, nw.astype(np.int64).sum(1)[w], 0)
    share = (beta + nw.astype(np.float64)) / (V * beta + nwsum.astype(np.float64))[None, :]
    shares = np.where(live, share.sum(1)[w], 0.0)
    sumsq = (nw.astype(np.int64) ** 2).sum(0).astype(np.uint64)
    return counts, totals, shares, sumsq


def check_word_stats(g, ids, nw, nwsum):
    counts, totals, shares, sumsq = g.topic_word_stats(ids)
    ec, et, es, eq = expected_word_stats(nw, nwsum, ids, g.beta)
    np.testing.assert_array_equal(counts, ec)
    np.testing.assert_array_equal(totals, et)
    np.testing.assert_array_equal(sumsq, eq)
    np.testing.assert_allclose(shares, es, rtol=1e-13, atol=0)
    assert np.all(shares[ids < 0] == 0)
    again = g.topic_word_stats(ids)
    for a, b in zip((counts, totals, shares, sumsq), again):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------- shapes
PROPS_BY_N = {1: (), 7: MALLET_PROPS, 64: (0.001, 0.01, 0.02, 0.05, 0.1, 0.25, 0.5, 1.0)}
# sampler seeds under which the input exercises the kernel (asserted below; checked on the CPU with
# oracle.ExactSampler, which draws what the device draws): K * 7 + 1 everywhere but K = 20, where
# that seed leaves the twenty top-1 words all different
SEEDS = {20: 2, 64: 449, 100: 701, 512: 3585, 2048: 14337}


@pytest.mark.parametrize("K", [20, 64, 100, 512, 2048])
def test_codocuments_and_word_stats_against_numpy(K):
    from ldagibbssampling_amd.sampler import GibbsSampler
    c = _corpus(_lengths(K, V300), V300, 5)
    assert c.num_docs == 300 and {0, 1, 64, 65, 150} <= set(np.diff(c.doc_off).tolist())
    alpha = shape_alpha(K)
    with GibbsSampler(K, V300, c.doc_off, c.words, alpha, BETA, seed=SEEDS[K], sampler=_sampler_kind(K)) as g:
        g.sweep(2)
        z = g.z()
        nw, nwsum = g.counts()[:2]
        nd = doc_counts(c.doc_off, z, K)
        # some document's largest count is shared by two topics: the tie rule decides
        top2 = np.sort(nd, axis=1)[:, -2:]
        assert np.any((top2[:, 0] == top2[:, 1]) & (top2[:, 1] > 0)), "no rank-1 tie"
        for n in (1, 7, 64):
            ids = g.top_words(n)[0]
            pres = presence(c.doc_off, c.words, z, ids, V300)
            want = expected_codoc(pres)
            # the input exercises the kernel
            live = ids[ids >= 0]
            assert len(np.unique(live)) < len(live), "no word stands in two topics' lists"
            if n > 1:
                i, j = np.tril_indices(n)
                assert np.any(want[:, i != j] > 0), "no off-diagonal cell is positive"
            if n == 64:
                assert pres[:, 32:, :].any(), "no document sets a slot >= 32"
            props = PROPS_BY_N[n]
            codoc, stats = g.topic_codocuments(ids, props)
            assert codoc.dtype == np.int32 and stats.dtype == np.int64
            np.testing.assert_array_equal(codoc, want)
            np.testing.assert_array_equal(stats, expected_doc_stats(nd, alpha, props))
            # cells of empty slots are 0; the diagonal is the document frequency under the topic
            i, j = np.tril_indices(n)
            assert np.all(codoc[(ids[:, i] < 0) | (ids[:, j] < 0)] == 0)
            again = g.topic_codocuments(ids, props)
            assert again[0].tobytes() == codoc.tobytes() and again[1].tobytes() == stats.tobytes()
            check_word_stats(g, ids, nw, nwsum)


# ---------------------------------------------------------- arbitrary lists
def test_arbitrary_lists_with_empty_slots_and_absent_words():
    from ldagibbssampling_amd.sampler import GibbsSampler
    K, n = 20, 5
    c = _corpus(_lengths(3, 120), 60, 9)
    alpha = np.linspace(0.2, 1.1, K)
    with GibbsSampler(K, 60, c.doc_off, c.words, alpha, BETA, seed=11) as g:
        g.sweep(2)
        z = g.z()
        nw, nwsum = g.counts()[:2]
        rng = np.random.default_rng(1)
        ids = np.stack([rng.permutation(60)[:n] for _ in range(K)]).astype(np.int32)
        ids[:, 2] = -1                               # an empty slot in the middle of every list
        ids[4] = -1                                  # a topic with no list at all
        absent = np.argwhere((nw == 0) & (np.arange(K)[None, :] != 4))
        assert len(absent), "every word has every topic"
        w0, k0 = (int(x) for x in absent[0])          # a listed word with count 0 in its topic
        ids[k0] = [w0, -1, -1, (w0 + 1) % 60, -1]
        pres = presence(c.doc_off, c.words, z, ids, 60)
        want = expected_codoc(pres)
        assert want.any() and not want[k0, 0]
        codoc, stats = g.topic_codocuments(ids, (0.05, 0.5))
        np.testing.assert_array_equal(codoc, want)
        np.testing.assert_array_equal(stats, expected_doc_stats(doc_counts(c.doc_off, z, K), alpha, (0.05, 0.5)))
        check_word_stats(g, ids, nw, nwsum)


# ------------------------------------------- counted under the topic's own z
def test_codocuments_count_only_the_topics_own_assignments():
    from ldagibbssampling_amd.sampler import GibbsSampler
    a, b = 2, 5
    off = np.array([0, 3, 4, 4], np.int64)           # the last document is empty
    words = np.array([a, a, b, b], np.int32)
    z = np.array([0, 1, 1, 0], np.int32)             # document 0: a under 0 and 1, b under 1 only
    ids = np.array([[a, b], [a, b], [-1, -1]], np.int32)
    with GibbsSampler(3, 8, off, words, np.full(3, 0.5), 0.01, seed=1, z_init=z) as g:
        g.apply()
        np.testing.assert_array_equal(g.z(), z)
        codoc, stats = g.topic_codocuments(ids)
        #                                      (a,a) (b,a) (b,b)
        assert codoc.tolist() == [[1, 0, 1],   # topic 0: a in document 0, b in document 1, never together
                                  [1, 1, 1],   # topic 1: a and b together in document 0
                                  [0, 0, 0]]
        # documents holding the topic; documents it ranks first in (document 0: topic 1 with 2 of 3)
        assert stats.tolist() == [[2, 1], [1, 1], [0, 0]]


# --------------------------------------------------- thresholds hit exactly
def test_a_weight_equal_to_a_threshold_counts():
    """alpha_k = 1, K = 10, documents of 10 tokens: (1 + n_dk) / 20 is exactly
    0.1, 0.2, 0.3, 0.5 for n_dk = 1, 3, 5, 9."""
    from ldagibbssampling_amd.sampler import GibbsSampler
    K = 10
    z = np.array([0] * 1 + [1] * 9 + [2] * 3 + [3] * 5 + [4] + [5], np.int32)
    off = np.array([0, 10, 20], np.int64)
    words = (np.arange(20) % 7).astype(np.int32)
    alpha = np.ones(K)
    for x, y in ((2.0, 0.1), (4.0, 0.2), (6.0, 0.3), (10.0, 0.5)):
        assert x / 20.0 == y                          # the host's quotient is the threshold's own bits
    ids = np.full((K, 1), -1, np.int32)
    with GibbsSampler(K, 7, off, words, alpha, 0.01, seed=1, z_init=z) as g:
        g.apply()
        stats = g.topic_codocuments(ids, MALLET_PROPS)[1]
    #        docs rank1 .01 .02 .05 .1 .2 .3 .5
    want = [[1, 0, 1, 1, 1, 1, 0, 0, 0],    # n_dk = 1: 0.1
            [1, 1, 1, 1, 1, 1, 1, 1, 1],    # 9: 0.5
            [1, 0, 1, 1, 1, 1, 1, 0, 0],    # 3: 0.2
            [1, 1, 1, 1, 1, 1, 1, 1, 0],    # 5: 0.3
            [1, 0, 1, 1, 1, 1, 0, 0, 0],
            [1, 0, 1, 1, 1, 1, 0, 0, 0]] + [[0] * 9] * 4
    assert stats.tolist() == want
    np.testing.assert_array_equal(stats, expected_doc_stats(doc_counts(off, z, K), alpha, MALLET_PROPS))


# ------------------------------------------------------------------- errors
def test_diagnostics_errors():
    from ldagibbssampling_amd.sampler import GibbsSampler
    K, V = 20, 60
    c = _corpus(_lengths(1, 12), V, 2)
    with GibbsSampler(K, V, c.doc_off, c.words, np.full(K, 0.5), 0.01, seed=3) as g:
        ids = np.full((K, 3), -1, np.int32)
        ids[:, 0] = np.arange(K)
        # lda_create leaves the shard's counts as the pending delta
        for call in (lambda: g.topic_codocuments(ids), lambda: g.topic_word_stats(ids)):
            with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
                call()
            assert e.value.status == -4
        g.sweep(1)
        L, h = g._L, g._h
        out = np.zeros(K * 65 * 33, np.int64)
        p, good = out.ctypes.data, ids.ctypes.data
        props = np.array(MALLET_PROPS)

        def failed(status, word):
            return status == -1 and word in L.lda_last_error()

        for n in (0, 65):
            assert failed(L.lda_topic_codocuments(h, n, good, 0, None, p, p), b"LDA_DIAG_WORDS_MAX")
            assert failed(L.lda_topic_word_stats(h, n, good, p, p, p, p), b"LDA_DIAG_WORDS_MAX")
        assert failed(L.lda_topic_codocuments(h, 3, None, 0, None, p, p), b"null word_ids")
        assert failed(L.lda_topic_word_stats(h, 3, None, p, p, p, p), b"null word_ids")
        for bad in (-2, V):
            b = ids.copy()
            b[7, 2] = bad
            assert failed(L.lda_topic_codocuments(h, 3, b.ctypes.data, 0, None, p, p), b"outside [-1, V)")
            assert failed(L.lda_topic_word_stats(h, 3, b.ctypes.data, p, p, p, p), b"outside [-1, V)")
        b = ids.copy()
        b[7, 2] = 7
        assert failed(L.lda_topic_codocuments(h, 3, b.ctypes.data, 0, None, p, p), b"twice")
        assert failed(L.lda_topic_word_stats(h, 3, b.ctypes.data, p, p, p, p), b"twice")
        assert failed(L.lda_topic_codocuments(h, 3, good, 9, props.ctypes.data, p, p), b"LDA_DIAG_PROPS_MAX")
        assert failed(L.lda_topic_codocuments(h, 3, good, 2, None, p, p), b"null props")
        for bad in ([0.2, 0.1], [0.3, 0.3], [0.0], [1.5]):
            q = np.array(bad)
            assert failed(L.lda_topic_codocuments(h, 3, good, len(q), q.ctypes.data, p, p), b"strictly ascending")
        assert failed(L.lda_topic_codocuments(h, 3, good, 0, None, None, p), b"null output")
        assert failed(L.lda_topic_codocuments(h, 3, good, 0, None, p, None), b"null output")
        for i in range(4):
            a = [p] * 4
            a[i] = None
            assert failed(L.lda_topic_word_stats(h, 3, good, *a), b"null output")
        # a pending delta again: sample() without apply(); after apply() the calls answer
        g.sample()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.topic_codocuments(ids)
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.topic_word_stats(ids)
        g.apply()
        codoc, stats = g.topic_codocuments(ids, (1.0,))
        assert codoc.shape == (K, 6) and stats.shape == (K, 3)
        assert g.topic_word_stats(ids)[0].shape == (K, 3)


# -------------------------------------------------------------- model level
def _model(corpus, K, alpha_sum, devices=None, iters=4):
    from ldagibbssampling_amd import topic_model as tm
    il = tm.InstanceList.fromCorpus(corpus)
    m = tm.ParallelTopicModel(K, alpha_sum, 0.01)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(iters)
    m.setOptimizeInterval(0)
    if devices is not None:
        m.setDevices(devices)
    m.addInstances(il)
    m.estimate()
    return m


def test_model_diagnostics_on_one_and_three_shards():
    from test_diagnostics import restate
    K, n = 100, 7
    c = _corpus(_lengths(4, V300), V300, 8)
    m1 = _model(c, K, 50.0)
    m3 = _model(c, K, 50.0, devices=[0, 0, 0])
    try:
        assert m1.numShards() == 1 and m3.numShards() == 3
        z = m1.topicAssignments()
        np.testing.assert_array_equal(m3.topicAssignments(), z)
        s1, s3 = m1.topicStatistics(n), m3.topicStatistics(n)
        for name in s1:
            assert s1[name].tobytes() == s3[name].tobytes(), name
        d1, d3 = m1.getDiagnostics(n), m3.getDiagnostics(n)
        assert d1.columns.tobytes() == d3.columns.tobytes()
        assert d1.codocuments.tobytes() == d3.codocuments.tobytes()
        # against numpy: the statistics, the histogram's sums, then the columns
        nw, nwsum = m1.typeTopicCounts()
        alpha = m1.alpha
        nd = doc_counts(c.doc_off, z, K)
        ids = s1["word_ids"]
        np.testing.assert_array_equal(ids, d1.wordIds)
        np.testing.assert_array_equal(s1["codoc"], expected_codoc(presence(c.doc_off, c.words, z, ids, V300)))
        np.testing.assert_array_equal(s1["doc_stats"], expected_doc_stats(nd, alpha, MALLET_PROPS))
        ec, et, es, eq = expected_word_stats(nw, nwsum, ids, m1.beta)
        np.testing.assert_array_equal(s1["counts"], ec)
        np.testing.assert_array_equal(s1["totals"], et)
        np.testing.assert_array_equal(s1["sumsq"], eq)
        np.testing.assert_allclose(s1["share_sums"], es, rtol=1e-13, atol=0)
        max_len = int(np.diff(c.doc_off).max())
        H = np.zeros((K, max_len + 1), np.int64)
        for k in range(K):
            H[k] = np.bincount(nd[:, k], minlength=max_len + 1)
        H[:, 0] = 0
        np.testing.assert_array_equal(H.sum(1), s1["doc_stats"][:, 0])
        want = restate(V300, m1.beta, nwsum, H, ids, s1["counts"], s1["totals"], s1["share_sums"], s1["sumsq"],
                       s1["codoc"], s1["doc_stats"])
        np.testing.assert_allclose(d1.columns, want, rtol=1e-12, atol=1e-12)
        i, j = np.tril_indices(n)
        np.testing.assert_array_equal(d1.codocuments[:, i, j], s1["codoc"])
        np.testing.assert_array_equal(d1.codocuments, d1.codocuments.transpose(0, 2, 1))
        rows = d1.as_rows()
        assert len(rows) == K and rows[5]["topic"] == 5 and rows[5]["coherence"] == d1.coherence[5]
        assert rows[5]["words"] == d1.topWords[5] == [int(w) for w in ids[5] if w >= 0]
    finally:
        m1.close()
        m3.close()


def test_diagnostics_end_to_end():
    """The training corpus of test_perplexity at K = 20, 30 sweeps.  The seed
    is one under which every topic leads some document: with seeds 1, 3 and 5
    the chain still holds, after 30 sweeps, a topic of ~2500 tokens spread over
    ~1000 documents that is the largest in none of them (rank_1_docs = 0: the
    kind of topic this readout is there to show), found on the CPU with
    oracle.ExactSampler under the model's sweep schedule; seeds 2 and 4 hold
    none."""
    from ldagibbssampling_amd import topic_model as tm
    from ldagibbssampling_amd.corpus import synthetic_lda
    K = 20
    c = synthetic_lda(num_docs=2200, num_types=3000, num_topics=K, doc_len=None, mean_len=80, min_len=10,
                      max_len=300, seed=20261015, k_true=min(K, 50))
    perm = np.random.default_rng(0).permutation(c.num_docs)
    train = c.subset(np.sort(perm[c.num_docs // 10:]))
    m = tm.ParallelTopicModel(K, 10.0, 0.01)
    try:
        m.setRandomSeed(2)
        m.setTopicDisplay(0, 0)
        m.setNumIterations(30)
        m.setOptimizeInterval(0)
        m.addInstances(tm.InstanceList.fromCorpus(train))
        m.estimate()
        d = m.getDiagnostics(10)
        assert d.columns.shape == (K, 11) and np.isfinite(d.columns).all()
        assert (d.coherence <= 0).all()
        assert ((d.rank_1_docs > 0) & (d.rank_1_docs <= 1)).all()
        assert ((d.eff_num_words >= 1) & (d.eff_num_words <= train.num_types)).all()
        assert d.tokens.sum() == train.num_tokens
        assert all(len(w) == 10 for w in d.topWords) and d.codocuments.shape == (K, 10, 10)
    finally:
        m.close()
