"""GPU checks of the readouts selected on the device: lda_top_words
(k_top_words_slab + k_top_words_merge), lda_doc_top_topics, lda_doc_counts,
their ldatm_ mirrors, and the text outputs that now take their order from them.

Every expectation is numpy on counts() / topicAssignments() with
np.lexsort((ids, -values)): value descending, equal values by ascending id.
Everything is exact (integers, or fp64 weights from the host's expression
(alpha_k + n_dk) / (n_d + alphaSum), whose IEEE quotient numpy computes too).

Slabs: the slab pass gives a slab at least 256 rows, so V = 1 and 7 are one
partial slab, V = 300 two slabs, and V = 3001 twelve slabs (eleven of 251
rows and one of 240) at every K used here (the cap is 1024 / (Kp / 64) >= 32
slabs).
"""
import ctypes as C

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def _corpus(lengths, V, seed):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    return Corpus(off, words, V)


def _lengths(seed, n=40):
    """An empty document, a one-token one, one wave's 64 lanes, 65, several
    passes, among ordinary ones, shuffled."""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 64, 65, 150]
    lens = np.array(fixed + rng.integers(2, 40, n - len(fixed)).tolist(), np.int64)
    rng.shuffle(lens)
    return lens


def _sampler_kind(K):
    return "sparse" if K > capi.MAX_TOPICS_DENSE else "dense"


def _seq_sum(alpha):
    s = 0.0
    for a in alpha:          # added in index order, as the library adds them
        s += float(a)
    return s


def expected_top_words(nw, n):
    V, K = nw.shape
    ids = np.full((K, n), -1, np.int32)
    cnt = np.zeros((K, n), np.int32)
    w = np.arange(V)
    for k in range(K):
        col = nw[:, k].astype(np.int64)
        order = np.lexsort((w, -col))
        order = order[col[order] > 0][:n]
        ids[k, :len(order)] = order
        cnt[k, :len(order)] = col[order]
    return ids, cnt


def expected_top_topics(nd, lens, alpha, alpha_sum, m):
    M, K = nd.shape
    topics = np.full((M, m), -1, np.int32)
    cnt = np.zeros((M, m), np.int32)
    weights = (alpha[None, :] + nd) / (lens.astype(np.float64)[:, None] + alpha_sum)
    k = np.arange(K)
    for j in range(M):
        order = np.lexsort((k, -weights[j]))[:m]
        topics[j, :len(order)] = order
        cnt[j, :len(order)] = nd[j, order]
    return topics, cnt


def _has_tie(cnt):
    """Some topic's selection holds two equal positive counts."""
    a, b = cnt[:, :-1], cnt[:, 1:]
    return bool(np.any((a == b) & (a > 0)))


# ------------------------------------------------------- top words, shapes
@pytest.mark.parametrize("V", [1, 7, 300, 3001])
@pytest.mark.parametrize("K", [20, 64, 100, 512, 2048])
def test_top_words_against_numpy(K, V):
    from ldagibbssampling_amd.sampler import GibbsSampler
    assert (capi.padded_topics(K) != K) == (K in (20, 100))          # 20 and 100 are padded
    c = _corpus(_lengths(K + V), V, 5)
    with GibbsSampler(K, V, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=K * 7 + V,
                      sampler=_sampler_kind(K)) as g:
        g.sweep(3)
        nw = g.counts()[0]
        assert nw.sum() == c.num_tokens
        for n in (1, 7, 64):
            ids, cnt = g.top_words(n)
            eids, ecnt = expected_top_words(nw, n)
            np.testing.assert_array_equal(ids, eids)
            np.testing.assert_array_equal(cnt, ecnt)
            assert np.all(cnt[ids < 0] == 0)
            if V >= 7 and n >= 7:
                # the small corpus leaves many equal counts: the tie order is exercised
                assert _has_tie(ecnt), "no tie among any topic's best n"
        if V >= 7:
            # n = 1: in some topic the winner is tied with the runner-up, so the id decided
            two = expected_top_words(nw, 2)[1]
            assert np.any((two[:, 0] == two[:, 1]) & (two[:, 0] > 0))
        again = g.top_words(64)
        assert again[0].tobytes() == eids.tobytes() and again[1].tobytes() == ecnt.tobytes()


# -------------------------------------------- top words, constructed states
def _constructed(K, V, word_topic_count):
    """A one-document-per-token corpus whose z gives nw[w, k] = the given
    counts: (sampler, nw).  Set through set_z + apply."""
    from ldagibbssampling_amd.sampler import GibbsSampler
    words, z = [], []
    for (w, k), n in sorted(word_topic_count.items()):
        words += [w] * n
        z += [k] * n
    words = np.array(words, np.int32)
    z = np.array(z, np.int32)
    # documents of 50 tokens (the last one shorter)
    off = np.append(np.arange(0, len(words), 50), len(words)).astype(np.int64)
    g = GibbsSampler(K, V, off, words, np.full(K, 0.3), 0.05, seed=1)
    g.set_z(z)
    g.apply()
    nw = g.counts()[0]
    exp = np.zeros((V, K), np.int32)
    for (w, k), n in word_topic_count.items():
        exp[w, k] = n
    np.testing.assert_array_equal(nw, exp)
    return g, nw


def _check_top_words(g, nw, ns=(1, 7, 64)):
    for n in ns:
        ids, cnt = g.top_words(n)
        eids, ecnt = expected_top_words(nw, n)
        np.testing.assert_array_equal(ids, eids)
        np.testing.assert_array_equal(cnt, ecnt)
    return eids, ecnt


def test_top_words_ascending_counts_every_row_inserts():
    """(a) topic 0 holds word w exactly w + 1 times: within a slab every row
    beats the running threshold."""
    V, K = 600, 20                              # three slabs of 200 rows
    g, nw = _constructed(K, V, {(w, 0): w + 1 for w in range(V)})
    eids, ecnt = _check_top_words(g, nw)
    assert eids[0].tolist() == list(range(V - 1, V - 65, -1)) and ecnt[0, 0] == V
    assert np.all(eids[1:] == -1) and np.all(ecnt[1:] == 0)
    g.close()


def test_top_words_descending_counts():
    """(b) the mirror image: after a slab's first n rows nothing inserts."""
    V, K = 600, 20
    g, nw = _constructed(K, V, {(w, 3): V - w for w in range(V)})
    eids, ecnt = _check_top_words(g, nw)
    assert eids[3].tolist() == list(range(64)) and ecnt[3, 0] == V
    g.close()


def test_top_words_single_topic_everything_else_fills():
    """(c) all tokens in one topic (a padded K: topics 100..127 exist only as
    padding and are never reported)."""
    V, K = 300, 100
    rng = np.random.default_rng(3)
    g, nw = _constructed(K, V, {(w, 77): int(rng.integers(1, 5)) for w in range(V)})
    eids, ecnt = _check_top_words(g, nw)
    assert eids.shape == (K, 64)
    assert np.all(np.delete(eids, 77, axis=0) == -1) and np.all(np.delete(ecnt, 77, axis=0) == 0)
    assert np.all(eids[77] >= 0) and _has_tie(ecnt)
    g.close()


def test_top_words_fewer_than_n_distinct_words():
    """(d) a topic with 5 words among 700 rows (three slabs of 234 rows, each
    holding one or two of them)."""
    V, K = 700, 64
    g, nw = _constructed(K, V, {(3, 9): 4, (650, 9): 4, (300, 9): 9, (299, 9): 1, (699, 9): 2, (0, 63): 1})
    eids, ecnt = _check_top_words(g, nw)
    assert eids[9, :6].tolist() == [300, 3, 650, 699, 299, -1] and ecnt[9, :6].tolist() == [9, 4, 4, 2, 1, 0]
    assert eids[63, :2].tolist() == [0, -1]
    g.close()


def test_top_words_all_equal_counts_gives_the_smallest_ids():
    """(e) every word with the same count in a topic."""
    V, K = 600, 20
    g, nw = _constructed(K, V, {(w, 5): 2 for w in range(V)})
    eids, ecnt = _check_top_words(g, nw)
    assert eids[5].tolist() == list(range(64)) and np.all(ecnt[5] == 2)
    g.close()


# ------------------------------------------------------------- model level
def _model(corpus, K, alpha_sum, devices=None, iters=4, alpha=None, **opts):
    from ldagibbssampling_amd import topic_model as tm
    il = tm.InstanceList.fromCorpus(corpus)
    m = tm.ParallelTopicModel(K, alpha_sum, 0.01)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(iters)
    m.setOptimizeInterval(0)
    for k, v in opts.items():
        getattr(m, k)(*v) if isinstance(v, tuple) else getattr(m, k)(v)
    if devices is not None:
        m.setDevices(devices)
    if alpha is not None:
        a = np.ascontiguousarray(alpha, np.float64)
        st = m._L.ldatm_set_hyper(m._h, a.ctypes.data, _seq_sum(a), 0.01)
        assert st == 0, m._L.ldatm_last_error()
    m.addInstances(il)
    m.estimate()
    return m, il


def _model_nd(m, corpus):
    z = m.topicAssignments()
    doc = np.repeat(np.arange(corpus.num_docs), np.diff(corpus.doc_off))
    nd = np.zeros((corpus.num_docs, m.numTopics), np.int32)
    np.add.at(nd, (doc, z), 1)
    return nd


def test_top_words_on_one_and_three_shards():
    c = _corpus(_lengths(4), 3001, 8)
    m1, _ = _model(c, 100, 50.0)
    m3, _ = _model(c, 100, 50.0, devices=[0, 0, 0])
    assert m1.numShards() == 1 and m3.numShards() == 3
    nw = m1.typeTopicCounts()[0]
    np.testing.assert_array_equal(m3.typeTopicCounts()[0], nw)
    for n in (1, 7, 64):
        a, b = m1.topWords(n), m3.topWords(n)
        e = expected_top_words(nw, n)
        for x, y, z in zip(a, b, e):
            assert x.tobytes() == y.tobytes() == z.tobytes()
    got = m1.getTopWords(3)
    assert got[0] == [(int(w), int(k)) for w, k in zip(*[x[0] for x in expected_top_words(nw, 3)]) if w >= 0]
    m1.close()
    m3.close()


def _top_words_text(m, il, num_words, nl):
    from ldagibbssampling_amd.topic_model import format_double
    nw = m.typeTopicCounts()[0]
    alpha = m.alpha
    names = [str(w) for w in il.getDataAlphabet().toArray()]
    V, K = nw.shape
    out = []
    for k in range(K):
        col = nw[:, k].astype(np.int64)
        order = np.lexsort((np.arange(V), -col))
        order = order[col[order] > 0]
        order = order[:max(0, min(num_words - 1, len(order)))]      # Mallet prints numWords - 1
        if nl:
            out.append(f"{k}\t{format_double(alpha[k], 1)}\n")
            out += [f"{names[w]}\t{format_double(float(col[w]), 1)}\n" for w in order]
        else:
            out.append(f"{k}\t{format_double(alpha[k], 1)}\t" + "".join(f"{names[w]} " for w in order) + "\n")
    return "".join(out)


def test_display_top_words_text_on_both_sides_of_the_cap():
    """numWords - 1 = 0, 1, 7, 64 (the device route, at its cap), 65 and 199
    (the host route over the whole table): the same bytes as the restatement."""
    c = _corpus(_lengths(6), 300, 9)
    m, il = _model(c, 20, 10.0)
    for num_words in (1, 2, 8, 65, 66, 200):
        for nl in (False, True):
            assert m.displayTopWords(num_words, nl) == _top_words_text(m, il, num_words, nl), (num_words, nl)
    m.close()


# -------------------------------------------------------- document readouts
ALPHAS = {
    "symmetric": lambda K: np.full(K, 0.5),
    # distinct values over two decades, in no order of the topic id
    "asymmetric": lambda K: 0.02 + 2.0 * np.random.default_rng(K).permutation(K) / K,
}
_shards = {}


def _shard(K, kind):
    """One sampler per (K, alpha) after 2 sweeps with its nd rows (computed
    once, shared, never changed)."""
    if (K, kind) not in _shards:
        from ldagibbssampling_amd.sampler import GibbsSampler
        c = _corpus(_lengths(17), 200, 3)
        alpha = ALPHAS[kind](K)
        g = GibbsSampler(K, c.num_types, c.doc_off, c.words, alpha, 0.01, seed=9, sampler=_sampler_kind(K))
        g.sweep(2)
        nd = g.counts(with_nd=True)[2]
        nd.setflags(write=False)
        _shards[(K, kind)] = (g, c, alpha, nd)
    return _shards[(K, kind)]


@pytest.mark.parametrize("kind", list(ALPHAS))
@pytest.mark.parametrize("K", [20, 100, 512, 2048])
def test_doc_top_topics_against_numpy(K, kind):
    g, c, alpha, nd = _shard(K, kind)
    D = c.num_docs
    lens = np.diff(c.doc_off)
    assert {0, 1, 65, 150} <= set(lens.tolist())
    A = _seq_sum(alpha)
    rng = np.random.default_rng(K)
    ids = rng.permutation(D)[:D - 3]
    ids[5] = ids[0]                                  # a permuted subset with a duplicate
    for m in (1, 5, 64):                             # m = 64 > K = 20: slots past K fill
        topics, cnt = g.doc_top_topics(m)
        et, ec = expected_top_topics(nd, lens, alpha, A, m)
        np.testing.assert_array_equal(topics, et)
        np.testing.assert_array_equal(cnt, ec)
        if m > K:
            assert np.all(topics[:, K:] == -1) and np.all(cnt[:, K:] == 0) and np.all(topics[:, :K] >= 0)
        # a document's row is the same bytes whatever list it was asked in
        lt, lc = g.doc_top_topics(m, docs=ids)
        assert lt.tobytes() == et[ids].tobytes() and lc.tobytes() == ec[ids].tobytes()
        st, sc = g.doc_top_topics(m, doc_begin=7, num_docs=D - 12)
        assert st.tobytes() == et[7:D - 5].tobytes() and sc.tobytes() == ec[7:D - 5].tobytes()
        one = g.doc_top_topics(m, docs=[int(ids[3])])
        assert one[0].tobytes() == et[ids[3]].tobytes()
    # the empty document ranks by alpha alone; documents with fewer than 5
    # topics are filled in alpha order (ascending id when alpha is uniform)
    empty = int(np.flatnonzero(lens == 0)[0])
    t5 = g.doc_top_topics(5, docs=[empty])[0][0]
    assert t5.tolist() == np.lexsort((np.arange(K), -alpha))[:5].tolist()
    assert np.any((nd > 0).sum(axis=1) < 5)


@pytest.mark.parametrize("K", [20, 2048])
def test_doc_counts_against_counts(K):
    g, c, alpha, nd = _shard(K, "asymmetric")
    D = c.num_docs
    np.testing.assert_array_equal(g.doc_counts(), nd)
    ids = np.random.default_rng(1).permutation(D)[:D - 2]
    ids[4] = ids[1]
    np.testing.assert_array_equal(g.doc_counts(docs=ids), nd[ids])
    np.testing.assert_array_equal(g.doc_counts(doc_begin=3, num_docs=10), nd[3:13])
    assert g.doc_counts(docs=ids).tobytes() == g.doc_counts(docs=ids).tobytes()


def _document_topics_text(m, corpus, nd, threshold, mx):
    from ldagibbssampling_amd.topic_model import format_double
    alpha, alpha_sum, K = m.alpha, m.alphaSum, m.numTopics
    if mx < 0 or mx > K:
        mx = K
    out = ["#doc source topic proportion ...\n"]
    k = np.arange(K)
    for d in range(corpus.num_docs):
        out.append(f"{d} null-source ")
        L = int(corpus.doc_off[d + 1] - corpus.doc_off[d])
        w = (alpha + nd[d]) / (float(L) + alpha_sum)
        for t in np.lexsort((k, -w))[:mx]:
            if w[t] < threshold:
                break
            out.append(f"{t} {format_double(w[t], 0)} ")
        out.append(" \n")
    return "".join(out)


@pytest.mark.parametrize("kind", list(ALPHAS))
def test_model_document_readouts_on_one_and_three_shards(kind):
    """ldatm_doc_top_topics / ldatm_doc_counts / getTopicProbabilities /
    documentTopics against numpy on topicAssignments(), 1 and 3 shards."""
    K = 100
    c = _corpus(_lengths(23), 150, 12)
    D = c.num_docs
    lens = np.diff(c.doc_off)
    alpha = None if kind == "symmetric" else ALPHAS[kind](K)
    models = [_model(c, K, 50.0, devices=dev, alpha=alpha)[0] for dev in (None, [0, 0, 0])]
    assert [m.numShards() for m in models] == [1, 3]
    nd = _model_nd(models[0], c)
    rng = np.random.default_rng(2)
    ids = rng.permutation(D)[:D - 4]
    ids[2] = ids[9]
    for m in models:
        np.testing.assert_array_equal(_model_nd(m, c), nd)          # sharding does not change z
        a, A = m.alpha, m.alphaSum
        np.testing.assert_array_equal(m.docCounts(), nd)
        np.testing.assert_array_equal(m.docCounts(ids), nd[ids])
        for n in (1, 5, 64):
            et, ec = expected_top_topics(nd, lens, a, A, n)
            for docs, sel in ((None, slice(None)), (ids, ids)):
                t, cnt = m.docTopTopics(n, docs)
                assert t.tobytes() == et[sel].tobytes() and cnt.tobytes() == ec[sel].tobytes()
        t, w = m.topTopics(ids, n=5)
        et, ec = expected_top_topics(nd, lens, a, A, 5)
        np.testing.assert_array_equal(t, et[ids])
        np.testing.assert_array_equal(w, (a[et[ids]] + ec[ids]) / (lens[ids].astype(np.float64) + A)[:, None])
        # getTopicProbabilities: its own arithmetic, the sequential sum included
        for d in (0, int(np.flatnonzero(lens == 0)[0]), D - 1):
            dist = nd[d].astype(np.float64) + a
            s = 0.0
            for v in dist:
                s += float(v)
            assert m.getTopicProbabilities(d).tobytes() == (dist / s).tobytes()
        for threshold, mx in ((0.0, -1), (0.0, 3), (0.05, 10), (0.0, 100)):
            assert m.documentTopics(threshold, mx) == _document_topics_text(m, c, nd, threshold, mx), (threshold, mx)
    for m in models:
        m.close()


def test_document_topics_when_alpha_sum_is_not_the_sum_of_alpha():
    """The constructor's alphaSum / K * K need not give alphaSum back: with a
    uniform alpha the device order still is the host's; with a non-uniform
    alpha whose stated sum holds other bits the text comes from the count
    rows.  Either way it is the restatement's bytes."""
    K = 20
    c = _corpus(_lengths(31), 90, 14)
    m, _ = _model(c, K, 1.0)
    assert _seq_sum(m.alpha) != m.alphaSum          # 20 x 0.05 added in order is not 1.0
    nd = _model_nd(m, c)
    for threshold, mx in ((0.0, 3), (0.05, 10), (0.0, -1)):
        assert m.documentTopics(threshold, mx) == _document_topics_text(m, c, nd, threshold, mx)
    a = ALPHAS["asymmetric"](K)
    assert m._L.ldatm_set_hyper(m._h, a.ctypes.data, float(np.nextafter(_seq_sum(a), 9.0)), 0.01) == 0
    for threshold, mx in ((0.0, 3), (0.05, 10)):
        assert m.documentTopics(threshold, mx) == _document_topics_text(m, c, nd, threshold, mx)
    m.close()


# ---------------------------------------------------------------- estimate
def test_estimate_is_the_same_with_the_display_on_off_or_silent(capfd):
    """setTopicDisplay(5, 7) silent and verbose, and setTopicDisplay(0, 0):
    the same z, alpha and beta bits, with an optimisation that fires."""
    c = _corpus(_lengths(41, n=60), 120, 15)
    results = []
    for display, verbosity in (((5, 7), 0), ((5, 7), 1), ((0, 0), 0)):
        m, _ = _model(c, 20, 10.0, iters=20, setOptimizeInterval=5, setBurninPeriod=5, setSaveSampleInterval=1,
                      setTopicDisplay=display, setVerbosity=verbosity)
        results.append((m.topicAssignments().tobytes(), m.alpha.tobytes(), m.alphaSum, m.beta))
        assert not np.allclose(m.alpha, 0.5) and m.beta != 0.01        # the optimisation did move them
        m.close()
        err = capfd.readouterr().err
        # the topics are shown before sweeps 5, 10, 15 and 20 when verbose only
        assert (err.count("\n0\t") >= 4) == (verbosity == 1 and display[0] == 5)
    assert results[0] == results[1] == results[2]


# ------------------------------------------------------------------ errors
def test_readout_errors():
    from ldagibbssampling_amd.sampler import GibbsSampler
    K = 20
    c = _corpus(_lengths(1, n=12), 60, 2)
    D = c.num_docs
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.5), 0.01, seed=3) as g:
        # lda_create leaves the shard's counts as the pending delta
        for call in (lambda: g.top_words(3), lambda: g.doc_top_topics(3), lambda: g.doc_counts()):
            with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
                call()
            assert e.value.status == -4
        g.sweep(1)
        out = np.zeros(K * 65, np.int32)
        p = out.ctypes.data
        for n in (0, 65):
            assert g._L.lda_top_words(g._h, n, p, p) == -1 and b"LDA_TOP_WORDS_MAX" in g._L.lda_last_error()
            assert g._L.lda_doc_top_topics(g._h, n, 0, 1, None, p, p) == -1
            assert b"LDA_TOP_TOPICS_MAX" in g._L.lda_last_error()
        assert g._L.lda_top_words(g._h, 1, None, p) == -1 and b"null" in g._L.lda_last_error()
        assert g._L.lda_doc_counts(g._h, 0, 1, None, None) == -1 and b"null" in g._L.lda_last_error()
        one = np.array([1], np.int64)
        assert g._L.lda_doc_counts(g._h, 1, 1, one.ctypes.data, p) == -1 and b"doc_begin" in g._L.lda_last_error()
        for call in (lambda: g.doc_top_topics(3, docs=[0, D]), lambda: g.doc_counts(docs=[-1])):
            with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*document id"):
                call()
        for call in (lambda: g.doc_top_topics(3, doc_begin=1, num_docs=D), lambda: g.doc_counts(doc_begin=D + 1, num_docs=0)):
            with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*range"):
                call()
        # M = 0 succeeds and touches nothing (NULL outputs are not read)
        assert g.doc_counts(docs=[]).shape == (0, K)
        assert g.doc_top_topics(4, doc_begin=D, num_docs=0)[0].shape == (0, 4)
        assert g._L.lda_doc_counts(g._h, 0, 0, None, None) == 0
        assert g._L.lda_doc_top_topics(g._h, 2, 0, 0, None, None, None) == 0
        # a pending delta again: sample() without apply()
        g.sample()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.top_words(3)
        g.apply()
        assert g.top_words(3)[0].shape == (K, 3)
