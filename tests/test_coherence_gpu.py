"""GPU checks of reference-corpus coherence: lda_word_cooccurrences (k_cooc),
its ldatm_ mirror, ParallelTopicModel.wordCooccurrences and getCoherence.

Every count is compared with array_equal against the brute-force restatement
in coherence_numpy.py (units enumerated, set membership); the coherence values
against ldatm_coherence_finish of the restated counts, bit for bit (the same
host function over equal integers).

The corpus: 300 documents over V = 300 -- test_readout_gpu._lengths' mix (0, 1,
64, 65 and 150 tokens among lengths of 2 .. 40), the planted lengths W - 1, W,
W + 1, 63 + W and 64 + W for W = 1, 2, 10, 64, 65 (a window tile is 64 starts:
these are one start short of a window, one window, two starts, one full tile
and one tile plus a start) and one document of 300 tokens for W = 256.  Words
repeat within a document (42 frequent words take half the tokens); about 5 % of
the host corpus' tokens are -1.

Geometry the shapes reach: a block of k_cooc holds min(K, 65536 / (32 (n + 1)
+ 2 n (n + 1))) topics.  (K, n) = (20, 64): 6 topics a group, four groups, the
last of 2; (100, 20): 43 a group, three groups, the last of 14; (512, 7): 178 a
group, three groups, the last of 156; (2048, 10): 114 a group, 18 groups, the
last of 110; (2048, 1): 963 a group, three groups, the last of 122.  One group
alone: K = 20 with n = 7 or 10 (the chunk, state and model tests).  A block has
4 waves; in document mode a wave takes 64 documents (five tiles here, the last
of 44), in window mode a document at a time, 64 window starts a pass.

The lists: topic k draws from a pool of 40 frequent words (30 of them at most,
the rest of a longer list from the other words), so most listed words stand in
many lists; word 40 stands in every list at slot k mod n (at n = 1 in every
second list: one slot a list, and every list the same would test nothing) and
word 41 in min(K - 1, 65) lists; every fifth list has -1 in the middle and list 7
is all -1."""
import numpy as np
import pytest

import coherence_numpy as N
from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu

V300 = 300
WINDOWS = (0, 1, 2, 10, 64, 65, 110, 256)
POOL, EVERY, SOME = 40, 40, 41
SHAPES = [(20, 64), (100, 20), (512, 7), (2048, 10), (2048, 1)]


# ------------------------------------------------------------------ helpers
def _lengths(seed, n):
    """test_readout_gpu._lengths: an empty document, a one-token one, one
    wave's 64 lanes, 65, several passes, among ordinary ones, shuffled."""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 64, 65, 150]
    lens = np.array(fixed + rng.integers(2, 40, n - len(fixed)).tolist(), np.int64)
    rng.shuffle(lens)
    return lens


def _words(rng, tokens):
    """Half the tokens from the 42 frequent words, half from all of V."""
    w = rng.integers(0, V300, tokens)
    hot = rng.random(tokens) < 0.5
    w[hot] = rng.integers(0, POOL + 2, int(hot.sum()))
    return w.astype(np.int32)


def _corpora():
    """(train, host): the same 300 documents; host with about 5 % of -1."""
    rng = np.random.default_rng(2026)
    planted = [W + d for W in (1, 2, 10, 64, 65) for d in (-1, 0, 1, 63, 64)] + [300]
    lens = np.concatenate([_lengths(11, V300 - len(planted)), np.array(planted, np.int64)])
    rng.shuffle(lens)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = _words(rng, int(off[-1]))
    out = words.copy()
    out[rng.random(len(out)) < 0.05] = -1
    return Corpus(off, words, V300), Corpus(off, out, V300)


def _some_topics(K, n):
    """The (at most 65) topics whose lists hold word 41: not list 7, which is
    empty, and at n = 1 not the lists that hold word 40."""
    return [k for k in range(1 if n == 1 else 0, K, 2 if n == 1 else 1) if k != 7][:65]


def _lists(K, n, seed):
    rng = np.random.default_rng(seed)
    ids = np.full((K, n), -1, np.int32)
    m = min(n, 30)
    for k in range(K):
        row = np.concatenate([rng.permutation(POOL)[:m], SOME + 1 + rng.permutation(V300 - SOME - 1)[:n - m]])
        ids[k] = rng.permutation(row)
        if k % 5 == 2 and n >= 3:
            ids[k, n // 2] = -1
    for k in range(K):
        if n > 1 or k % 2 == 0:
            ids[k, k % n] = EVERY
    for k in _some_topics(K, n):
        ids[k, (k + 1) % n] = SOME
    ids[7] = -1
    return ids


def _sampler(K, c):
    from ldagibbssampling_amd.sampler import GibbsSampler
    kind = "sparse" if K > capi.MAX_TOPICS_DENSE else "dense"
    return GibbsSampler(K, V300, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=K + 1, sampler=kind)


@pytest.fixture(scope="module")
def corpora():
    return _corpora()


@pytest.fixture(scope="module")
def host_presence(corpora):
    """The restatement's units of the host corpus, once per window; read-only."""
    _, host = corpora
    return {W: N.presence(host.doc_off, host.words, W) for W in WINDOWS}


def _short(c, longest):
    """The documents of at most `longest` tokens, as a corpus."""
    keep = np.nonzero(np.diff(c.doc_off) <= longest)[0]
    return c.subset(keep)


# ------------------------------------------------------------ the sampler ABI
def test_the_corpus_and_the_lists_are_what_the_docstring_says(corpora):
    train, host = corpora
    lens = np.diff(host.doc_off)
    assert len(lens) == 300 and {0, 1, 64, 65, 150, 300} <= set(lens.tolist())
    for W in (1, 2, 10, 64, 65):
        assert {W - 1, W, W + 1, 63 + W, 64 + W} <= set(lens.tolist())
    assert 0.03 < (host.words < 0).mean() < 0.07 and (train.words >= 0).all()
    # documents repeat words
    d = int(np.argmax(lens == 150))
    doc = train.words[train.doc_off[d]:train.doc_off[d + 1]]
    assert len(np.unique(doc)) < len(doc)
    for K, n in SHAPES:
        ids = _lists(K, n, K + n)
        assert (ids[7] == -1).all()
        for k in range(K):
            live = ids[k][ids[k] >= 0]
            assert len(np.unique(live)) == len(live)
        assert (ids == SOME).sum() == len(_some_topics(K, n)) == min(65, K - 1)
        if n > 1:
            assert all(ids[k, k % n] == EVERY for k in range(K) if k != 7)
        if n >= 3:
            assert any((row[1:-1] == -1).any() and (row >= 0).any() for row in ids)
        live = ids[(ids >= 0) & (ids < POOL)]
        assert n == 1 or np.bincount(live, minlength=POOL).min() > 1      # every pool word in many lists


@pytest.mark.parametrize("K,n", SHAPES)
def test_counts_equal_the_restatement(K, n, corpora, host_presence):
    train, host = corpora
    ids = _lists(K, n, K + n)
    T = n * (n + 1) // 2
    i, j = np.tril_indices(n)
    with _sampler(K, train) as g:
        for W in WINDOWS:
            want, units = N.cooccurrences(ids, host.doc_off, host.words, W, host_presence[W])
            cooc, u = g.word_cooccurrences(ids, W, host.doc_off, host.words)
            assert cooc.dtype == np.int64 and cooc.shape == (K, T)
            assert u == units
            np.testing.assert_array_equal(cooc, want)
            assert np.all(cooc[(ids[:, i] < 0) | (ids[:, j] < 0)] == 0)      # cells of empty slots
            if W == 1:
                # one token a unit: no pair, the diagonals are the term frequencies
                assert u == host.num_tokens and not cooc[:, i != j].any()
                tf = np.bincount(host.words[host.words >= 0], minlength=V300)
                np.testing.assert_array_equal(cooc[:, i == j], np.where(ids >= 0, tf[np.maximum(ids, 0)], 0))
            if W == 10:
                again = g.word_cooccurrences(ids, W, host.doc_off, host.words)
                assert again[0].tobytes() == cooc.tobytes() and again[1] == u
                if n > 1:
                    assert cooc[:, i != j].any(), "no off-diagonal cell is positive"
        # a window at least as long as the longest document counts the documents themselves
        short = _short(host, 110)
        assert 65 < int(np.diff(short.doc_off).max()) <= 110
        doc_mode = g.word_cooccurrences(ids, 0, short.doc_off, short.words)
        np.testing.assert_array_equal(doc_mode[0], N.cooccurrences(ids, short.doc_off, short.words, 0)[0])
        for W in (110, 256):
            win = g.word_cooccurrences(ids, W, short.doc_off, short.words)
            assert win[1] == doc_mode[1] and win[0].tobytes() == doc_mode[0].tobytes()
        # the shard's own documents equal the same corpus passed from the host
        for W in (0, 10):
            own = g.word_cooccurrences(ids, W)
            passed = g.word_cooccurrences(ids, W, train.doc_off, train.words)
            assert own[1] == passed[1] and own[0].tobytes() == passed[0].tobytes()
        np.testing.assert_array_equal(own[0], N.cooccurrences(ids, train.doc_off, train.words, 10)[0])
        # two corpora's results add: the first 100 documents and the rest
        a = host.subset(np.arange(100))
        b = host.subset(np.arange(100, 300))
        ca, cb = (g.word_cooccurrences(ids, 10, c.doc_off, c.words) for c in (a, b))
        whole = g.word_cooccurrences(ids, 10, host.doc_off, host.words)
        np.testing.assert_array_equal(ca[0] + cb[0], whole[0])
        assert ca[1] + cb[1] == whole[1]


def test_the_worked_example_on_the_device():
    from test_coherence import EX_IDS, EX_WANT, example_corpus
    from ldagibbssampling_amd.sampler import GibbsSampler
    off, words = example_corpus()
    train = np.where(words < 0, 3, words).astype(np.int32)
    with GibbsSampler(2, 4, off, train, np.full(2, 0.5), 0.01, seed=1) as g:
        for W, (units, t0, t1) in EX_WANT.items():
            cooc, u = g.word_cooccurrences(EX_IDS, W, off, words)
            assert u == units and cooc.tolist() == [t0, t1], W
        # no documents at all, and only empty ones: zeros
        for o in ([0], [5, 5, 5]):
            cooc, u = g.word_cooccurrences(EX_IDS, 2, np.array(o, np.int64), words)
            assert u == 0 and not cooc.any()


def test_chunks_do_not_change_the_result(corpora):
    """The hook bounds a chunk's tokens.  At 1 every document with a token
    starts a chunk (each longer than the bound, so each goes alone).  Over
    documents of 20 tokens a bound of 20 starts a chunk at every document and
    60 at every third; the document of 150 tokens among them goes alone."""
    train, host = corpora
    K, n = 20, 7
    ids = _lists(K, n, 5)
    rng = np.random.default_rng(4)
    lens = np.full(31, 20, np.int64)
    lens[13] = 150
    off = np.zeros(32, np.int64)
    np.cumsum(lens, out=off[1:])
    even = Corpus(off, np.where(rng.random(int(off[-1])) < 0.05, -1, _words(rng, int(off[-1]))).astype(np.int32),
                  V300)
    with _sampler(K, train) as g:
        L = g._L
        try:
            for c, bounds in ((host, (1,)), (even, (20, 60))):
                for W in (0, 10):
                    L.lda_debug_cooc_chunk_tokens(0)
                    whole = g.word_cooccurrences(ids, W, c.doc_off, c.words)
                    np.testing.assert_array_equal(whole[0], N.cooccurrences(ids, c.doc_off, c.words, W)[0])
                    for bound in bounds:
                        L.lda_debug_cooc_chunk_tokens(bound)
                        cut = g.word_cooccurrences(ids, W, c.doc_off, c.words)
                        assert cut[1] == whole[1] and cut[0].tobytes() == whole[0].tobytes(), (W, bound)
        finally:
            L.lda_debug_cooc_chunk_tokens(0)


def test_a_call_between_sample_and_apply_leaves_the_state_alone(corpora):
    train, host = corpora
    K, n = 20, 10
    ids = _lists(K, n, 9)
    with _sampler(K, train) as g:
        # lda_create leaves the shard's counts as the pending delta: not an error here
        first = g.word_cooccurrences(ids, 10)
        g.sweep(2)
        z, check = g.z(), g.counts_checksum()
        g.sample()
        z_pending = g.z()
        got = g.word_cooccurrences(ids, 10)
        host_got = g.word_cooccurrences(ids, 0, host.doc_off, host.words)
        np.testing.assert_array_equal(g.z(), z_pending)
        g.apply()
        g2 = g.counts_checksum()
        assert got[0].tobytes() == first[0].tobytes() and got[1] == first[1]
        np.testing.assert_array_equal(host_got[0], N.cooccurrences(ids, host.doc_off, host.words, 0)[0])
    # the same chain without the calls ends in the same state
    with _sampler(K, train) as g:
        g.sweep(2)
        assert g.counts_checksum() == check
        np.testing.assert_array_equal(g.z(), z)
        g.sample()
        g.apply()
        assert g.counts_checksum() == g2


def test_sampler_errors(corpora):
    train, host = corpora
    K, V = 20, V300
    with _sampler(K, train) as g:
        L, h = g._L, g._h
        ids = np.full((K, 3), -1, np.int32)
        ids[:, 0] = np.arange(K)
        out = np.zeros(K * 6, np.int64)
        off = np.array([0, 2, 2, 5], np.int64)
        words = np.array([0, -1, 299, 3, 3], np.int32)
        p, good = out.ctypes.data, ids.ctypes.data

        def call(n=3, lists=good, window=0, Dh=3, o=off.ctypes.data, w=words.ctypes.data, c=p, u=p):
            return L.lda_word_cooccurrences(h, n, lists, window, Dh, o, w, c, u)

        def failed(status, word):
            return status == -1 and word in L.lda_last_error()

        assert call() == 0
        for n in (0, 65):
            assert failed(call(n=n), b"LDA_DIAG_WORDS_MAX")
        assert failed(call(lists=None), b"null word_ids")
        for bad in (-2, V):
            b = ids.copy()
            b[7, 2] = bad
            assert failed(call(lists=b.ctypes.data), b"outside [-1, V)")
        b = ids.copy()
        b[7, 2] = 7
        assert failed(call(lists=b.ctypes.data), b"twice")
        assert failed(call(c=None), b"null output")
        assert failed(call(u=None), b"null output")
        for bad in (-1, 257):
            assert failed(call(window=bad), b"LDA_COOC_WINDOW_MAX")
        assert failed(call(Dh=-1), b"bad sizes")
        assert failed(call(o=np.array([0, 3, 2, 5], np.int64).ctypes.data), b"doc_off not monotone")
        assert failed(call(w=None), b"words is null")
        for bad in (-2, V):
            w = words.copy()
            w[1] = bad
            assert failed(call(w=w.ctypes.data), b"out of range [-1, V)")
        units = np.zeros(1, np.int64)
        assert call(Dh=0, u=units.ctypes.data) == 0 and units[0] == 0 and not out.any()


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


def _reference(model, c):
    from ldagibbssampling_amd import topic_model as tm
    il = tm.InstanceList(model.alphabet)
    for d in range(c.num_docs):
        il.add(tm.Instance(c.doc(d)))
    return il


def test_model_counts_on_one_and_three_shards(corpora, host_presence):
    train, host = corpora
    K, n = 20, 10
    ids = _lists(K, n, 21)
    m1 = _model(train, K)
    m3 = _model(train, K, devices=[0, 0, 0])
    try:
        assert m1.numShards() == 1 and m3.numShards() == 3
        ref = _reference(m1, host)
        for W in (0, 10):
            a, b = m1.wordCooccurrences(ids, W), m3.wordCooccurrences(ids, W)
            assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes()
            np.testing.assert_array_equal(a[0], N.cooccurrences(ids, train.doc_off, train.words, W)[0])
            a, b = m1.wordCooccurrences(ids, W, ref), m3.wordCooccurrences(ids, W, ref)
            assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes()
            want, units = N.cooccurrences(ids, host.doc_off, host.words, W, host_presence[W])
            assert a[1] == units
            np.testing.assert_array_equal(a[0], want)
        # counting only under the topic gives a subset of the documents
        top = m1.topWords(n)[0]
        np.testing.assert_array_equal(top, m3.topWords(n)[0])
        anyz, underz = m1.wordCooccurrences(top, 0)[0], m1.topicCodocuments(top)[0]
        assert (anyz >= underz).all() and (anyz > underz).any()
    finally:
        m1.close()
        m3.close()


def test_get_coherence_equals_finish_of_the_restated_counts(corpora, host_presence, tmp_path):
    from ldagibbssampling_amd import topic_model as tm
    train, host = corpora
    K, n = 20, 10
    m = _model(train, K)
    try:
        ref = _reference(m, host)
        ids = m.topWords(n)[0]
        results = {}
        for measure, window in (("u_mass", 0), ("c_uci", 10), ("c_npmi", 10)):
            want, units = N.cooccurrences(ids, host.doc_off, host.words, window, host_presence[window])
            sums, pairs = tm.coherence_finish(measure, want, units)
            r = m.getCoherence(measure, n, reference=ref)           # window None: the measure's customary one
            assert r.window == window and r.units == units
            np.testing.assert_array_equal(r.wordIds, ids)
            np.testing.assert_array_equal(r.cooc, want)
            np.testing.assert_array_equal(r.pairs, pairs)
            assert r.sums.tobytes() == sums.tobytes()
            assert r.values.tobytes() == np.where(pairs > 0, sums / np.maximum(pairs, 1), 0.0).tobytes()
            assert r.mean == float(r.values[pairs > 0].mean())
            assert r.topWords[3] == [int(w) for w in ids[3] if w >= 0]
            # and the restatement's own formulas, at the CPU test's derived tolerance
            ws, wp, mags = N.finish(measure, want, units)
            logs = 2 if measure == "c_npmi" else 1
            assert np.all(np.abs(r.sums - ws) <= (4 * wp * 2.0 ** -53 + logs * 2.0 ** -52) * mags)
            results[measure] = r
        assert (results["c_npmi"].values <= 1.0 + 1e-9).all() and (results["c_npmi"].values >= -1.0 - 1e-9).all()
        # an explicit window and epsilon, on the training corpus
        r = m.getCoherence("c_uci", n, window=0, epsilon=0.5)
        want, units = N.cooccurrences(ids, train.doc_off, train.words, 0)
        np.testing.assert_array_equal(r.cooc, want)
        assert r.sums.tobytes() == tm.coherence_finish("c_uci", want, units, epsilon=0.5)[0].tobytes()
        # a saved and loaded model gives the same coherence against a host reference
        path = str(tmp_path / "model.bin")
        m.save(path)
        loaded = tm.ParallelTopicModel.load(path)
        try:
            r2 = loaded.getCoherence("c_npmi", n, reference=ref)
            r1 = results["c_npmi"]
            assert r2.values.tobytes() == r1.values.tobytes() and r2.cooc.tobytes() == r1.cooc.tobytes()
            assert r2.units == r1.units
        finally:
            loaded.close()
    finally:
        m.close()


def test_after_fifty_sweeps_every_pair_of_top_words_is_kept(corpora):
    """The top words of a trained topic occur in the training corpus, so in
    document mode on that corpus D(i) > 0 for every non-empty slot, and u_mass
    keeps every pair."""
    train, _ = corpora
    K, n = 20, 10
    m = _model(train, K, iters=50)
    try:
        r = m.getCoherence("u_mass", n)
        live = (r.wordIds >= 0).sum(1)
        assert r.window == 0 and r.units == int((np.diff(train.doc_off) > 0).sum())
        np.testing.assert_array_equal(r.pairs, live * (live - 1) // 2)
        assert (live > 1).all() and np.isfinite(r.values).all() and (r.values < 0).any()
    finally:
        m.close()
