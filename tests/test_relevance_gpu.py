"""GPU checks of lda_relevant_words (k_word_totals + k_relevant_slab<B> +
k_relevant_merge), lda_salient_words (k_salient_slab + k_salient_merge),
lda_word_rows (k_word_rows), their ldatm_ mirrors and prepareVis.

Every expectation is the numpy restatement (relevance_numpy) on the counts of
the same context.  Integer outputs (ids, counts, totals) are compared exactly;
logprob, loglift, saliency and distinctiveness within TOL = 1e-9, relative:
the device's log is not the host libm's.  For the same reason every order
comparison first asserts, on the numpy side, that the restatement's own
adjacent keys are either from identical inputs or more than 1e-7 apart
(check_key_gaps over all candidates of every topic, check_saliency_gaps over
the top n + 1); a fixture that breaks that fails the test.

Tables are set with lda_set_z + lda_apply from relevance_numpy.fixture (seed
20261021: word ~ 1 / (1 + id), z = word mod K with probability 0.7, else
uniform), beta = 0.01.

Geometry.  V is cut as lda_top_words cuts it: slabs of at least 256 rows, so
V = 203 is one ragged slab (203 mod 8 = 3) and V = 1037 five; the hook's 64
rows make 17 slabs there, the last of 13 rows.  A pass handles
capi.relevance_batch(n) lambdas (8 / 4 / 2 / 1 for n up to 10 / 21 / 42 / 64),
so passes start at multiples of it.  No launcher caps its grid."""
import json

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

import relevance_numpy as N
import topic_distance_numpy as TD

pytestmark = pytest.mark.gpu

TOL = 1e-9
BETA = 0.01
LAMBDAS = [0.0, 0.25, 0.6, 1.0]


# ------------------------------------------------------------------ helpers
def _sampler(words, z, V, K, doc_len=50, seed=5):
    """A context whose global table is exactly (words, z)."""
    from ldagibbssampling_amd.sampler import GibbsSampler
    off = np.append(np.arange(0, len(words), doc_len), len(words)).astype(np.int64)
    g = GibbsSampler(K, V, off, np.ascontiguousarray(words, np.int32), np.full(K, 0.3), BETA, seed=seed,
                     sampler="sparse" if K > capi.MAX_TOPICS_DENSE else "dense")
    g.set_z(np.ascontiguousarray(z, np.int32))
    g.apply()
    return g


def _fixture(V, K, tokens):
    words, z = N.fixture(V, K, tokens)
    nw, nwsum = N.counts_of(words, z, V, K)
    return words, z, nw, nwsum


def _close(got, want, what):
    """got within TOL of want, relative; both exactly 0.0 in the empty slots."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64
    zero = want == 0.0
    assert np.all(got[zero] == 0.0), what
    err = float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero]))) if np.any(~zero) else 0.0
    print(f"{what}: max relative error {err:.3e}")
    assert err <= TOL, (what, err)


def _check_relevant(g, nw, nwsum, n, lambdas, got=None):
    gap = N.check_key_gaps(nw, nwsum, BETA, lambdas)
    print(f"smallest gap between unequal-input adjacent keys: {gap:.3e}")
    got = g.relevant_words(n, lambdas) if got is None else got
    exp = N.expected_relevant(nw, nwsum, BETA, n, lambdas)
    for a, e, name in zip(got[:3], exp[:3], ("ids", "counts", "totals")):
        assert a.dtype == e.dtype and a.shape == e.shape, name
        np.testing.assert_array_equal(a, e, err_msg=name)
    _close(got[3], exp[3], "logprob")
    _close(got[4], exp[4], "loglift")
    return got


def _check_salient(g, nw, nwsum, n, got=None):
    gap = N.check_saliency_gaps(nw, nwsum, n)
    print(f"smallest relative gap among the top {n + 1} saliencies: {gap:.3e}")
    got = g.salient_words(n) if got is None else got
    exp = N.expected_salient(nw, nwsum, n)
    for a, e, name in zip(got[:2], exp[:2], ("ids", "totals")):
        assert a.dtype == e.dtype and a.shape == e.shape, name
        np.testing.assert_array_equal(a, e, err_msg=name)
    _close(got[2], exp[2], "saliency")
    _close(got[3], exp[3], "distinctiveness")
    return got


def _same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def small():
    """Case 1's table: V = 203 (203 mod 8 = 3), K = 5 (Kp = 64: 59 padded topics), 6000 tokens."""
    words, z, nw, nwsum = _fixture(203, 5, 6000)
    g = _sampler(words, z, 203, 5)
    assert capi.padded_topics(5) == 64
    got = g.counts()
    assert np.array_equal(got[0], nw) and np.array_equal(got[1], nwsum)
    yield g, nw, nwsum
    g.close()


@pytest.fixture(scope="module")
def medium():
    """Case 2's table: V = 1037, K = 70 (two 64-topic groups, the second mostly padding), 40 000 tokens."""
    words, z, nw, nwsum = _fixture(1037, 70, 40000)
    g = _sampler(words, z, 1037, 70)
    assert capi.padded_topics(70) == 128
    yield g, nw, nwsum
    g.close()


# ------------------------------------------------------------------- case 1
@pytest.mark.parametrize("n", [1, 7, 64])
def test_relevant_words_small_table_against_numpy(small, n):
    g, nw, nwsum = small
    got = _check_relevant(g, nw, nwsum, n, LAMBDAS)
    assert got[0].shape == (4, 5, n)
    assert np.any(got[0][0] != got[0][3])          # lambda = 0 and lambda = 1 rank differently
    one = g.relevant_words(n)                      # the default, a scalar 0.6
    assert _same_bytes([a[2:3] for a in got], one)


# ------------------------------------------------------------------- case 2
def test_relevant_and_salient_words_do_not_depend_on_the_slabs(medium):
    g, nw, nwsum = medium
    L = capi.load()
    default = _check_relevant(g, nw, nwsum, 7, LAMBDAS)
    sal = _check_salient(g, nw, nwsum, 256)
    try:
        L.lda_debug_relevance_slab_rows(64)        # 17 slabs, the last of 13 rows; salient: chunks of 64 rows
        assert -(-1037 // 64) == 17 and 1037 - 16 * 64 == 13
        cut = g.relevant_words(7, LAMBDAS)
        sal_cut = g.salient_words(256)
        cut64 = g.relevant_words(64, [0.6])
    finally:
        L.lda_debug_relevance_slab_rows(0)
    assert _same_bytes(default, cut)
    assert _same_bytes(sal, sal_cut)
    _check_relevant(g, nw, nwsum, 7, LAMBDAS, got=cut)
    assert _same_bytes(cut64, g.relevant_words(64, [0.6]))
    _check_relevant(g, nw, nwsum, 64, [0.6], got=cut64)


# ------------------------------------------------------------------- case 3
def test_exact_device_to_device(medium):
    g, nw, nwsum = medium
    # the lambda = 1 plane is lda_top_words' order wherever the counts differ: equal counts tie in
    # lda_top_words (by id) and in logprob alike
    for n in (7, 64):
        ids, cnt = g.top_words(n)
        r = g.relevant_words(n, 1.0)
        assert np.array_equal(r[0][0], ids) and np.array_equal(r[1][0], cnt)
    lam = np.linspace(0.0, 1.0, 128)
    for n in (7, 30, 64):
        B = capi.relevance_batch(n)
        assert B == {7: 8, 30: 2, 64: 1}[n]
        full = g.relevant_words(n, lam)
        again = g.relevant_words(n, lam)
        assert _same_bytes(full, again)                                    # two calls, identical bytes
        # planes 0, 1, 63, 64, 127 and the first plane of the second, a middle and the last pass
        starts = sorted({0, 1, 63, 64, 127, B, B * (64 // B), 128 - B})
        assert starts == {8: [0, 1, 8, 63, 64, 120, 127], 2: [0, 1, 2, 63, 64, 126, 127],
                          1: [0, 1, 63, 64, 127]}[B]
        for l in starts:
            single = g.relevant_words(n, lam[l])
            assert _same_bytes([a[l:l + 1] for a in full], single), (n, l)
    # a repeated lambda gives identical planes, wherever it sits
    rep = g.relevant_words(7, [0.6, 0.1, 0.6, 0.3, 0.3, 0.9, 0.0, 1.0, 0.6])
    for a in rep:
        assert a[0].tobytes() == a[2].tobytes() == a[8].tobytes() and a[3].tobytes() == a[4].tobytes()


# ------------------------------------------------------------------- case 4
def test_edges():
    """K = 4, V = 40, 12 words in use.  Topic 0 has 3 candidate words (n = 7:
    a tail of -1 / 0), topic 3 no token (all -1), words 12 .. 39 no token
    (nowhere, and not salient either), words 5 and 9 one row: 5 comes first
    under every lambda."""
    cells = [(0, 0, 5), (1, 0, 3), (2, 0, 1),
             (3, 1, 4), (4, 1, 2), (5, 1, 3), (9, 1, 3), (6, 1, 1), (7, 1, 2), (8, 1, 6), (10, 1, 1), (2, 1, 2),
             (5, 2, 2), (9, 2, 2), (3, 2, 1), (8, 2, 1), (11, 2, 7), (0, 2, 1)]
    words = np.concatenate([np.full(c, w) for w, _, c in cells]).astype(np.int32)
    z = np.concatenate([np.full(c, k) for _, k, c in cells]).astype(np.int32)
    V, K, n = 40, 4, 7
    nw, nwsum = N.counts_of(words, z, V, K)
    assert np.array_equal(nw[5], nw[9]) and nwsum[3] == 0 and np.count_nonzero(nw[:, 0]) == 3
    with _sampler(words, z, V, K, doc_len=10) as g:
        ids, cnt, tot, lp, ll = _check_relevant(g, nw, nwsum, n, LAMBDAS)
        assert np.all(ids[:, 0, 3:] == -1) and np.all(ids[:, 0, :3] >= 0) and np.all(cnt[:, 0, 3:] == 0)
        assert np.all(ids[:, 3] == -1) and np.all(tot[:, 3] == 0) and np.all(lp[:, 3] == 0.0)
        assert ids.max() <= 11
        # n = 10 holds every candidate of topic 1 (9 words), where the twins rank 8th and 9th by lift
        ids, cnt, tot, lp, ll = _check_relevant(g, nw, nwsum, 10, LAMBDAS)
        for l in range(len(LAMBDAS)):
            for k in (1, 2):
                row = ids[l, k].tolist()
                assert row.index(9) == row.index(5) + 1
                i = row.index(5)
                assert lp[l, k, i] == lp[l, k, i + 1] and ll[l, k, i] == ll[l, k, i + 1]
        sid, stot, sal, dist = _check_salient(g, nw, nwsum, 30)
        assert np.all(sid[12:] == -1) and sorted(sid[:12].tolist()) == list(range(12))
        i = sid.tolist().index(5)
        assert sid[i + 1] == 9 and sal[i] == sal[i + 1] and dist[i] == dist[i + 1]
        rows, totals = g.word_rows([39, 5, 9, 0])
        assert np.array_equal(rows, nw[[39, 5, 9, 0]]) and totals.tolist() == [0, 5, 5, 6]


# ------------------------------------------------------------------- case 5
def test_relevant_words_at_the_large_k_sampler_kind():
    V, K = 300, 2048
    words, z, nw, nwsum = _fixture(V, K, 20000)
    assert capi.padded_topics(K) == 2048 and K > capi.MAX_TOPICS_DENSE
    with _sampler(words, z, V, K) as g:
        got = _check_relevant(g, nw, nwsum, 5, [0.6])
        assert np.any(got[0] < 0) and np.any(nwsum == 0)     # short and empty topics were compared
        _check_salient(g, nw, nwsum, 30)


# ------------------------------------------------------------------- case 6
@pytest.mark.parametrize("n", [30, 256])
def test_salient_words_small_table(small, n):
    g, nw, nwsum = small
    ids, tot, sal, dist = _check_salient(g, nw, nwsum, n)
    if n > 203:
        assert np.all(ids[:203] >= 0) and np.all(ids[203:] == -1) and np.all(tot[203:] == 0)
        assert np.all(sal[203:] == 0.0) and np.all(dist[203:] == 0.0)
    assert _same_bytes((ids, tot, sal, dist), g.salient_words(n))
    assert _same_bytes([a[:10] for a in (ids, tot, sal, dist)], g.salient_words(10))


def test_word_rows(small):
    g, nw, nwsum = small
    rows, tot = g.word_rows([])
    assert rows.shape == (0, 5) and tot.shape == (0,)
    assert g._L.lda_word_rows(g._h, 0, None, None, None) == 0           # M = 0 touches nothing
    rng = np.random.default_rng(4)
    ids = np.concatenate([rng.permutation(203), rng.integers(0, 203, 150), [7, 7, 7, 202, 0]]).astype(np.int32)
    rows, tot = g.word_rows(ids)
    full = g.counts()[0]
    assert rows.dtype == np.int32 and tot.dtype == np.int64
    assert np.array_equal(rows, full[ids]) and np.array_equal(tot, nw.sum(axis=1)[ids])
    out = np.zeros(8, np.int64)
    bad = np.array([0, 203], np.int32)
    assert g._L.lda_word_rows(g._h, 2, bad.ctypes.data, out.ctypes.data, out.ctypes.data) == -1
    assert b"out of range" in g._L.lda_last_error()
    bad[1] = -1
    assert g._L.lda_word_rows(g._h, 2, bad.ctypes.data, out.ctypes.data, out.ctypes.data) == -1


def test_word_rows_in_chunks_at_k_2048():
    """2^23 / 2048 = 4096 rows a chunk: 8229 ids are two full chunks and a ragged one of 37."""
    V, K = 300, 2048
    words, z, nw, nwsum = _fixture(V, K, 20000)
    assert (1 << 23) // K == 4096 and 8229 == 2 * 4096 + 37
    ids = np.random.default_rng(6).integers(0, V, 8229).astype(np.int32)
    with _sampler(words, z, V, K) as g:
        rows, tot = g.word_rows(ids)
        assert np.array_equal(rows, nw[ids]) and np.array_equal(tot, nw.sum(axis=1)[ids])


# ------------------------------------------------------------------- case 7
def test_state_and_a_long_lived_context():
    V, K = 203, 5
    words, z, nw, nwsum = _fixture(V, K, 1500)
    lam128 = np.linspace(0.0, 1.0, 128)
    with _sampler(words, z, V, K, seed=9) as g:
        _check_relevant(g, nw, nwsum, 1, [0.6])                          # n = 1, L = 1: the smallest scratch
        g.sample()                                                       # a pending delta
        out = np.zeros(64, np.int64)
        p = out.ctypes.data
        lam = np.array([0.6])
        for status in (g._L.lda_relevant_words(g._h, 1, 1, lam.ctypes.data, p, p, p, p, p),
                       g._L.lda_salient_words(g._h, 1, p, p, p, p),
                       g._L.lda_word_rows(g._h, 1, np.zeros(1, np.int32).ctypes.data, p, p)):
            assert status == -4 and b"pending" in g._L.lda_last_error()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE"):
            g.relevant_words(3)
        g.apply()
        top = g.top_words(10)
        nw1, nwsum1 = g.counts()[:2]
        assert not np.array_equal(nw1, nw)                               # the sweep moved the table
        got = _check_relevant(g, nw1, nwsum1, 64, lam128)                # regrown scratch, B = 1
        assert np.array_equal(got[0][127][:, :10], top[0])
        _check_salient(g, nw1, nwsum1, 256)
        g.sweep(1)
        g.top_words(3)
        nw2, nwsum2 = g.counts()[:2]
        _check_relevant(g, nw2, nwsum2, 7, LAMBDAS)                      # smaller again: the scratch is reused
        _check_salient(g, nw2, nwsum2, 30)
        rows, tot = g.word_rows(np.arange(V, dtype=np.int32))
        assert np.array_equal(rows, nw2) and np.array_equal(tot, nw2.sum(axis=1))


# ------------------------------------------------------------------- case 8
def _model(corpus, K, devices=None, iters=4):
    from ldagibbssampling_amd import topic_model as tm
    m = tm.ParallelTopicModel(K, 0.5 * K, BETA)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(iters)
    m.setOptimizeInterval(0)
    if devices is not None:
        m.setDevices(devices)
    m.addInstances(tm.InstanceList.fromCorpus(corpus))
    m.estimate()
    return m


def test_model_faces_on_one_and_two_shards(tmp_path):
    from ldagibbssampling_amd import topic_model as tm
    V, K = 300, 3
    words, _ = N.fixture(V, K, 3000)
    off = np.arange(0, 3001, 30).astype(np.int64)
    c = Corpus(off, words, V)
    m1, m2 = _model(c, K), _model(c, K, devices=[0, 0])
    assert m1.numShards() == 1 and m2.numShards() == 2
    assert m1.topicAssignments().tobytes() == m2.topicAssignments().tobytes()
    nw, nwsum = m1.typeTopicCounts()
    names = None if m1.alphabet is None else [str(w) for w in m1.alphabet.toArray()]
    word = (lambda w: int(w)) if m1.alphabet is None else m1.alphabet.lookupObject
    lam = [0.0, 0.25, 0.5, 0.75, 1.0]
    N.check_key_gaps(nw, nwsum, BETA, lam + [0.6])
    N.check_saliency_gaps(nw, nwsum, 30)
    r1, r2 = m1.relevantWords(10, lam), m2.relevantWords(10, lam)
    planes = lambda r: (r.wordIds, r.counts, r.totals, r.logprob, r.loglift)
    assert _same_bytes(planes(r1), planes(r2)) and np.array_equal(r1.lambdas, lam)
    assert _same_bytes(m1.salientWords(30), m2.salientWords(30))
    assert _same_bytes(m1.wordRows([5, 1, 5, 299]), m2.wordRows([5, 1, 5, 299]))
    js = TD.topic_distances(nw, nwsum, BETA, metric="jensen_shannon")
    for m in (m1, m2):
        r = m.relevantWords(10, lam)
        exp = N.expected_relevant(nw, nwsum, BETA, 10, lam)
        for a, e in zip(planes(r)[:3], exp[:3]):
            assert a.dtype == e.dtype
            np.testing.assert_array_equal(a, e)
        _close(r.logprob, exp[3], "model logprob")
        _close(r.loglift, exp[4], "model loglift")
        # getRelevantWords: lambda 0.6, (word, relevance) with the relevance of the device's planes
        e6 = N.expected_relevant(nw, nwsum, BETA, 10, [0.6])
        got = m.getRelevantWords(10, 0.6)
        assert [[w for w, _ in t] for t in got] == [[word(w) for w in e6[0][0, k] if w >= 0] for k in range(K)]
        rel = e6[3][0] - (1.0 - 0.6) * (e6[3][0] - e6[4][0])
        _close(np.array([[x for _, x in t] for t in got]), rel, "relevance")
        sal = N.expected_salient(nw, nwsum, 30)
        gs = m.getSalientWords(30)
        assert [w for w, _ in gs] == [word(w) for w in sal[0]]
        _close(np.array([x for _, x in gs]), sal[2], "saliency")
        rows, tot = m.wordRows([5, 1, 5, 299])
        assert np.array_equal(rows, nw[[5, 1, 5, 299]]) and np.array_equal(tot, nw.sum(axis=1)[[5, 1, 5, 299]])
        # the text is the format of the model's own arrays
        r6 = m.relevantWords(10, 0.6)
        text = tm.format_relevant_words(r6.wordIds[0], r6.counts[0], r6.totals[0], r6.logprob[0], r6.loglift[0], 0.6,
                                        names)
        assert m.relevantWordsText(10, 0.6) == text and text.count("\n") == 1 + 10 * K
        path = tmp_path / "relevant.txt"
        m.printRelevantWords(path, 10, 0.6)
        assert path.read_text() == text
        assert text.split("\n")[1].split(" ")[:3] == ["0", "0", str(word(e6[0][0, 0, 0]))]
        # prepareVis: every list but x / y (and the device's logs, within TOL) equals the restatement's
        vis = m.prepareVis(R=5, lambdaStep=0.25)
        want = N.expected_vis(nw, nwsum, BETA, 5, 0.25, js, names)
        assert sorted(vis) == sorted(want)
        for key in ("R", "lambda.step", "plot.opts", "topic.order", "token.table"):
            assert vis[key] == want[key], key
        for key in ("topics", "cluster", "Freq"):
            assert vis["mdsDat"][key] == want["mdsDat"][key], key
        for key in ("Term", "Category", "Freq", "Total"):
            assert vis["tinfo"][key] == want["tinfo"][key], key
        ndef = want["tinfo"]["Category"].count("Default")
        assert ndef == 5 and vis["tinfo"]["logprob"][:5] == [5.0, 4.0, 3.0, 2.0, 1.0] == vis["tinfo"]["loglift"][:5]
        _close(np.array(vis["tinfo"]["logprob"]), np.array(want["tinfo"]["logprob"]), "tinfo logprob")
        _close(np.array(vis["tinfo"]["loglift"]), np.array(want["tinfo"]["loglift"]), "tinfo loglift")
        x, y = np.array(vis["mdsDat"]["x"]), np.array(vis["mdsDat"]["y"])
        err = float(np.max(np.abs(N.pairwise(x, y) - N.pairwise(want["mdsDat"]["x"], want["mdsDat"]["y"]))))
        print(f"2-D pairwise distances: max abs difference {err:.3e}")
        assert err <= 1e-9
        order = [k - 1 for k in vis["topic.order"]]
        back = np.argsort(order)
        for a in (x[back], y[back]):                      # the sign rule, in topic-id order
            assert np.all(a == 0.0) or a[int(np.argmax(np.abs(a)))] > 0
        path = tmp_path / "vis.json"
        m.saveVis(path, R=5, lambdaStep=0.25)
        assert json.load(open(path)) == json.loads(json.dumps(vis))
    m1.close()
    m2.close()
