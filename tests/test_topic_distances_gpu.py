"""GPU checks of lda_topic_distances (k_topic_sums, k_topic_pairs,
k_topic_dist_final), lda_topic_nearest (k_topic_nearest), their ldatm_ mirrors
and the Python faces, against the numpy restatement in topic_distance_numpy.py
computed from counts().

Tolerance: absolute 1e-9 on cosine, Jensen-Shannon, Kullback-Leibler and the
SQUARE of Hellinger (the root magnifies rounding without bound near 0, so the
distance itself is not compared).  Not a measured number: a sequential fp64 sum
of n <= 3001 terms is off by at most n 2^-53 sum|terms|, and sum|terms| <=
2 ln((N + V beta) / beta) < 40 here, about 1e-11; 1e-9 is 100 times that and
five orders below the smallest effect of a dropped or doubled word row (~1/N).

Slabs (lda_topic_distance_slabs, the rule in lda_mi355x.h): at least 256 rows a
slab, so V = 1 and 7 are one partial slab, V = 300 two slabs of 150, and V = 3001
twelve slabs -- eleven of 251 rows and a ragged one of 240 -- at every K used
with it.  Tiles are 64 x 64 topics: K = 20 and 100 are padded and are a single
partial tile or end in one, 512 and 2048 are several tiles.
"""
import ctypes as C
import math

import numpy as np
import pytest

import topic_distance_numpy as TD
from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu

TOL = 1e-9
METRICS = ("cosine", "hellinger", "jensen_shannon", "kullback_leibler")
SYMMETRIC = ("cosine", "hellinger", "jensen_shannon")
LN2 = math.log(2.0)


# ------------------------------------------------------------------ helpers
def _corpus(lengths, V, seed):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    return Corpus(off, words, V)


def _lengths(seed, n=40):
    """Ragged documents: an empty one, a one-token one, 64, 65 and 150 tokens
    among ordinary ones, shuffled."""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 64, 65, 150]
    lens = np.array(fixed + rng.integers(2, 40, n - len(fixed)).tolist(), np.int64)
    rng.shuffle(lens)
    return lens


def _sampler(K, V, seed, beta=0.05, lengths_seed=None):
    from ldagibbssampling_amd.sampler import GibbsSampler
    c = _corpus(_lengths(K + V if lengths_seed is None else lengths_seed), V, seed)
    g = GibbsSampler(K, V, c.doc_off, c.words, np.full(K, 0.3), beta, seed=K * 7 + V + seed,
                     sampler="sparse" if K > capi.MAX_TOPICS_DENSE else "dense")
    g.sweep(3)
    return g


def _slabs(V, K, K2):
    L = capi.load()
    s, r = C.c_int32(), C.c_int32()
    assert L.lda_topic_distance_slabs(V, K, K2, C.byref(s), C.byref(r)) == 0
    return s.value, r.value


def _rows_to_check(K, K2, V, seed):
    """Every row, or where K K2 V > 1e8 sixteen: the first and last row of the
    first and of the last 64-topic tile and twelve random ones."""
    if K * K2 * V <= 1e8:
        return np.arange(K)
    last = 64 * ((K - 1) // 64)
    fixed = [0, 63, last, K - 1]
    rest = np.setdiff1d(np.arange(K), fixed)
    return np.array(fixed + np.random.default_rng(seed).choice(rest, 12, replace=False).tolist())


def _close(got, want, metric, what):
    """got / want within TOL; Hellinger by its square (want is the squared
    restatement then)."""
    g = got * got if metric == "hellinger" else got
    err = float(np.max(np.abs(g - want))) if g.size else 0.0
    print(f"{what} {metric}: max abs error {err:.3e}")
    assert err <= TOL, (what, metric, err)


def _restate(a, b, metric, rows=None):
    """The restatement for samplers a (rows) and b (columns; None: a)."""
    nw, nwsum = a.counts()[:2]
    if b is None:
        return TD.topic_distances(nw, nwsum, a.beta, metric=metric, rows=rows, squared_hellinger=True)
    nw2, nwsum2 = b.counts()[:2]
    return TD.topic_distances(nw, nwsum, a.beta, nw2, nwsum2, b.beta, metric=metric, rows=rows,
                              squared_hellinger=True)


def _bounds(d, metric):
    if metric == "hellinger":
        assert d.min() >= 0.0 and d.max() <= 1.0
    elif metric == "jensen_shannon":
        assert d.min() >= 0.0 and d.max() <= LN2 + 1e-12
    elif metric == "kullback_leibler":
        assert d.min() >= -1e-12


def _self_mode_structure(d, metric):
    K = d.shape[0]
    diag = d[np.arange(K), np.arange(K)]
    if metric in SYMMETRIC:
        assert d.tobytes() == np.ascontiguousarray(d.T).tobytes(), f"{metric} is not bit-symmetric"
        want = 1.0 if metric == "cosine" else 0.0
        assert np.all(diag == want) and not np.any(np.signbit(diag))
    else:
        assert np.all(diag == 0.0) and not np.any(np.signbit(diag))


# ------------------------------------------------- random states, self mode
@pytest.mark.parametrize("V", [1, 7, 300, 3001])
@pytest.mark.parametrize("K", [20, 64, 100, 512])
def test_self_distances_against_numpy(K, V):
    assert (capi.padded_topics(K) != K) == (K in (20, 100))          # 20 and 100 are padded
    slabs, slab_rows = _slabs(V, K, K)
    if V <= 7:
        assert (slabs, slab_rows) == (1, V)                          # one partial slab
    if V == 3001:
        assert (slabs, slab_rows) == (12, 251) and V - 11 * 251 == 240   # several slabs, a ragged last one
    with _sampler(K, V, 5) as g:
        assert g.counts()[0].sum() == g.N
        rows = _rows_to_check(K, K, V, K + V)
        for metric in METRICS:
            d = g.topic_distances(metric)
            assert d.shape == (K, K) and d.dtype == np.float64 and np.all(np.isfinite(d))
            _close(d[rows], _restate(g, None, metric, rows), metric, f"K={K} V={V}")
            _self_mode_structure(d, metric)
            _bounds(d, metric)
            assert g.topic_distances(metric).tobytes() == d.tobytes()          # repeats bit for bit
            assert g.topic_distances(capi.TOPIC_METRICS[metric], other=g).tobytes() == d.tobytes()
            if V == 1:
                # one word: every topic is the distribution (1.0)
                assert np.all(d == (1.0 if metric == "cosine" else 0.0))


def test_self_distances_at_k_2048_on_the_sparse_sampler():
    K, V = 2048, 300
    assert _slabs(V, K, K) == (2, 150)
    with _sampler(K, V, 11) as g:
        assert g.sampler_kind == "sparse"
        rows = _rows_to_check(K, K, V, 3)
        assert len(rows) == 16 and {0, 63, 1984, 2047} <= set(rows.tolist())
        for metric in METRICS:
            d = g.topic_distances(metric)
            assert d.shape == (K, K)
            _close(d[rows], _restate(g, None, metric, rows), metric, "K=2048 V=300")
            _self_mode_structure(d, metric)
            _bounds(d, metric)
        assert g.topic_distances("kullback_leibler").tobytes() == d.tobytes()


# --------------------------------------------------------- constructed states
def _constructed(K, V, word_topic_count, beta=0.05):
    """A sampler whose z gives nw[w, k] = the given counts (set_z + apply)."""
    from ldagibbssampling_amd.sampler import GibbsSampler
    words, z = [], []
    for (w, k), n in sorted(word_topic_count.items()):
        words += [w] * n
        z += [k] * n
    words = np.array(words, np.int32)
    z = np.array(z, np.int32)
    off = np.append(np.arange(0, len(words), 50), len(words)).astype(np.int64)
    g = GibbsSampler(K, V, off, words, np.full(K, 0.3), beta, seed=1)
    g.set_z(z)
    g.apply()
    exp = np.zeros((V, K), np.int32)
    for (w, k), n in word_topic_count.items():
        exp[w, k] = n
    np.testing.assert_array_equal(g.counts()[0], exp)
    return g


TWINS = (3, 70, 99)            # identical columns, in the first and the second 64-topic tile
ONE_WORD, EMPTY = 5, 6


@pytest.fixture(scope="module")
def constructed():
    K, V = 100, 300
    rng = np.random.default_rng(17)
    cells = {}
    for k in range(K):
        if k in TWINS or k in (ONE_WORD, EMPTY):
            continue
        for w in rng.choice(V, int(rng.integers(1, 30)), replace=False):
            cells[(int(w), k)] = int(rng.integers(1, 9))
    for k in TWINS:
        cells.update({(10, k): 4, (20, k): 2, (150, k): 7, (151, k): 7, (299, k): 1})
    cells[(42, ONE_WORD)] = 30
    g = _constructed(K, V, cells)
    nwsum = g.counts()[1]
    assert nwsum[EMPTY] == 0 and nwsum[ONE_WORD] == 30 and len({int(nwsum[k]) for k in TWINS}) == 1
    yield g
    g.close()


@pytest.mark.parametrize("metric", METRICS)
def test_identical_columns_and_the_determinism_contract(constructed, metric):
    g = constructed
    d = g.topic_distances(metric)
    same = 1.0 if metric == "cosine" else 0.0
    for a in TWINS:
        for b in TWINS:
            assert d[a, b] == same, (a, b, d[a, b])                 # exactly, off the diagonal too
    others = [c for c in range(g.K) if c not in TWINS]
    # a pair's value depends on the two columns alone, not on its place in the matrix
    for t in TWINS[1:]:
        assert d[others, t].tobytes() == d[others, TWINS[0]].tobytes()
        assert d[t, others].tobytes() == d[TWINS[0], others].tobytes()
    _self_mode_structure(d, metric)
    _bounds(d, metric)
    want = _restate(g, None, metric)
    _close(d[EMPTY], want[EMPTY], metric, "empty topic's row")
    _close(d, want, metric, "constructed")
    if metric != "cosine":
        # the one-word topic (phi = 0.668 on its word) against the empty, uniform one: by hand
        # Hellinger 0.62, Jensen-Shannon 0.31, KL 3.2 one way and 1.1 the other
        assert d[ONE_WORD, EMPTY] > 0.25 and d[EMPTY, ONE_WORD] > 0.25
    if metric == "kullback_leibler":
        assert d[ONE_WORD, EMPTY] > 2.0 * d[EMPTY, ONE_WORD]


# ------------------------------------------------------------------ cross mode
@pytest.fixture(scope="module")
def pair():
    a = _sampler(100, 300, 21, beta=0.05, lengths_seed=1)
    b = _sampler(512, 300, 22, beta=0.01, lengths_seed=2)
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("metric", METRICS)
def test_cross_distances_against_numpy(pair, metric):
    a, b = pair
    assert _slabs(300, 100, 512) == (2, 150)
    before = (b.counts()[0].tobytes(), b.counts()[1].tobytes(), b.z().tobytes())
    ab = a.topic_distances(metric, other=b)
    ba = b.topic_distances(metric, other=a)
    assert ab.shape == (100, 512) and ba.shape == (512, 100)
    _close(ab, _restate(a, b, metric), metric, "a x b")
    _close(ba, _restate(b, a, metric), metric, "b x a")            # KL: its own restatement
    _bounds(ab, metric)
    if metric in SYMMETRIC:
        assert float(np.max(np.abs(ab - ba.T))) <= 2e-9
    else:
        assert float(np.max(np.abs(ab - ba.T))) > 1e-3              # asymmetric
    assert a.topic_distances(metric, other=b).tobytes() == ab.tobytes()
    # nothing of the other sampler is written
    assert before == (b.counts()[0].tobytes(), b.counts()[1].tobytes(), b.z().tobytes())


def test_cross_mode_error_paths(pair):
    a, b = pair
    L = capi.load()
    out = np.zeros(512 * 512, np.float64)
    ids = np.zeros(512 * 64, np.int32)
    po, pi = out.ctypes.data, ids.ctypes.data

    def failed(status, code, text):
        return status == code and text in L.lda_last_error()

    with _sampler(20, 7, 3) as small:
        # V differs: the Python face refuses, and so does the library, with a message
        with pytest.raises(ValueError, match="word types"):
            a.topic_distances("cosine", other=small)
        assert failed(L.lda_topic_distances(a._h, small._h, 0, po), -1, b"num_types")
        assert failed(L.lda_topic_nearest(a._h, small._h, 0, 3, pi, po), -1, b"num_types")
    # the other checks, in the header's order
    assert failed(L.lda_topic_distances(a._h, b._h, 4, po), -1, b"metric")
    assert failed(L.lda_topic_distances(a._h, b._h, -1, None), -1, b"metric")
    for n in (0, -1, capi.TOPIC_NEAREST_MAX + 1):
        assert failed(L.lda_topic_nearest(a._h, b._h, 2, n, None, po), -1, b"LDA_TOPIC_NEAREST_MAX")
    assert failed(L.lda_topic_distances(a._h, b._h, 2, None), -1, b"null output")
    assert failed(L.lda_topic_nearest(a._h, None, 2, 3, pi, None), -1, b"null output")
    assert failed(L.lda_topic_nearest(a._h, None, 2, 3, None, po), -1, b"null output")
    # a pending delta on either side
    ok = a.topic_distances("hellinger", other=b)
    for pending, calls in ((a, (lambda: a.topic_distances(), lambda: a.topic_distances(other=b),
                                lambda: b.nearest_topics(3, other=a))),
                           (b, (lambda: a.topic_distances(other=b), lambda: a.nearest_topics(3, other=b),
                                lambda: b.topic_distances("cosine")))):
        pending.sample()
        for call in calls:
            with pytest.raises(capi.LdaError, match="lda_apply") as e:
                call()
            assert e.value.status == -4
        pending.apply()
    assert a.topic_distances("hellinger", other=b).shape == ok.shape


# -------------------------------------------------------------- nearest topics
def _check_nearest(g, other, metric, n, matrix):
    topics, values = g.nearest_topics(n, metric, other=other)
    et, ev = TD.expected_nearest(matrix, n, metric, other is None)
    assert topics.dtype == np.int32 and values.dtype == np.float64 and topics.shape == (g.K, n)
    np.testing.assert_array_equal(topics, et)
    assert values.tobytes() == ev.tobytes()                          # the matrix's own bits, NaN tails included
    return topics, values


@pytest.mark.parametrize("metric", METRICS)
def test_nearest_topics_against_the_devices_own_matrix(pair, metric):
    """The matrix is checked against numpy above; this isolates the selection:
    ids equal and values bitwise those of expected_nearest on topic_distances'
    own result."""
    a, b = pair
    self_matrix = a.topic_distances(metric)
    cross_matrix = a.topic_distances(metric, other=b)
    for n in (1, 5, 64):
        t, v = _check_nearest(a, None, metric, n, self_matrix)
        assert not np.any(t == np.arange(a.K)[:, None])              # no row lists itself
        assert np.all(t >= 0)                                        # 99 candidates
        t, v = _check_nearest(a, b, metric, n, cross_matrix)
        assert np.all(t >= 0) and np.all(np.isfinite(v))             # K2 = 512: full at n = 64
        step = np.diff(v, axis=1)
        assert np.all(step <= 0) if metric == "cosine" else np.all(step >= 0)
    # equal values (b's empty topics are one column) are listed by ascending id
    t, v = a.nearest_topics(64, metric, other=b)
    assert not np.any((np.diff(v, axis=1) == 0) & (np.diff(t, axis=1) <= 0))


@pytest.mark.parametrize("metric", METRICS)
def test_nearest_topics_on_the_constructed_state(constructed, metric):
    g = constructed
    d = g.topic_distances(metric)
    for n in (1, 5, 64):
        t, v = _check_nearest(g, None, metric, n, d)
        assert not np.any(t == np.arange(g.K)[:, None])
    t, v = g.nearest_topics(5, metric)
    same = 1.0 if metric == "cosine" else 0.0
    # ties at the best possible value: the lower id first
    assert t[3, :2].tolist() == [70, 99] and t[70, :2].tolist() == [3, 99] and t[99, :2].tolist() == [3, 70]
    assert np.all(v[list(TWINS), :2] == same)


@pytest.mark.parametrize("metric", ["cosine", "jensen_shannon"])
def test_nearest_topics_with_fewer_candidates_than_n(metric):
    K = 20
    with _sampler(K, 300, 9) as g:
        d = g.topic_distances(metric)
        t, v = _check_nearest(g, None, metric, 64, d)
        assert np.all(t[:, :K - 1] >= 0) and np.all(t[:, K - 1:] == -1)
        assert np.all(np.isfinite(v[:, :K - 1])) and np.all(np.isnan(v[:, K - 1:]))
        for row in range(K):
            assert sorted(t[row, :K - 1].tolist()) == [k for k in range(K) if k != row]
        step = np.diff(v[:, :K - 1], axis=1)
        assert np.all(step <= 0) if metric == "cosine" else np.all(step >= 0)
        # other = the sampler itself is self mode too
        t2, v2 = g.nearest_topics(64, metric, other=g)
        assert t2.tobytes() == t.tobytes() and v2.tobytes() == v.tobytes()


# ------------------------------------------------------------------ model face
def _model(corpus, K, devices=None, beta=0.01, iters=4):
    from ldagibbssampling_amd import topic_model as tm
    il = tm.InstanceList.fromCorpus(corpus)
    m = tm.ParallelTopicModel(K, 0.5 * K, beta)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(iters)
    m.setOptimizeInterval(0)
    if devices is not None:
        m.setDevices(devices)
    m.addInstances(il)
    m.estimate()
    return m


def test_model_face_on_one_and_three_shards():
    from ldagibbssampling_amd import topic_model as tm
    c = _corpus(_lengths(4), 300, 8)
    m1 = _model(c, 100)
    m3 = _model(c, 100, devices=[0, 0, 0])
    mb = _model(_corpus(_lengths(6), 300, 9), 20, beta=0.05)
    try:
        assert m1.numShards() == 1 and m3.numShards() == 3
        nw, nwsum = m1.typeTopicCounts()
        np.testing.assert_array_equal(m3.typeTopicCounts()[0], nw)
        for metric in METRICS:
            d1, d3 = m1.topicDistances(metric=metric), m3.topicDistances(metric=metric)
            assert d1.shape == (100, 100) and d1.tobytes() == d3.tobytes()     # the counts are replicated
            _close(d1, TD.topic_distances(nw, nwsum, 0.01, metric=metric, squared_hellinger=True), metric, "model")
            cross = m1.topicDistances(other=mb, metric=metric)
            assert cross.shape == (100, 20)
            assert m3.topicDistances(other=mb, metric=metric).tobytes() == cross.tobytes()
            nwb, nwsumb = mb.typeTopicCounts()
            _close(cross, TD.topic_distances(nw, nwsum, 0.01, nwb, nwsumb, 0.05, metric=metric,
                                             squared_hellinger=True), metric, "model x model")
            t, v = m1.nearestTopics(5, other=mb, metric=metric)
            et, ev = TD.expected_nearest(cross, 5, metric, False)
            np.testing.assert_array_equal(t, et)
            assert v.tobytes() == ev.tobytes()
            t, v = m3.nearestTopics(5, metric=metric)
            et, ev = TD.expected_nearest(d1, 5, metric, True)
            np.testing.assert_array_equal(t, et)
            assert v.tobytes() == ev.tobytes()
        # another alphabet over as many words: refused before any native call
        il = tm.InstanceList.fromCorpus(c, tm.Alphabet(f"w{i}" for i in range(300)))
        mo = tm.ParallelTopicModel(20, 10.0, 0.01)
        mo.addInstances(il)
        try:
            with pytest.raises(ValueError, match="alphabets differ"):
                m1.topicDistances(other=mo)
            with pytest.raises(ValueError, match="alphabets differ"):
                m1.nearestTopics(3, other=mo)
        finally:
            mo.close()
    finally:
        for m in (m1, m3, mb):
            m.close()
