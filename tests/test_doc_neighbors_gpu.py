"""GPU checks of lda_doc_distances, lda_doc_nearest and lda_doc_neighbors
(k_doc_rows, k_doc_row_sums, k_doc_pairs, k_doc_select), their ldatm_ mirrors
and the Python faces, against the numpy restatement in doc_neighbors_numpy.py
computed from doc_counts() and alpha.

Tolerance: absolute 1e-9 on cosine, Jensen-Shannon and the SQUARE of Hellinger
(the root magnifies rounding without bound near 0).  Not a measured number: a
sequential fp64 sum of K <= 4096 terms with sum|terms| below about 30 is off by
about K 2^-53 30 = 1.4e-11, and the logarithm's last bits add the same order.
Cosine must also agree with score_docs("cosine") at rtol 1e-12, the project's
fp64 bar: two summation forms of one quantity.

The selection is compared with np.lexsort on the device's own doc_distances
matrix: ids exact, values bitwise, every case.

Shapes: tiles are 64 x 64 (query, candidate) pairs and K is walked 32 topics at
a time, so D = 1, 2 are one partial tile, 65 crosses into a second, 300 and
1100 are several with a ragged last one; K = 4, 20 are one partial step, 100
ends in one, 512 and 2048 are whole steps.  The chunk hook (64, 64) and (100,
3) makes the second trip of both chunk loops and the running-list merge run at
these sizes.  Document lengths 0, 1, 63, 64, 65 and K + 10 are present wherever
D allows.
"""
import math

import numpy as np
import pytest

import doc_neighbors_numpy as DN
from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu

TOL = 1e-9
METRICS = ("cosine", "hellinger", "jensen_shannon")
LN2 = math.log(2.0)
V = 50
# (K, D, asymmetric alpha)
CASES = [(4, 1, False), (4, 2, False), (20, 65, True), (100, 300, True), (512, 300, False), (20, 1100, False),
         (512, 1100, False), (2048, 65, False)]


# ------------------------------------------------------------------ helpers
def _lengths(K, D, seed):
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 63, 64, 65, K + 10]
    if D == 1:
        return np.array([5], np.int64)
    if D == 2:
        return np.array([0, 7], np.int64)
    lens = np.array(fixed + rng.integers(2, 40, D - len(fixed)).tolist(), np.int64)
    rng.shuffle(lens)
    return lens


def _corpus(lengths, seed):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    return Corpus(off, rng.integers(0, V, int(off[-1])).astype(np.int32), V)


def _alpha(K, asymmetric):
    return np.linspace(0.05, 0.9, K) if asymmetric else np.full(K, 0.3)


class _State:
    """A sampler after 2 sweeps and what the tests share about it."""

    def __init__(self, K, D, asymmetric):
        from ldagibbssampling_amd.sampler import GibbsSampler
        self.K, self.D = K, D
        c = _corpus(_lengths(K, D, K + D), 3 * K + D)
        self.g = GibbsSampler(K, V, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=K * 7 + D,
                              sampler="sparse" if K > capi.MAX_TOPICS_DENSE else "dense")
        self.g.sweep(2)
        self.alpha = _alpha(K, asymmetric)
        if asymmetric:
            self.g.set_alpha_beta(self.alpha, 0.05)
        self.lens = np.diff(c.doc_off)
        self.z0 = self.g.z()
        self.nw0 = self.g.counts()[0]
        self.nd = self.g.doc_counts()
        assert self.nd.sum(axis=1).tolist() == self.lens.tolist()
        self.rows = DN.rows_from_counts(self.nd, self.alpha)
        rng = np.random.default_rng(K + 31 * D)
        # count queries: own documents (the first, the last, one per tile edge), then foreign rows; 70 of them
        # cross the 64-wide query tile
        own = np.unique(np.clip([0, 1, 63, 64, D // 2, D - 1], 0, D - 1))
        self.qcounts = np.concatenate([self.nd[own], rng.integers(0, 6, (70 - len(own), K)).astype(np.int32)])
        self.qcounts[len(own)] = 0                                   # an all-zero count row: the prior alone
        th = rng.dirichlet(np.full(K, 0.2), 5)
        th[0, : K // 2] = 0.0                                        # zeros: x ln x = 0
        th[0] /= th[0].sum()
        th[1] *= 3.0                                                 # not normalised: used as given
        self.theta = th
        self._dist = {}

    def distances(self, metric, form):
        """The device's full matrix of the shared queries, computed once."""
        key = (metric, form)
        if key not in self._dist:
            kw = {"counts": self.qcounts} if form == "counts" else {"theta": self.theta}
            self._dist[key] = self.g.doc_distances(metric, **kw)
        return self._dist[key]

    def unchanged(self):
        assert np.array_equal(self.g.z(), self.z0) and np.array_equal(self.g.counts()[0], self.nw0)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "K%d-D%d%s" % (c[0], c[1], "-asym" if c[2] else ""))
def state(request):
    s = _State(*request.param)
    try:
        yield s
    finally:
        s.g.close()


def _close(got, want, metric, what):
    g = got * got if metric == "hellinger" else got
    err = float(np.max(np.abs(g - want))) if g.size else 0.0
    print(f"{what} {metric}: max abs error {err:.3e}")
    assert err <= TOL, (what, metric, err)


def _bounds(d, metric):
    assert np.isfinite(d).all() and not np.signbit(d).any(), metric
    if metric == "cosine":
        assert d.min() > 0.0 and d.max() <= 1.0
    elif metric == "hellinger":
        assert d.min() >= 0.0 and d.max() <= 1.0
    else:
        assert d.min() >= 0.0 and d.max() <= LN2


def _same(got, want, what=""):
    gi, gv = got
    wi, wv = want
    assert gi.dtype == np.int64 and gv.dtype == np.float64
    assert np.array_equal(gi, wi), what
    assert gv.tobytes() == np.ascontiguousarray(wv).tobytes(), what


# ------------------------------------------------------------- distances
def test_distances_against_numpy(state):
    s, g = state, state.g
    for metric in METRICS:
        dc = s.distances(metric, "counts")
        assert dc.shape == (70, s.D)
        _close(dc, DN.distances(DN.rows_from_counts(s.qcounts, s.alpha), s.rows, metric, squared_hellinger=True),
               metric, "counts")
        _bounds(dc, metric)
        dt = s.distances(metric, "theta")
        _close(dt, DN.distances(s.theta, s.rows, metric, squared_hellinger=True), metric, "theta")
        assert np.isfinite(dt).all() and not np.signbit(dt).any()
        # a repeat returns the same bytes; a range and a shuffled list with duplicates the same columns
        assert g.doc_distances(metric, counts=s.qcounts).tobytes() == dc.tobytes()
        rng = np.random.default_rng(5)
        docs = np.concatenate([rng.permutation(s.D), rng.integers(0, s.D, 3)])
        assert g.doc_distances(metric, counts=s.qcounts[:3], docs=docs).tobytes() == \
            np.ascontiguousarray(dc[:3][:, docs]).tobytes()
        b, m = s.D // 3, max(1, s.D // 2)
        assert g.doc_distances(metric, theta=s.theta, doc_begin=b, num_docs=min(m, s.D - b)).tobytes() == \
            np.ascontiguousarray(dt[:, b:b + m]).tobytes()
    np.testing.assert_allclose(s.distances("cosine", "theta"), g.score_docs(s.theta, "cosine"), rtol=1e-12, atol=0)
    s.unchanged()


def test_own_counts_are_the_candidates_own_rows(state):
    """A query with a document's counts is that document's row bit for bit:
    exactly 0 (Hellinger, Jensen-Shannon) and exactly 1 (cosine) to it."""
    s = state
    own = np.unique(np.clip([0, 1, 63, 64, s.D // 2, s.D - 1], 0, s.D - 1))
    for metric in METRICS:
        d = s.distances(metric, "counts")
        want = 1.0 if metric == "cosine" else 0.0
        for i, doc in enumerate(own):
            assert d[i, doc] == want and not np.signbit(d[i, doc]), (metric, doc)


# --------------------------------------------------------------- selection
@pytest.mark.parametrize("n", [1, 5, 64])
def test_nearest_is_lexsort_of_the_devices_own_matrix(state, n):
    s, g = state, state.g
    rng = np.random.default_rng(n)
    skip = rng.integers(-1, s.D, 70)
    skip[0] = 0                                                     # query 0 holds document 0's counts
    for metric in METRICS:
        d = s.distances(metric, "counts")
        # min_tokens = 1, the default, keeps the empty documents out
        _same(g.nearest_docs(n, metric, counts=s.qcounts), DN.nearest(d, n, metric, lengths=s.lens), "plain")
        _same(g.nearest_docs(n, metric, counts=s.qcounts, min_tokens=3),
              DN.nearest(d, n, metric, lengths=s.lens, min_tokens=3), "min_tokens")
        got = g.nearest_docs(n, metric, counts=s.qcounts, skip=skip, min_tokens=2)
        _same(got, DN.nearest(d, n, metric, lengths=s.lens, min_tokens=2, skip=skip), "skip")
        assert not ((got[0] == skip[:, None]) & (skip[:, None] >= 0)).any()
        candidates = int((s.lens >= 2).sum())
        if n > candidates:                                          # the tail holds -1 / NaN
            assert (got[0][:, candidates:] == -1).all() and np.isnan(got[1][:, candidates:]).all()
        dt = s.distances(metric, "theta")
        _same(g.nearest_docs(n, metric, theta=s.theta), DN.nearest(dt, n, metric, lengths=s.lens), "theta")
    s.unchanged()


@pytest.mark.parametrize("n", [3, 64])
def test_neighbors_equal_counts_then_nearest(state, n):
    s, g = state, state.g
    rng = np.random.default_rng(7)
    shuffled = np.concatenate([rng.permutation(s.D), rng.integers(0, s.D, 4)])
    for metric in METRICS:
        for docs in (None, shuffled):
            ids = np.arange(s.D) if docs is None else docs
            got = g.doc_neighbors(n, metric, docs=docs, min_tokens=2)
            want = g.nearest_docs(n, metric, counts=g.doc_counts(docs=ids), skip=ids, min_tokens=2)
            _same(got, want, metric)
            assert not (got[0] == ids[:, None]).any()               # no document is its own neighbour
            _same(g.doc_neighbors(n, metric, docs=docs, min_tokens=2), got, "repeat")
    s.unchanged()


def test_chunks_do_not_change_a_bit(state):
    """The second trip of the candidate and the query chunk loops and the
    merge of the running lists: every result as with the default chunks."""
    s, g = state, state.g
    n = 5
    rng = np.random.default_rng(11)
    docs = np.concatenate([rng.permutation(s.D), rng.integers(0, s.D, 4)])

    def results():
        out = []
        for metric in METRICS:
            out.append(g.doc_distances(metric, counts=s.qcounts).tobytes())
            out.append(g.doc_distances(metric, theta=s.theta, docs=docs).tobytes())
            for r in (g.nearest_docs(n, metric, counts=s.qcounts, min_tokens=2, skip=np.arange(70) % s.D),
                      g.nearest_docs(64, metric, theta=s.theta), g.doc_neighbors(n, metric, min_tokens=2),
                      g.doc_neighbors(64, metric, docs=docs)):
                out += [r[0].tobytes(), r[1].tobytes()]
        return out

    L = capi.load()
    want = results()
    try:
        # the uneven cut: 3 queries a chunk; 48 at D = 1100, where 3 would mean thousands of launches
        for chunk in ((64, 64), (100, 3 if s.D <= 300 else 48)):
            L.lda_debug_doc_nearest_chunk(*chunk)
            assert results() == want, chunk
    finally:
        L.lda_debug_doc_nearest_chunk(0, 0)
    s.unchanged()


# ------------------------------------------------------- constructed state
def test_identical_documents_in_different_tiles():
    """Documents 2, 5 and 68 hold the same counts (5 and 68 by other words and
    another token order; 68 sits in the second 64-wide tile), document 7 is
    empty.  The three are at exactly 0 / 1 from each other, have bit-equal
    values to every fourth document and come first in each other's lists in id
    order."""
    from ldagibbssampling_amd.sampler import GibbsSampler
    K, D = 20, 70
    rng = np.random.default_rng(3)
    lens = rng.integers(5, 30, D)
    lens[[2, 5, 68]] = 12
    lens[7] = 0
    c = _corpus(lens, 17)
    z = rng.integers(0, K, c.num_tokens).astype(np.int32)
    topics = np.array([3, 3, 3, 3, 9, 9, 9, 0, 0, 19, 19, 4], np.int32)
    off = c.doc_off
    z[off[2]:off[3]] = topics
    z[off[5]:off[6]] = topics[::-1]
    z[off[68]:off[69]] = rng.permutation(topics)
    alpha = np.linspace(0.1, 0.7, K)
    twins = [2, 5, 68]
    with GibbsSampler(K, V, c.doc_off, c.words, alpha, 0.05, seed=1) as g:
        g.set_z(z)
        g.apply()
        nd = g.doc_counts()
        assert np.array_equal(nd[2], nd[5]) and np.array_equal(nd[2], nd[68]) and nd[7].sum() == 0
        for metric in METRICS:
            same = 1.0 if metric == "cosine" else 0.0
            d = g.doc_distances(metric, counts=nd)                   # D x D, every document against every document
            _close(d, DN.distances(DN.rows_from_counts(nd, alpha), DN.rows_from_counts(nd, alpha), metric,
                                   squared_hellinger=True), metric, "constructed")
            for a in twins:
                for b in twins:
                    assert d[a, b] == same and not np.signbit(d[a, b]), (metric, a, b)
                assert d[a].tobytes() == d[2].tobytes() and d[:, a].tobytes() == d[:, 2].tobytes(), (metric, a)
            assert (np.diag(d) == same).all()
            ids, vals = g.doc_neighbors(4, metric)
            for a in twins:
                others = [t for t in twins if t != a]
                assert ids[a, :2].tolist() == others and (vals[a, :2] == same).all(), (metric, a)
            # the later ranks are the same documents at the same bits for the three
            assert np.array_equal(ids[2, 2:], ids[5, 2:]) and np.array_equal(ids[2, 2:], ids[68, 2:])
            assert vals[2, 2:].tobytes() == vals[5, 2:].tobytes() == vals[68, 2:].tobytes()
            # the empty document is the prior alone; min_tokens = 1 keeps it out of every list
            assert not (ids == 7).any()
            prior = g.doc_distances(metric, theta=alpha / alpha.sum(), docs=[7])
            assert abs(prior[0, 0] - same) <= 1e-12
        assert np.array_equal(g.z(), z)


# ------------------------------------------------------- errors and state
def test_argument_checks_name_their_argument_and_a_pending_delta_is_a_state_error():
    from ldagibbssampling_amd.sampler import GibbsSampler
    K, D = 4, 6
    c = _corpus(np.array([3, 0, 5, 2, 9, 1]), 2)
    with GibbsSampler(K, V, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=3) as g:
        theta = np.full((2, K), 0.25)
        counts = np.ones((2, K), np.int32)
        calls = (lambda: g.doc_distances("cosine", theta=theta), lambda: g.nearest_docs(2, counts=counts),
                 lambda: g.doc_neighbors(2))
        for call in calls:                                           # lda_create leaves a pending delta
            with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
                call()
            assert e.value.status == -4
        g.sweep(1)
        L, h = g._L, g._h
        out = np.zeros(64, np.float64)
        ids = np.zeros(64, np.int64)
        po, pi, pt, pc = out.ctypes.data, ids.ctypes.data, theta.ctypes.data, counts.ctypes.data

        def failed(status, word):
            return status == -1 and word in L.lda_last_error()

        for metric in (-1, 3):
            assert failed(L.lda_doc_distances(h, metric, 2, pt, None, 0, D, None, po), b"metric")
            assert failed(L.lda_doc_nearest(h, metric, 2, 2, pt, None, None, 1, pi, po), b"metric")
            assert failed(L.lda_doc_neighbors(h, metric, 2, 0, D, None, 1, pi, po), b"metric")
        for n in (0, capi.DOC_NEAREST_MAX + 1):
            assert failed(L.lda_doc_nearest(h, 1, n, 2, pt, None, None, 1, pi, po), b"LDA_DOC_NEAREST_MAX")
            assert failed(L.lda_doc_neighbors(h, 1, n, 0, D, None, 1, pi, po), b"LDA_DOC_NEAREST_MAX")
        for a, b in ((pt, pc), (None, None)):
            assert failed(L.lda_doc_distances(h, 1, 2, a, b, 0, D, None, po), b"theta / counts")
            assert failed(L.lda_doc_nearest(h, 1, 2, 2, a, b, None, 1, pi, po), b"theta / counts")
        assert failed(L.lda_doc_distances(h, 1, 2, pt, None, 0, D, None, None), b"null output")
        assert failed(L.lda_doc_nearest(h, 1, 2, 2, pt, None, None, 1, None, po), b"null output")
        assert failed(L.lda_doc_neighbors(h, 1, 2, 0, D, None, 1, pi, None), b"null output")
        assert failed(L.lda_doc_distances(h, 1, -1, pt, None, 0, D, None, po), b"bad sizes")
        assert failed(L.lda_doc_neighbors(h, 1, 2, 0, -1, None, 1, pi, po), b"bad sizes")
        bad_doc = np.array([0, D], np.int64)
        assert failed(L.lda_doc_distances(h, 1, 2, pt, None, 0, 2, bad_doc.ctypes.data, po), b"document id")
        assert failed(L.lda_doc_distances(h, 1, 2, pt, None, 1, D, None, po), b"document range")
        assert failed(L.lda_doc_neighbors(h, 1, 2, 0, 2, bad_doc.ctypes.data, 1, pi, po), b"document id")
        assert failed(L.lda_doc_neighbors(h, 1, 2, D, 1, None, 1, pi, po), b"document range")
        assert failed(L.lda_doc_nearest(h, 1, 2, 2, pt, None, None, 0, pi, po), b"min_tokens")
        assert failed(L.lda_doc_neighbors(h, 1, 2, 0, D, None, 0, pi, po), b"min_tokens")
        for bad in (D, -2):
            skip = np.array([-1, bad], np.int64)
            assert failed(L.lda_doc_nearest(h, 1, 2, 2, pt, None, skip.ctypes.data, 1, pi, po), b"skip")
        t = theta.copy()
        t[1, 1] = -0.5
        assert failed(L.lda_doc_distances(h, 1, 2, t.ctypes.data, None, 0, D, None, po), b"theta holds")
        t[1] = 0.0
        assert failed(L.lda_doc_nearest(h, 1, 2, 2, t.ctypes.data, None, None, 1, pi, po), b"theta row sums to zero")
        cn = counts.copy()
        cn[0, 2] = -1
        assert failed(L.lda_doc_distances(h, 1, 2, None, cn.ctypes.data, 0, D, None, po), b"counts holds a negative")
        assert not out.any() and not ids.any()                       # nothing was written
        # nothing to do
        assert L.lda_doc_distances(h, 1, 0, pt, None, 0, D, None, None) == 0
        assert L.lda_doc_distances(h, 1, 2, pt, None, 0, 0, None, None) == 0
        assert L.lda_doc_nearest(h, 1, 2, 0, pt, None, None, 1, None, None) == 0
        assert L.lda_doc_neighbors(h, 1, 2, 0, 0, None, 1, None, None) == 0
        assert g.doc_distances("cosine", theta=theta).shape == (2, D)
        g.sample()                                                   # a pending delta again
        for call in calls:
            with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
                call()
        g.apply()
        assert g.doc_neighbors(2)[0].shape == (D, 2)


# -------------------------------------------------------------- model level
def _model(corpus, K, devices):
    from ldagibbssampling_amd import topic_model as tm
    m = tm.ParallelTopicModel(K, 0.5 * K, 0.01)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(4)
    m.setOptimizeInterval(0)
    m.setDevices(devices)
    m.addInstances(tm.InstanceList.fromCorpus(corpus))
    m.estimate()
    return m


def test_model_face_on_one_and_three_shards(tmp_path):
    from ldagibbssampling_amd import topic_model as tm
    K, D = 20, 300
    c = _corpus(_lengths(K, D, 4), 8)
    rng = np.random.default_rng(6)
    theta = rng.dirichlet(np.full(K, 0.3), 6)
    docs = np.concatenate([rng.permutation(D)[:150], rng.integers(0, D, 5)])
    skip = rng.integers(-1, D, 6)
    held = [tm.Instance(rng.integers(0, V, 15)) for _ in range(3)]
    seen = []
    for devices in ([0], [0, 0, 0]):
        m = _model(c, K, devices)
        try:
            assert m.numShards() == len(devices)
            nd = m.docCounts()
            rows = DN.rows_from_counts(nd, m.alpha)
            got = {}
            for metric in METRICS:
                d = m.documentDistances(theta=theta, metric=metric)
                _close(d, DN.distances(theta, rows, metric, squared_hellinger=True), metric, "model")
                dl = m.documentDistances(counts=nd[:4], docs=docs, metric=metric)
                assert dl.tobytes() == np.ascontiguousarray(m.documentDistances(counts=nd[:4], metric=metric)[:, docs]
                                                            ).tobytes()
                near = m.nearestDocuments(theta, 7, metric, minTokens=2)
                _same(near, DN.nearest(d, 7, metric, lengths=np.diff(c.doc_off), min_tokens=2), "model nearest")
                near_skip = m.nearestDocuments(theta, 64, metric, skip=skip)
                _same(near_skip, DN.nearest(d, 64, metric, lengths=np.diff(c.doc_off), skip=skip), "model skip")
                nb = m.documentNeighbors(5, metric=metric, minTokens=2)
                _same(nb, m.nearestDocuments(None, 5, metric, minTokens=2, counts=nd, skip=np.arange(D)), "neighbors")
                nbl = m.documentNeighbors(5, docs=docs, metric=metric, minTokens=2)
                _same(nbl, (nb[0][docs], nb[1][docs]), "neighbors of a list")
                one = m.getDocumentNeighbors(int(docs[0]), 5, metric, 2)
                assert one == [(int(i), f"example:{int(i)}", float(v)) for i, v in zip(nbl[0][0], nbl[1][0]) if i >= 0]
                text = tm.format_document_neighbors(*nb)
                assert m.documentNeighborsText(5, metric, 2) == text and text.startswith("#doc neighbor name value\n0 ")
                path = tmp_path / "neighbors.txt"
                m.printDocumentNeighbors(path, 5, metric, 2)
                assert path.read_text() == text
                inf = m.getInferencer()
                th = inf.getSampledDistributions(held, 20, 5, 5, seed=9)
                _same(inf.nearestInstances(held, 4, metric, 20, 5, 5, seed=9), m.nearestDocuments(th, 4, metric),
                      "nearestInstances")
                got[metric] = [x.tobytes() for x in (d, dl, *near, *near_skip, *nb, *nbl)]
            seen.append((m.topicAssignments().tobytes(), got))
        finally:
            m.close()
    assert seen[0][0] == seen[1][0]                                  # one corpus and seed: the same z
    assert seen[0][1] == seen[1][1]                                  # and the same bytes from every call
