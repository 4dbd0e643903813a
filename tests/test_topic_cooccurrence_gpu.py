"""GPU checks of the topic co-occurrence readout: lda_topic_cooccurrence
(k_topic_cooc + k_topic_cooc_mirror), its ldatm_ mirror, the measures, the
partners and the text.

Every expectation is the numpy restatement (topic_cooccurrence_numpy) on the z
that the test planted with set_z, so nothing needs training.  All six outputs
are integers and are compared byte for byte; no tolerance appears anywhere.

Geometry.  One wave takes a document; a block is four waves and the grid is
capped at 8 blocks per CU, P = 32 x CUs documents a trip: the second-trip test
holds 2 P + 37 documents.  Up to K = capi.TOPIC_COOC_LDS_TOPICS a block keeps
the packed triangles in LDS and flushes them once; above, every pair is a
global atomic: the shape test takes K on both sides of the constant, and the
hook lda_debug_topic_cooccurrence_global runs the global path at a small K,
where both must give the same bytes.  A document's distinct topics go into a
per-wave list that is walked 64 pairs at a time: documents with 1, 2, 20, 100,
299 and 2500 distinct topics cover a list shorter than, equal to and (far)
longer than a wave, with an odd and an even number of entries."""
import contextlib
import itertools

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

import topic_cooccurrence_numpy as N

pytestmark = pytest.mark.gpu

V = 50
LDS_K = capi.TOPIC_COOC_LDS_TOPICS
HEAD = ("tokens", "present")


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


def _sampler_kind(K):
    return "sparse" if K > capi.MAX_TOPICS_DENSE else "dense"


@contextlib.contextmanager
def _planted_sampler(docs, K, seed=11):
    from ldagibbssampling_amd.sampler import GibbsSampler
    c, z = _planted(docs)
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=seed,
                      sampler=_sampler_kind(K)) as g:
        g.set_z(z)
        g.apply()
        yield g, c, z


@contextlib.contextmanager
def _global_atomics():
    L = capi.load()
    L.lda_debug_topic_cooccurrence_global(1)
    try:
        yield
    finally:
        L.lda_debug_topic_cooccurrence_global(0)


def _same(got, exp, K, stats=N.STATS):
    assert set(got) == {"docs_used", *HEAD, *stats}
    assert isinstance(got["docs_used"], int) and got["docs_used"] == exp["docs_used"]
    for name in HEAD + tuple(stats):
        a, e = got[name], exp[name]
        assert a.dtype == np.int64 and a.shape == ((K,) if name in HEAD else (K, K)), name
        assert a.tobytes() == e.tobytes(), (name, np.argwhere(a != e)[:5])


def _check(g, c, z, K, min_tokens=10, min_count=2, min_prop=0.05, stats=N.STATS):
    got = g.topic_cooccurrence(stats, min_tokens, min_count, min_prop)
    exp = N.expected_cooccurrence(z, c.doc_off, K, min_tokens, min_count, min_prop, stats)
    _same(got, exp, K, stats)
    return exp


# ------------------------------------------------------------------- shapes
@pytest.mark.parametrize("K", [4, 20, LDS_K, LDS_K + 1, 300, 2048, 4096])
def test_cooccurrence_against_numpy(K):
    docs = _shape_docs(K, seed=K)
    distinct = max(len(np.unique(d)) for d in docs)
    assert distinct == (min(K, 20) if K < 300 else 299 if K < 4096 else 2500)
    with _planted_sampler(docs, K) as (g, c, z):
        assert g.z().tobytes() == z.tobytes()
        exp = _check(g, c, z, K)                                       # jsLDA's thresholds
        assert 0 < exp["docs_used"] < len(docs) and exp["codocs"].any()
        assert np.array_equal(np.diag(exp["codocs"]), exp["present"])
        assert np.array_equal(np.diag(exp["overlap"]), exp["tokens"])
        all_in = _check(g, c, z, K, 1, 1, 0.0)                         # every nonzero topic is present
        assert np.array_equal(all_in["codocs"] > 0, all_in["overlap"] > 0)
        assert all_in["tokens"].sum() == len(z)


def test_cooccurrence_every_subset_of_tables():
    """A NULL table is neither allocated nor accumulated, and the others do
    not change; on both paths."""
    K = 20
    with _planted_sampler(_shape_docs(K, seed=3), K) as (g, c, z):
        full = N.expected_cooccurrence(z, c.doc_off, K)
        for r in range(4):
            for stats in itertools.combinations(N.STATS, r):
                for ctx in (contextlib.nullcontext(), _global_atomics()):
                    with ctx:
                        got = g.topic_cooccurrence(stats)
                    _same(got, {k: v for k, v in full.items() if k in ("docs_used", *HEAD, *stats)}, K, stats)
        got = g.topic_cooccurrence("overlap")                          # a single name
        assert set(got) == {"docs_used", *HEAD, "overlap"}


@pytest.mark.parametrize("K", [4, LDS_K])
def test_cooccurrence_lds_and_global_paths_agree(K):
    with _planted_sampler(_shape_docs(K, seed=5 + K), K) as (g, c, z):
        for thr in ((10, 2, 0.05), (1, 1, 0.0)):
            exp = _check(g, c, z, K, *thr)
            with _global_atomics():
                _same(g.topic_cooccurrence(N.STATS, *thr), exp, K)


# --------------------------------------------------------------- thresholds
def test_cooccurrence_thresholds():
    K = 20
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
    longest = max(len(d) for d in docs)
    with _planted_sampler(docs, K) as (g, c, z):
        biggest = N.doc_topic_counts(z, c.doc_off, K).max()
        for min_prop in (0.0, 0.05, 0.25, 1.0):
            for min_count in (1, 2, int(biggest) + 1):
                for min_tokens in (1, 10, longest + 1):
                    exp = _check(g, c, z, K, min_tokens, min_count, min_prop)
                    if min_tokens > longest:
                        assert exp["docs_used"] == 0 and not any(exp[s].any() for s in HEAD + N.STATS)
                    elif min_count > biggest:
                        assert exp["docs_used"] > 0 and not exp["present"].any() and not exp["codocs"].any()
                        assert exp["overlap"].any() and exp["product"].any()
        # the planted documents alone: the shares sit where the comments say
        end = int(c.doc_off[6])
        a = N.expected_cooccurrence(z[:end], c.doc_off[:7], K, 1, 2, 0.05)
        b = N.expected_cooccurrence(z[:end], c.doc_off[:7], K, 1, 2, 0.25)
        assert (a["codocs"][1, 2], a["codocs"][3, 4], b["codocs"][1, 2], b["codocs"][3, 4]) == (2, 3, 0, 2)


# -------------------------------------------------------------- 64-bit cells
def test_cooccurrence_cells_above_2_to_the_32():
    K = 4
    big = np.concatenate([np.full(70000, 1), np.full(70000, 3)])
    rng = np.random.default_rng(2)
    rng.shuffle(big)
    docs = [np.array([0, 0, 1]), big, np.array([2] * 12 + [3] * 5)]
    with _planted_sampler(docs, K) as (g, c, z):
        exp = _check(g, c, z, K, 1, 1, 0.0)
        assert exp["product"][1, 3] == 4_900_000_000 > 2 ** 32 and exp["product"][3, 1] == 4_900_000_000
        assert exp["product"][1, 1] == 4_900_000_000 + 1 and exp["overlap"][1, 3] == 70000
        with _global_atomics():
            _same(g.topic_cooccurrence(N.STATS, 1, 1, 0.0), exp, K)


# ---------------------------------------------------------------- second trip
def test_grid_cap_topic_cooc_second_trip():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P = 32 * cus                                    # 8 blocks per CU, four one-document waves each
    K, D = 4, 64 * cus + 37
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
    with _planted_sampler(docs, K) as (g, c, z):
        assert g.D == D
        exp = _check(g, c, z, K, 1, 1, 0.0)
        assert exp["docs_used"] == D - 5
        _check(g, c, z, K)
        # the third trip's documents alone change the result
        short = N.expected_cooccurrence(z[:c.doc_off[2 * P]], c.doc_off[:2 * P + 1], K, 1, 1, 0.0)
        assert short["docs_used"] < exp["docs_used"] and short["product"].tobytes() != exp["product"].tobytes()
        with _global_atomics():
            _same(g.topic_cooccurrence(N.STATS, 1, 1, 0.0), exp, K)


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


def test_model_cooccurrence_on_two_and_three_shards(tmp_path):
    from ldagibbssampling_amd import topic_model as tm
    K = 20
    c, _ = _planted(_ragged_docs(K, 300, seed=4, max_len=60))
    for devices in ([0, 0], [0, 0, 0]):
        m = _model(c, K, devices)
        assert m.numShards() == len(devices)
        z = m.topicAssignments()
        for thr in ((10, 2, 0.05), (1, 1, 0.0), (5, 3, 0.25)):
            exp = N.expected_cooccurrence(z, c.doc_off, K, *thr)       # the whole corpus
            _same(m.topicCooccurrence(N.STATS, *thr), exp, K)
            _same(m.topicCooccurrence(("product",), *thr), {k: v for k, v in exp.items()
                                                          if k not in ("codocs", "overlap")}, K, ("product",))
            for measure in tm.CORR_MEASURES:
                mat = m.topicCorrelations(measure, *thr)
                want = tm.topic_correlation_finish(measure, exp["docs_used"], exp["tokens"], exp["present"],
                                                   exp[tm.MEASURE_TABLE[measure]])
                assert mat.tobytes() == want.tobytes(), measure
                assert N.same_floats(mat, N.finish(measure, exp["docs_used"], exp["tokens"], exp["present"],
                                                   exp[tm.MEASURE_TABLE[measure]])), measure
                for n in (3, K + 5):
                    ids, values = m.topicPartners(n, measure, *thr)
                    wi, wv = N.partners(want, n)
                    assert ids.dtype == np.int32 and np.array_equal(ids, wi) and N.same_floats(values, wv)
                    assert m.getTopicPartners(n, measure, *thr) == \
                        [[(int(t), float(v)) for t, v in zip(wi[k], wv[k]) if t >= 0] for k in range(K)]
                    text = tm.format_topic_correlations(wi, wv)
                    assert m.topicCorrelationsText(n, measure, *thr) == text
                path = tmp_path / "topic_correlations.txt"
                m.printTopicCorrelations(path, 3, measure, *thr)
                assert path.read_text() == tm.format_topic_correlations(*N.partners(want, 3))
                cutoff = float(np.nanmedian(want[np.isfinite(want)]))
                edges = m.topicGraph(measure, cutoff, *thr)
                assert edges == [(k, l, float(want[k, l])) for k in range(K) for l in range(k + 1, K)
                                 if want[k, l] >= cutoff]
        assert text.startswith("#topic partner value\n0 ")
        m.close()


# --------------------------------------------------------- state and errors
def test_cooccurrence_state_and_errors():
    import ctypes as C
    import math
    K = 20
    docs = _ragged_docs(K, 12, seed=1, max_len=40)
    from ldagibbssampling_amd.sampler import GibbsSampler
    c, z = _planted(docs)
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=3) as g:
        # lda_create leaves the shard's counts as the pending delta
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
            g.topic_cooccurrence()
        assert e.value.status == -4
        g.sweep(1)
        out = np.zeros(K * K, np.int64)
        used = C.c_int64(7)
        u, p = C.byref(used), out.ctypes.data
        call, err = g._L.lda_topic_cooccurrence, g._L.lda_last_error
        for args in ((None, p, p), (u, None, p), (u, p, None)):
            assert call(g._h, 10, 2, 0.05, *args, p, p, p) == -1 and b"null output" in err()
        for mt in (0, -2):
            assert call(g._h, mt, 2, 0.05, u, p, p, p, p, p) == -1 and b"min_tokens" in err()
        for mc in (0, -2):
            assert call(g._h, 10, mc, 0.05, u, p, p, p, p, p) == -1 and b"min_count" in err()
        for mp in (-1e-9, 1.0 + 1e-9, math.nan, math.inf, -math.inf):
            assert call(g._h, 10, 2, mp, u, p, p, p, p, p) == -1 and b"min_prop" in err()
        assert not out.any() and used.value == 7                       # nothing was written
        g.sample()                                                     # a pending delta again
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.topic_cooccurrence()
        g.apply()
        _check(g, c, g.z(), K)


@pytest.mark.parametrize("D", [0, 3])
def test_cooccurrence_without_documents_or_tokens(D):
    K = 20
    with _planted_sampler([np.zeros(0, np.int32)] * D, K) as (g, _, _):
        got = g.topic_cooccurrence(min_tokens=1)
        assert got["docs_used"] == 0 and not any(got[s].any() for s in HEAD + N.STATS)
        assert got["codocs"].shape == (K, K)


def test_cooccurrence_changes_no_state():
    K = 100
    from ldagibbssampling_amd.sampler import GibbsSampler
    c, _ = _planted(_ragged_docs(K, 300, seed=6, max_len=60))
    mk = lambda: GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=21)
    with mk() as g, mk() as ref:
        g.sweep(2)
        ref.sweep(2)
        z, before, sweeps = g.z(), g.counts_checksum(), g.sweep_index
        assert before == ref.counts_checksum() and sweeps == ref.sweep_index
        a = g.topic_cooccurrence()
        b = g.topic_cooccurrence()
        _same(a, N.expected_cooccurrence(z, c.doc_off, K), K)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
        assert g.z().tobytes() == z.tobytes() and g.counts_checksum() == before and g.sweep_index == sweeps
        g.sweep(1)
        ref.sweep(1)
        assert g.z().tobytes() == ref.z().tobytes() and g.counts_checksum() == ref.counts_checksum()
        assert g.sweep_index == ref.sweep_index
