"""GPU checks of the top documents per topic: lda_topic_top_docs
(k_topic_docs_count + k_topic_docs_slab + k_topic_docs_merge), its ldatm_
mirror and printTopicDocuments' text.

Every expectation is the numpy restatement (topic_docs_numpy) on z() of the
same context: nd from np.add.at, the weights from the header's expression,
np.lexsort((ids, -w)) cut at n.  Everything compared is an integer array and is
compared exactly; no tolerance appears anywhere.

Geometry.  The documents go through in chunks of 2^23 / Kp documents (the test
hook overrides it); a chunk is cut into slabs of at least 256 documents, at
most 1024 / (Kp / 64) of them, and slab s of every later chunk continues slab
s's list.  So D = 1 and 7 are one partial slab, D = 300 two slabs of 150 and
D = 3001 twelve slabs (eleven of 251 and one of 240) in one chunk at every K of
the shape test (K = 2048 cuts chunks of 4096 documents).  With the default
chunks the slab count 2^15 / Kp never reaches the cap 2^16 / Kp, so the cap
test (K = 4096: 64 topic groups, at most 16 slabs) sets one chunk of 8192
documents through the hook: its 5000 documents would be 20 slabs of 250 and
become 16 slabs of 313; the default there is three chunks of 2048, 2048 and
904 documents in 8 slabs of 256.  The count pass gives a wave a document and
caps its grid at 8 blocks per CU, P = 32 x CUs documents a trip: the
second-trip test holds 2 P + 37 documents in one chunk (Kp = 64: 131072).
"""
import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

import topic_docs_numpy as N

pytestmark = pytest.mark.gpu

V = 50
SETTINGS = [(s, mt) for s in (0.0, 10.0, 1e-3) for mt in (1, 5)]


# ------------------------------------------------------------------ helpers
def _corpus(lengths, seed, num_types=V):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    words = rng.integers(0, num_types, int(off[-1])).astype(np.int32)
    return Corpus(off, words, num_types)


def _lengths(seed, n):
    """test_readout_gpu's lengths: an empty document, a one-token one, one
    wave's 64 lanes, 65, several passes, among ordinary ones, shuffled (fewer
    than five documents: the first n of the ordinary ones)."""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 64, 65, 150] if n >= 5 else []
    lens = np.array(fixed + rng.integers(2, 40, n - len(fixed)).tolist(), np.int64)
    rng.shuffle(lens)
    return lens


def _sampler_kind(K):
    return "sparse" if K > capi.MAX_TOPICS_DENSE else "dense"


def _sampler(c, K, seed=11):
    from ldagibbssampling_amd.sampler import GibbsSampler
    return GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.3), 0.05, seed=seed,
                        sampler=_sampler_kind(K))


def _check(g, c, K, n, smoothing, min_tokens, z=None):
    got = g.topic_top_docs(n, smoothing, min_tokens)
    exp = N.expected_topic_docs(g.z() if z is None else z, c.doc_off, K, n, smoothing, min_tokens)
    for a, e in zip(got, exp):
        assert a.dtype == e.dtype and a.shape == (K, n)
        np.testing.assert_array_equal(a, e)
    return exp


# ------------------------------------------------------------------- shapes
@pytest.mark.parametrize("D", [1, 7, 300, 3001])
@pytest.mark.parametrize("K", [4, 20, 100, 500, 2048])
def test_topic_docs_against_numpy(K, D):
    assert (capi.padded_topics(K) != K) == (K in (4, 20, 100, 500))
    c = _corpus(_lengths(K + D, D), 5)
    with _sampler(c, K, seed=K * 7 + D) as g:
        g.apply()                               # lda_create leaves the counts pending: the random start
        for s, mt in SETTINGS:
            _check(g, c, K, 10, s, mt)
        g.sweep(3)
        z = g.z()
        for n in (1, 10, 64, 128):              # n > D at D = 1 and 7
            for s, mt in SETTINGS:
                exp = _check(g, c, K, n, s, mt, z)
                assert np.all(exp[1][exp[0] < 0] == 0) and np.all(exp[2][exp[0] < 0] == 0)
        if D < 10:
            assert np.any(exp[0] < 0)           # padded slots were compared
        again = g.topic_top_docs(128, 1e-3, 5)
        assert all(a.tobytes() == e.tobytes() for a, e in zip(again, exp))


# --------------------------------------------------------------------- ties
def test_topic_docs_long_runs_of_equal_weights():
    """200 one- and two-token documents and 50 identical ones: at smoothing 0
    every one-topic document weighs 1.0, whatever its length."""
    K = 4
    rng = np.random.default_rng(2)
    lens = np.concatenate([rng.integers(1, 3, 200), np.full(50, 6)]).astype(np.int64)
    c = _corpus(lens, 3)
    c.words[int(c.doc_off[200]):] = np.tile(np.arange(6, dtype=np.int32), 50)
    with _sampler(c, K) as g:
        g.sweep(3)
        z = g.z()
        for n in (10, 64, 128):
            for mt in (1, 2):
                docs, cnt, lens_ = _check(g, c, K, n, 0.0, mt, z)
                assert N.has_tie(K, 0.0, docs, cnt, lens_), "no equal adjacent weights in any topic's selection"
        # the identical documents under one assignment: 50 equal weights in every topic
        zz = z.copy()
        zz[int(c.doc_off[200]):] = np.tile(np.array([0, 0, 0, 1, 2, 3], np.int32), 50)
        g.set_z(zz)
        g.apply()
        docs, cnt, lens_ = _check(g, c, K, 64, 10.0, 3, zz)
        assert docs[0, :50].tolist() == list(range(200, 250)) and N.has_tie(K, 10.0, docs, cnt, lens_)


# ------------------------------------------------------------- every insert
def test_topic_docs_rising_weights_every_document_inserts():
    """Document d holds d + 1 tokens of topic 0 among L = 600: topic 0's
    weight rises with the id, so within a slab (three of 200) every document
    inserts at the head; topic 1 is the mirror image, nothing inserts after a
    slab's first n."""
    K, D = 20, 600
    c = _corpus(np.full(D, D, np.int64), 4)
    z = np.ones((D, D), np.int32)
    z[np.tril_indices(D)] = 0                  # row d: d + 1 zeros
    z = z.reshape(-1)
    with _sampler(c, K) as g:
        g.set_z(z)
        g.apply()
        for n in (1, 10, 128):
            docs, cnt, _ = _check(g, c, K, n, 0.0, 1, z)
            assert docs[0].tolist() == list(range(D - 1, D - 1 - n, -1)) and cnt[0, 0] == D
            assert docs[1].tolist() == list(range(n)) and cnt[1, 0] == D - 1
            assert np.all(docs[2:] == -1)
        _check(g, c, K, 64, 10.0, 1, z)


# ------------------------------------------------- slab cap and second trips
def test_topic_docs_slab_cap_at_k_4096():
    K, D = 4096, 5000
    rng = np.random.default_rng(6)
    c = _corpus(rng.integers(4, 13, D).astype(np.int64), 7)
    L = capi.load()
    with _sampler(c, K) as g:
        g.sweep(1)
        z = g.z()
        base = _check(g, c, K, 10, 0.0, 1, z)          # three chunks of 8 slabs
        try:
            L.lda_debug_topic_docs_chunk_docs(8192)    # one chunk: 16 slabs of 313 documents
            for n, s, mt in ((10, 0.0, 1), (128, 10.0, 5)):
                one = _check(g, c, K, n, s, mt, z)
        finally:
            L.lda_debug_topic_docs_chunk_docs(0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_check(g, c, K, 128, 10.0, 5, z), one))
        assert N.has_tie(K, 0.0, *base)


def test_grid_cap_topic_docs_count_second_trip():
    import torch
    P = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    K, D = 4, 2 * P + 37
    assert D <= (1 << 23) // capi.padded_topics(K)      # one chunk: the count pass loops, not the host
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 4, D).astype(np.int64)
    lens[[5, P + 5, 2 * P + 5]] = (150, 0, 1)           # a long, an empty and a one-token document a trip apart
    lens[[6, P + 6, 2 * P + 6]] = 150
    c = _corpus(lens, 9)
    with _sampler(c, K) as g:
        g.sweep(1)
        z = g.z()
        for n, s, mt in ((10, 0.0, 1), (128, 10.0, 1), (64, 1e-3, 5)):
            docs, _, _ = _check(g, c, K, n, s, mt, z)
        assert np.any(docs >= P) and np.any(docs >= 2 * P)


# ------------------------------------------------------------------- chunks
def test_topic_docs_chunks_give_the_default_arrays():
    K, D = 100, 3001
    c = _corpus(_lengths(K + D, D), 5)
    L = capi.load()
    with _sampler(c, K) as g:
        g.sweep(3)
        z = g.z()
        cases = ((10, 0.0, 1), (128, 10.0, 5))
        base = [_check(g, c, K, *case, z) for case in cases]
        try:
            for chunk in (1, 37, 256):
                L.lda_debug_topic_docs_chunk_docs(chunk)
                for case, exp in zip(cases, base):
                    got = g.topic_top_docs(*case)
                    assert all(a.tobytes() == e.tobytes() for a, e in zip(got, exp)), (chunk, case)
        finally:
            L.lda_debug_topic_docs_chunk_docs(0)


# -------------------------------------------------------------- model level
def _model(corpus, K, devices=None, iters=4):
    from ldagibbssampling_amd import topic_model as tm
    il = tm.InstanceList.fromCorpus(corpus)
    for d, inst in enumerate(il):
        inst.source = f"src/file {d}" if d % 2 == 0 else None
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


def test_model_topic_documents_on_one_and_three_shards(tmp_path):
    from ldagibbssampling_amd import topic_model as tm
    K, D = 20, 300
    c = _corpus(_lengths(3, D), 8)
    m1, m3 = _model(c, K), _model(c, K, devices=[0, 0, 0])
    assert m1.numShards() == 1 and m3.numShards() == 3
    names = [f"src/file {d}" if d % 2 == 0 else None for d in range(D)]
    for m in (m1, m3):
        z = m.topicAssignments()
        for n, s, mt in ((10, 10.0, 1), (128, 0.0, 5), (1, 1e-3, 1)):
            docs, w, cnt, lens = m.topicDocuments(n, s, mt)
            exp = N.expected_topic_docs(z, c.doc_off, K, n, s, mt)     # global ids
            for a, e in zip((docs, cnt, lens), exp):
                assert a.dtype == e.dtype
                np.testing.assert_array_equal(a, e)
            ew = N.weights(K, s, cnt, lens)
            assert np.array_equal(w[docs >= 0], ew[docs >= 0]) and np.all(np.isnan(w[docs < 0]))
            assert m.getTopicDocuments(n, s, mt) == \
                [[(int(d), float(x)) for d, x in zip(docs[k], ew[k]) if d >= 0] for k in range(K)]
            text = tm.format_topic_documents(docs, cnt, lens, s, names)
            assert m.topicDocumentsText(n, s, mt) == text
            path = tmp_path / "topic_docs.txt"
            m.printTopicDocuments(path, n, s, mt)
            assert path.read_text() == text
        assert text.startswith("#topic doc name proportion ...\n0 ") and " src/file " in text and " null-source " in text
    # the shards sample the same chain, so the two models' arrays are the same too
    assert m1.topicAssignments().tobytes() == m3.topicAssignments().tobytes()
    for a, b in zip(m1.topicDocuments(64, 10.0, 1), m3.topicDocuments(64, 10.0, 1)):
        assert a.tobytes() == b.tobytes()
    m1.close()
    m3.close()


# --------------------------------------------------------- state and errors
def test_topic_docs_state_and_errors():
    import math
    K = 20
    c = _corpus(_lengths(1, 12), 2)
    with _sampler(c, K) as g:
        # lda_create leaves the shard's counts as the pending delta
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
            g.topic_top_docs(3)
        assert e.value.status == -4
        g.sweep(1)
        ids = np.zeros(K * 129, np.int64)
        out = np.zeros(K * 129, np.int32)
        i, p = ids.ctypes.data, out.ctypes.data
        call = g._L.lda_topic_top_docs
        for n in (0, -1, capi.TOPIC_DOCS_MAX + 1):
            assert call(g._h, n, 0.0, 1, i, p, p) == -1 and b"LDA_TOPIC_DOCS_MAX" in g._L.lda_last_error()
        for s in (-1e-9, math.nan, math.inf):
            assert call(g._h, 3, s, 1, i, p, p) == -1 and b"smoothing" in g._L.lda_last_error()
        for mt in (0, -2):
            assert call(g._h, 3, 0.0, mt, i, p, p) == -1 and b"min_tokens" in g._L.lda_last_error()
        for args in ((None, p, p), (i, None, p), (i, p, None)):
            assert call(g._h, 3, 0.0, 1, *args) == -1 and b"null output" in g._L.lda_last_error()
        assert not ids.any() and not out.any()          # nothing was written
        # a pending delta again: sample() without apply()
        g.sample()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending"):
            g.topic_top_docs(3)
        g.apply()
        a, b = g.topic_top_docs(128, 10.0, 1), g.topic_top_docs(128, 10.0, 1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("D", [0, 3])
def test_topic_docs_without_documents_or_tokens(D):
    """No document (the host answers) and only empty ones (the merge finds
    every list empty): -1 / 0 / 0 everywhere."""
    K = 20
    c = _corpus(np.zeros(D, np.int64), 1)
    with _sampler(c, K) as g:
        g.sweep(1)
        docs, cnt, lens = g.topic_top_docs(7, 10.0, 1)
        assert docs.shape == (K, 7) and np.all(docs == -1) and not cnt.any() and not lens.any()


def test_topic_docs_between_two_sweeps_changes_nothing():
    K = 100
    c = _corpus(_lengths(9, 300), 4)
    with _sampler(c, K, seed=21) as g, _sampler(c, K, seed=21) as ref:
        g.sweep(2)
        ref.sweep(2)
        before = g.counts_checksum()
        assert before == ref.counts_checksum()
        _check(g, c, K, 64, 10.0, 1)
        assert g.counts_checksum() == before
        g.sweep(1)
        ref.sweep(1)
        assert g.z().tobytes() == ref.z().tobytes() and g.counts_checksum() == ref.counts_checksum()
