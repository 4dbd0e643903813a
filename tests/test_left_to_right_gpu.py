"""GPU checks of the left-to-right estimator: lda_left_to_right
(k_left_to_right, k_ltr_reduce) and the model-level ldatm_left_to_right /
MarginalProbEstimator, against the numpy restatement in ltr_numpy.py.

Tolerances (derived, not tuned).  Every weight is a product of positive fp64
factors and W, the prefixes and the particle sum add K <= 1500 (R <= 16)
positive terms, so in any summation order they carry a relative error of at
most (K + 8) 2^-53 < 2e-13: p_r, phat and doc_ll (a sum of logs of one sign)
are held to 1e-11 relative (1e-12 where a single W is compared), and a drawn
topic's prefix interval is widened by 1e-12 W.  The statistical bars bound the
standard error by the range of p_r[i] (6 (hi - lo) / 2 / sqrt(M R)); counts,
totals, repeated calls, subsets, chunks, particle prefixes and 1 vs 3 shards
are exact.
"""
import ctypes as C
import io
import itertools

import numpy as np
import pytest

import ltr_numpy as N
from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu
BETA = 0.01
LENGTHS = (0, 1, 2, 5, 17, 64, 65, 130)
CONFIGS = {
    # K: (V, sampler, alpha); C = Kp / 64 = 1, 1, 2, 8, 32
    3: (50, "dense", lambda K: np.array([0.3, 0.2, 0.4])),
    20: (200, "dense", lambda K: np.full(K, 0.5)),
    100: (300, "dense", lambda K: 0.05 + 0.4 * np.arange(K) / K),
    512: (200, "dense", lambda K: np.full(K, 0.1)),
    1500: (120, "sparse", lambda K: 0.02 + 0.1 * (np.arange(K) % 7)),
}
_cache = {}


def _ordered_sum(x):
    t = 0.0
    for v in x:
        t += float(v)
    return t


def _train_corpus(V, seed=3, n=40):
    """Training documents that hold every word type of [0, V - 2) and no
    other: exactly the last two types have empty rows."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, 60, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = rng.integers(0, V - 2, int(off[-1])).astype(np.int32)
    assert len(words) >= V - 2
    words[rng.permutation(len(words))[:V - 2]] = np.arange(V - 2, dtype=np.int32)
    return Corpus(off, words, V)


def _shard(K):
    """One sampler per K after 3 sweeps, with its counts and phi (fetched
    once, shared, never changed)."""
    if K not in _cache:
        from ldagibbssampling_amd.sampler import GibbsSampler
        V, sampler, alpha = CONFIGS[K]
        c = _train_corpus(V)
        g = GibbsSampler(K, V, c.doc_off, c.words, alpha(K), BETA, seed=9, sampler=sampler)
        g.sweep(3)
        nw, nwsum, _, _ = g.counts()
        phi = N.phi_table(nw, nwsum, BETA)
        for a in (nw, phi):
            a.setflags(write=False)
        _cache[K] = (g, alpha(K), nw, phi)
    return _cache[K]


def _held_docs(V, seed, lengths=LENGTHS, end_skipped=True):
    """Held-out documents of the given lengths; from 5 tokens on they hold
    both empty-row types (V - 1 inside, V - 2 last, or last but one without
    end_skipped); then a document of empty-row types only."""
    rng = np.random.default_rng(seed)
    docs = []
    for n in lengths:
        w = rng.integers(0, V - 2, n).astype(np.int32)
        if n >= 5:
            w[n // 2], w[n - 1 if end_skipped else n - 2] = V - 1, V - 2
        docs.append(w)
    docs.append(np.array([V - 1, V - 2, V - 1], np.int32))
    off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return off, np.concatenate(docs).astype(np.int32)


def _phat_from_z(phi, alpha, off, words, skip, z, upto_last=False):
    """phat per token recomputed from the particles' topics (every position,
    or each document's last scored one)."""
    R = z.shape[0]
    out = np.zeros(len(words))
    for d in range(len(off) - 1):
        s = slice(off[d], off[d + 1])
        doc, sk = words[s], skip[s]
        kept = np.nonzero(~sk)[0]
        if not len(kept):
            continue
        upto = int(kept[-1]) if upto_last else None
        p = np.array([N.p_from_z(phi, alpha, doc, sk, z[r, s], upto) for r in range(R)])
        out[s] = N.estimate(p)[0]
    return out


def test_deterministic_cases():
    g, alpha, nw, phi = _shard(20)
    V, A = g.V, float(np.sum(alpha))
    off, words = _held_docs(V, 5)
    skip = N.skipped(nw, words)
    assert skip.sum() == 2 * sum(n >= 5 for n in LENGTHS) + 3
    for resampling in (False, True):
        doc_ll, total, tokens, tp, z = g.left_to_right(off, words, 3, resampling, seed=4, token_prob=True, z=True)
        assert tokens == int((~skip).sum())
        assert total == _ordered_sum(doc_ll)
        # skipped tokens: no probability, no topic, in every particle
        assert np.all(tp[skip] == 0.0) and np.all(z[:, skip] == -1)
        assert np.all(tp[~skip] > 0.0) and np.all((z[:, ~skip] >= 0) & (z[:, ~skip] < g.K))
        # position 0 of every document (none of these starts with a skipped token)
        for d in range(len(off) - 2):
            if off[d + 1] > off[d]:
                w0 = words[off[d]]
                ref = float(np.sum(alpha * phi[w0])) / A
                assert abs(tp[off[d]] - ref) <= 1e-12 * ref, d
        # the one-token document: doc_ll is the log of that
        one = LENGTHS.index(1)
        assert abs(doc_ll[one] - np.log(tp[off[one]])) <= 1e-12 * abs(doc_ll[one])
        # the empty and the all-skipped document, exactly
        assert doc_ll[LENGTHS.index(0)] == 0.0 and doc_ll[-1] == 0.0
        assert np.all(doc_ll[[i for i, n in enumerate(LENGTHS) if n]] < 0.0)
    # a call of empty documents only, and one whose only document is all skipped
    e, t, n = g.left_to_right([0, 0, 0], [], 2)
    assert e.tolist() == [0.0, 0.0] and t == 0.0 and n == 0
    e, t, n, tp, z = g.left_to_right([0, 2], [V - 1, V - 2], 2, token_prob=True, z=True)
    assert e.tolist() == [0.0] and n == 0 and tp.tolist() == [0.0, 0.0] and np.all(z == -1)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("K", list(CONFIGS))
def test_every_draw_without_resampling(K, R, oracle):
    g, alpha, nw, phi = _shard(K)
    assert g.Kp // 64 == {3: 1, 20: 1, 100: 2, 512: 8, 1500: 32}[K]
    off, words = _held_docs(g.V, 7 + K)
    skip = N.skipped(nw, words)
    seed = 1234 + K
    doc_ll, total, tokens, tp, z = g.left_to_right(off, words, R, False, seed=seed, token_prob=True, z=True)
    assert z.shape == (R, len(words)) and tokens == int((~skip).sum()) and total == _ordered_sum(doc_ll)
    assert np.all(z[:, skip] == -1) and np.all((z[:, ~skip] >= 0) & (z[:, ~skip] < K))
    # p_r[i] from the topics before i (final once drawn), hence phat and doc_ll
    ref = _phat_from_z(phi, alpha, off, words, skip, z)
    np.testing.assert_allclose(tp, ref, rtol=1e-11, atol=0.0)
    for d in range(len(off) - 1):
        r = ref[off[d]:off[d + 1]]
        ll = float(np.sum(np.log(r[r > 0])))
        assert abs(doc_ll[d] - ll) <= 1e-11 * abs(ll), d
    # each drawn topic's prefix interval holds u W
    worst = 0.0
    for r in range(R):
        for d in range(len(off) - 1):
            nd = np.zeros(K)
            for i in range(off[d], off[d + 1]):
                if skip[i]:
                    continue
                pre = np.cumsum(N.weights(phi, alpha, nd, words[i]))
                W, k = pre[-1], z[r, i]
                t = N.uniform(seed, int(i), int(i - off[d]), r) * W
                lo = pre[k - 1] if k else 0.0
                assert lo - 1e-12 * W <= t, (r, d, i)
                assert t < pre[k] + 1e-12 * W, (r, d, i)
                worst = max(worst, (lo - t) / W, (t - pre[k]) / W)
                nd[k] += 1
    print(f"K={K} R={R}: the worst excursion of u W out of its interval {worst:.3e} W")


@pytest.mark.parametrize("K", [20, 512])
def test_last_position_with_resampling(K):
    """p_r of a document's last scored position saw the topics that the pass
    of its own limit left, and z_out holds those only if no later limit
    resampled them again: the documents end with a scored token."""
    g, alpha, nw, phi = _shard(K)
    off, words = _held_docs(g.V, 21, end_skipped=False)
    skip = N.skipped(nw, words)
    assert not skip[off[1:-1] - 1][np.diff(off[:-1]) > 0].any()
    doc_ll, total, tokens, tp, z = g.left_to_right(off, words, 2, True, seed=77, token_prob=True, z=True)
    assert np.all((z >= -1) & (z < K)) and np.all((z == -1) == skip[None, :])
    assert tokens == int((~skip).sum()) and total == _ordered_sum(doc_ll)
    ref = _phat_from_z(phi, alpha, off, words, skip, z, upto_last=True)
    last = ref > 0
    assert last.sum() == sum(n > 0 for n in LENGTHS)
    np.testing.assert_allclose(tp[last], ref[last], rtol=1e-11, atol=0.0)
    # the resampling passes moved topics: the final z is not the no-resampling one
    _, _, _, z0 = g.left_to_right(off, words, 2, False, seed=77, z=True)
    assert not np.array_equal(z0, z)


# ------------------------------------------------------ exact expectation
def _tiny():
    """K = 3, V = 5 (type 4 never occurs) on a corpus with three clear
    topics; the 5-token document [a, b, 4, c, d] whose two modes differ most,
    found by enumeration.  Shared by the two tests below."""
    if "tiny" not in _cache:
        from ldagibbssampling_amd.sampler import GibbsSampler
        docs = []
        for _ in range(6):
            docs += [[0] * 8 + [3] * 2, [1] * 8 + [3], [2] * 9, [0] * 4 + [3] * 3, [1] * 5 + [2]]
        off = np.zeros(len(docs) + 1, np.int64)
        np.cumsum([len(d) for d in docs], out=off[1:])
        alpha = np.array([0.3, 0.2, 0.4])
        g = GibbsSampler(3, 5, off, np.concatenate(docs).astype(np.int32), alpha, BETA, seed=2)
        g.sweep(20)
        nw, nwsum, _, _ = g.counts()
        assert nw[4].sum() == 0
        phi = N.phi_table(nw, nwsum, BETA)
        M, R = 2000, 16
        best = None
        for a, b, c, d in itertools.product(range(4), repeat=4):
            doc = [a, b, 4, c, d]
            skip = N.skipped(nw, doc)
            ex = [N.exact(phi, alpha, doc, skip, mode) for mode in (False, True)]
            for i in (3, 4):
                bar = max(6 * (e[0][i][2] - e[0][i][1]) / 2 / np.sqrt(M * R) + 1e-12 for e in ex)
                sep = abs(ex[0][0][i][0] - ex[1][0][i][0]) / bar
                if best is None or sep > best[0]:
                    best = (sep, doc, i, ex)
        _cache["tiny"] = (g, alpha, nw, phi, M, R) + best
    return _cache["tiny"]


@pytest.mark.parametrize("resampling", [False, True])
def test_exact_expectation(resampling):
    g, alpha, nw, phi, M, R, sep, doc, pos, ex = _tiny()
    assert sep > 3.0, (sep, doc, pos)            # the two modes are told apart at `pos`
    off = 5 * np.arange(M + 1, dtype=np.int64)
    words = np.tile(np.array(doc, np.int32), M)
    doc_ll, total, tokens, tp = g.left_to_right(off, words, R, resampling, seed=31, token_prob=True)
    assert tokens == 4 * M
    mean = tp.reshape(M, 5).mean(axis=0)
    assert mean[2] == 0.0 and ex[resampling][0][2] is None
    for i in (0, 1, 3, 4):
        e, lo, hi = ex[resampling][0][i]
        bar = 6 * (hi - lo) / 2 / np.sqrt(M * R) + 1e-12
        print(f"resampling={resampling} position {i}: mean {mean[i]:.6f} E {e:.6f} bar {bar:.2e}")
        assert abs(mean[i] - e) <= bar, i
    # ... and it is not the other mode's expectation
    other = ex[not resampling][0][pos]
    assert abs(mean[pos] - other[0]) > 6 * (other[2] - other[1]) / 2 / np.sqrt(M * R) + 1e-12


def test_single_particle_weight_is_unbiased():
    """R = 1 without resampling: exp(doc_ll) is an unbiased estimate of the
    enumerated marginal p(w); the bar is 6 standard errors of the restated
    sampler's own weights over as many runs."""
    g, alpha, nw, phi, M, R, sep, doc, pos, ex = _tiny()
    marginal = ex[0][1]
    skip = N.skipped(nw, doc)
    rng = np.random.default_rng(5)
    w = np.array([N.run_particle(phi, alpha, doc, skip, False, lambda j, i: rng.random())[0][~skip].prod()
                  for _ in range(M)])
    se = w.std(ddof=1) / np.sqrt(M)
    off = 5 * np.arange(M + 1, dtype=np.int64)
    doc_ll, _, _ = g.left_to_right(off, np.tile(np.array(doc, np.int32), M), 1, False, seed=8)
    got = float(np.exp(doc_ll).mean())
    print(f"marginal {marginal:.6e}, device {got:.6e}, numpy sampler {w.mean():.6e} +- {se:.2e}")
    assert abs(got - marginal) <= 6 * se


# ------------------------------------------- repeatability and independence
@pytest.mark.parametrize("resampling", [False, True])
def test_repeatable_and_independent(resampling):
    g, alpha, nw, phi = _shard(100)
    off, words = _held_docs(g.V, 40, lengths=(3, 0, 17, 70, 1, 33))
    args = dict(resampling=resampling, seed=19, token_prob=True, z=True)
    ll, total, tokens, tp, z = g.left_to_right(off, words, 3, **args)
    again = g.left_to_right(off, words, 3, **args)
    assert again[0].tobytes() == ll.tobytes() and again[1:3] == (total, tokens)
    assert again[3].tobytes() == tp.tobytes() and again[4].tobytes() == z.tobytes()
    # documents appended after: the first ones keep their bits
    off2, words2 = _held_docs(g.V, 41, lengths=(9, 64))
    both_off = np.concatenate([off, off[-1] + off2[1:]])
    both = g.left_to_right(both_off, np.concatenate([words, words2]), 3, **args)
    assert both[0][:len(ll)].tobytes() == ll.tobytes() and both[3][:len(tp)].tobytes() == tp.tobytes()
    assert both[4][:, :len(words)].tobytes() == z.tobytes()
    # offsets that do not start at zero address words from its first entry
    shifted = g.left_to_right(off + 11, words, 3, **args)
    assert shifted[0].tobytes() == ll.tobytes()
    # small chunks (the test hook): 3 particles x 20 tokens a chunk
    try:
        g._L.lda_debug_ltr_chunk_cells(60)
        cut = g.left_to_right(off, words, 3, **args)
    finally:
        g._L.lda_debug_ltr_chunk_cells(0)
    assert cut[0].tobytes() == ll.tobytes() and cut[1:3] == (total, tokens)
    assert cut[3].tobytes() == tp.tobytes() and cut[4].tobytes() == z.tobytes()
    # the particles of a call are the first ones of a call with more
    more = g.left_to_right(off, words, 5, **args)
    assert more[4][:3].tobytes() == z.tobytes() and more[2] == tokens
    # another seed draws other topics
    assert g.left_to_right(off, words, 3, resampling, seed=20, z=True)[3].tobytes() != z.tobytes()


def test_errors_and_limits():
    from ldagibbssampling_amd.sampler import GibbsSampler
    K, V = 20, 60
    c = _train_corpus(V, seed=2, n=12)
    off = np.array([0, 3, 3, 7], np.int64)
    words = np.array([1, 5, V - 1, 0, 2, 2, 9], np.int32)
    with GibbsSampler(K, V, c.doc_off, c.words, np.full(K, 0.5), BETA, seed=3) as g:
        g.sweep(1)
        ok = g.left_to_right(off, words, 2, seed=1)

        def still_works():
            again = g.left_to_right(off, words, 2, seed=1)
            assert again[0].tobytes() == ok[0].tobytes() and again[1:] == ok[1:]

        def refused(status, pattern, *a, **kw):
            with pytest.raises(capi.LdaError, match=pattern) as e:
                g.left_to_right(*a, **kw)
            assert e.value.status == status
            still_works()

        L, out = g._L, np.zeros(3)
        p = lambda a: a.ctypes.data
        for call in (lambda: L.lda_left_to_right(None, 3, p(off), p(words), 2, 1, 0, p(out), None, None, None, None),
                     lambda: L.lda_left_to_right(g._h, 3, None, p(words), 2, 1, 0, p(out), None, None, None, None),
                     lambda: L.lda_left_to_right(g._h, 3, p(off), None, 2, 1, 0, p(out), None, None, None, None),
                     lambda: L.lda_left_to_right(g._h, 3, p(off), p(words), 2, 1, 0, None, None, None, None, None)):
            assert call() == -1
            assert b"null" in L.lda_last_error()
            still_works()
        assert L.lda_left_to_right(g._h, -1, p(off), p(words), 2, 1, 0, p(out), None, None, None, None) == -1
        assert L.lda_left_to_right(g._h, 3, p(off), p(words), 0, 1, 0, p(out), None, None, None, None) == -1
        assert b"num_particles" in L.lda_last_error()
        # every output but doc_ll may be null
        assert L.lda_left_to_right(g._h, 3, p(off), p(words), 2, 1, 1, p(out), None, None, None, None) == 0
        assert out.tobytes() == ok[0].tobytes()
        refused(-1, "LDA_ERR_INVALID_ARG: .*monotone", np.array([0, 5, 3, 7], np.int64), words, 2)
        for w_bad in (V, -1):
            bad = words.copy()
            bad[4] = w_bad
            refused(-1, "LDA_ERR_INVALID_ARG: .*word id", off, bad, 2)
        # the limits
        refused(-5, "LDA_ERR_UNSUPPORTED: .*PARTICLES", off, words, capi.LTR_MAX_PARTICLES + 1)
        long_doc = np.zeros(capi.LTR_MAX_DOC_TOKENS + 1, np.int32)
        refused(-5, "LDA_ERR_UNSUPPORTED: .*DOC_TOKENS", [0, len(long_doc)], long_doc, 1, False)
        # Dh = 0 succeeds
        e, t, n = g.left_to_right([0], [], 4)
        assert e.shape == (0,) and t == 0.0 and n == 0
        # a pending delta: sample() without apply()
        g.sample()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
            g.left_to_right(off, words, 2)
        assert e.value.status == -4
        g.apply()
        assert np.all(np.isfinite(g.left_to_right(off, words, 2)[0]))


# ------------------------------------------------------------- model level
def _model(corpus, K, devices=None):
    from ldagibbssampling_amd import topic_model as tm
    m = tm.ParallelTopicModel(K, 0.5 * K, BETA)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(6)
    m.setOptimizeInterval(0)
    if devices is not None:
        m.setDevices(devices)
    m.addInstances(tm.InstanceList.fromCorpus(corpus))
    m.estimate()
    return m


def test_model_level():
    from ldagibbssampling_amd import topic_model as tm
    K, V = 20, 150
    c = _train_corpus(V, seed=8, n=60)
    one = _model(c, K, devices=[0])
    three = _model(c, K, devices=[0, 0, 0])
    assert one.numShards() == 1 and three.numShards() == 3
    rng = np.random.default_rng(4)
    raw = [rng.integers(0, V - 2, n).astype(np.int32) for n in (0, 1, 2, 33, 12, 70)]
    dirty = [w.copy() for w in raw]
    for i in (3, 4, 5):                            # out-of-vocabulary ids among them
        dirty[i] = np.insert(dirty[i], [1, len(dirty[i]) - 2], [V + 5, -3]).astype(np.int32)
    held, clean = [tm.Instance(w) for w in dirty], [tm.Instance(w) for w in raw]
    state = (one.topicAssignments().copy(), one.alpha.copy(), one.beta, [x.copy() for x in one.typeTopicCounts()])
    est = one.getProbEstimator()
    for resampling in (True, False):
        a = est.leftToRight(held, 4, resampling, seed=5)
        b = three.getProbEstimator().leftToRight(held, 4, resampling, seed=5)
        assert a.perDocument.tobytes() == b.perDocument.tobytes()
        assert a.logLikelihood == b.logLikelihood and a.tokens == b.tokens
        # out-of-vocabulary ids are dropped and not counted
        k = est.leftToRight(clean, 4, resampling, seed=5)
        assert k.perDocument.tobytes() == a.perDocument.tobytes() and k.tokens == a.tokens == sum(map(len, raw))
        assert a.logLikelihood == _ordered_sum(a.perDocument)
        assert a.perplexity == float(np.exp(-a.logLikelihood / a.tokens))
    # Mallet's signature: the total, and one line per document in the stream
    out = io.StringIO()
    total = est.evaluateLeftToRight(held, 4, True, out)
    r = est.leftToRight(held, 4, True)
    assert total == r.logLikelihood == _ordered_sum(r.perDocument)
    lines = out.getvalue().splitlines()
    assert len(lines) == len(held) and [float(x) for x in lines] == r.perDocument.tolist()
    assert est.evaluateLeftToRight(held, 4, True) == total
    # against the sampler-level call on the same counts: position 0 by hand
    nw, nwsum = one.typeTopicCounts()
    phi = N.phi_table(nw, nwsum, BETA)
    single = est.leftToRight([tm.Instance(raw[1])], 3)
    ref = np.log(np.sum(one.alpha * phi[raw[1][0]]) / np.sum(one.alpha))
    assert abs(single.logLikelihood - ref) <= 1e-12 * abs(ref) and single.tokens == 1
    # the limits
    with pytest.raises(capi.LdaError, match="LDA_ERR_UNSUPPORTED") as e:
        est.leftToRight(held, capi.LTR_MAX_PARTICLES + 1)
    assert e.value.status == -5
    with pytest.raises(capi.LdaError, match="LDA_ERR_UNSUPPORTED") as e:
        est.leftToRight([tm.Instance(np.zeros(capi.LTR_MAX_DOC_TOKENS + 1, np.int32))], 1, False)
    assert e.value.status == -5
    # the model is the same bits as before
    np.testing.assert_array_equal(one.topicAssignments(), state[0])
    assert one.alpha.tobytes() == state[1].tobytes() and one.beta == state[2]
    for x, y in zip(one.typeTopicCounts(), state[3]):
        np.testing.assert_array_equal(x, y)
    one.close()
    three.close()
