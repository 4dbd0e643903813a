"""GPU checks of held-out evaluation by document completion:
lda_heldout_loglik (k_doc_completion), lda_doc_completion and the model-level
ldatm_heldout_loglik / ldatm_evaluate / ldatm_set_held_out.

The checker is a numpy fp64 restatement from counts():
    inv = 1 / (nwsum + V beta), u_d = theta_d inv, b_d = beta sum_k u_d[k],
    p_i = u_d . nw[w_i] + b_d, ll_d = sum_i log p_i.

Tolerance (derived, not tuned): all terms of p are non-negative, so p carries
a relative error of at most (K + 8) 2^-53 in any summation order; log adds at
most 1 ulp; ll_d sums L terms of one sign.  Per document
    |delta_d| <= 4 L (K + 16) 2^-53 + 4 |ll_d| (L + 16) 2^-53,
and the total is held to the sum of these bars, also against
oracle.doc_completion_loglik.  Everything else is exact: the empty document's
0.0, total == sum(doc_ll) in order, repeated calls, subsets, chunks, 1 vs 3
shards, theta of doc_completion vs infer, the trace vs evaluate().
"""
import ctypes as C

import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus, document_completion_split

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
BETA = 0.01


def _bars(ll, lens, K):
    lens = np.asarray(lens, np.float64)
    return 4 * lens * (K + 16) * EPS + 4 * np.abs(ll) * (lens + 16) * EPS


def _reference(nw, nwsum, V, beta, theta, off, words):
    """ll_d in numpy fp64 (nw, nwsum already fp64)."""
    inv = 1.0 / (nwsum + V * beta)
    out = np.zeros(len(off) - 1)
    for d in range(len(off) - 1):
        u = theta[d] * inv
        w = words[off[d] - off[0]:off[d + 1] - off[0]]
        if len(w):
            out[d] = np.log(nw[w] @ u + beta * u.sum()).sum()
    return out


def _ordered_sum(x):
    t = 0.0
    for v in x:
        t += float(v)
    return t


def _train_corpus(V, seed=3, n=40):
    """40 training documents whose words come from [0, V - 2): the last two
    word types have empty rows."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(2, 120, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = rng.integers(0, V - 2, int(off[-1])).astype(np.int32)
    return Corpus(off, words, V)


def _held_docs(train, T, seed):
    """Held-out documents at the lengths the kernel can go wrong at: empty, 1,
    one wave's 64 lanes, 65, several batches, and T - 1, T, T + 1 for both
    token batches (16 and 64); the tokens include both empty-row types and the
    most frequent training type."""
    V = train.num_types
    rng = np.random.default_rng(seed)
    lens = [0, 1, 64, 65, 150, 15, 16, 17, 63, T - 1, T, T + 1, 2, 3, 40]
    common = int(np.bincount(train.words, minlength=V).argmax())
    docs = []
    for n in lens:
        w = rng.integers(0, V, n).astype(np.int32)
        if n >= 3:
            w[0], w[n // 2], w[n - 1] = V - 1, common, V - 2
        docs.append(w)
    docs[1][:] = V - 1                      # a one-token document of an empty-row type
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, np.concatenate(docs).astype(np.int32)


def _thetas(K, Q, seed):
    """Dirichlet draws, a one-hot row and a row with half its entries zero."""
    rng = np.random.default_rng(seed)
    t = rng.dirichlet(np.full(K, 0.3), Q)
    t[1] = 0.0
    t[1, K // 3] = 1.0
    t[2, ::2] = 0.0
    t[2] /= t[2].sum()
    return np.ascontiguousarray(t)


CONFIGS = {
    # K = 20: C = 1, the dense quarter-wave default
    "k20_dense": dict(K=20, V=200, sampler="dense", alpha=lambda K: np.full(K, 0.5)),
    # K = 300 pads to Kp = 512 (C = 8); alpha differs per topic
    "k300_padded": dict(K=300, V=200, sampler="dense", alpha=lambda K: 0.05 + 0.4 * np.arange(K) / K),
    # K = 1500: the sparse large-K layout, Kp = 2048, C = 32
    "k1500_sparse": dict(K=1500, V=200, sampler="sparse", alpha=lambda K: np.full(K, 0.1)),
    # K = 4096: C = 64, the widest instantiation
    "k4096_sparse": dict(K=4096, V=50, sampler="sparse", alpha=lambda K: np.full(K, 0.05)),
}
_cache = {}


def _shard(name):
    """One sampler per configuration after 2 sweeps, with its counts in fp64
    (fetched once, shared, never changed)."""
    if name not in _cache:
        from ldagibbssampling_amd.sampler import GibbsSampler
        cfg = CONFIGS[name]
        K = cfg["K"]
        c = _train_corpus(cfg["V"])
        g = GibbsSampler(K, c.num_types, c.doc_off, c.words, cfg["alpha"](K), BETA, seed=9, sampler=cfg["sampler"])
        g.sweep(2)
        nw, nwsum, _, _ = g.counts()
        nwf, nwsumf = nw.astype(np.float64), nwsum.astype(np.float64)
        nwf.setflags(write=False)
        nwsumf.setflags(write=False)
        _cache[name] = (g, c, nwf, nwsumf)
    return _cache[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_heldout_loglik_against_numpy(name, oracle):
    g, c, nw, nwsum = _shard(name)
    K, V = g.K, g.V
    assert g.Kp == capi.padded_topics(K)
    assert nw[V - 2:].sum() == 0                  # the two empty rows
    T = capi.doc_completion_batch(g.Kp // 64)
    off, words = _held_docs(c, T, 17)
    lens = np.diff(off)
    assert {0, 1, 64, 65, 150, T - 1, T, T + 1} <= set(lens.tolist())
    theta = _thetas(K, len(lens), 23)
    doc_ll, total = g.heldout_loglik(theta, off, words)
    ref = _reference(nw, nwsum, V, BETA, theta, off, words)
    bars = _bars(ref, lens, K)
    err = np.abs(doc_ll - ref)
    print(f"{name}: max |delta_d| / bar {np.max(err[lens > 0] / bars[lens > 0]):.3e}")
    assert np.all(err <= bars), (err, bars)
    assert doc_ll[0] == 0.0 and lens[0] == 0      # the empty document, exactly
    assert np.all(doc_ll[lens > 0] < 0.0)
    assert total == _ordered_sum(doc_ll)
    assert abs(total - _ordered_sum(ref)) <= bars.sum()
    ora = oracle.doc_completion_loglik(K, V, nw.astype(np.int32), nwsum.astype(np.int32), BETA, theta, off, words)
    print(f"{name}: |total - oracle| {abs(total - ora):.3e} (bar {bars.sum():.3e})")
    assert abs(total - ora) <= bars.sum()
    # a repeated call: the same bits
    again, total2 = g.heldout_loglik(theta, off, words)
    assert again.tobytes() == doc_ll.tobytes() and total2 == total
    # a permuted subset of the documents: the same per-document bits
    ids = np.random.default_rng(5).permutation(len(lens))[:len(lens) - 4]
    sub_off = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(lens[ids], out=sub_off[1:])
    sub_words = np.concatenate([words[off[d]:off[d + 1]] for d in ids]).astype(np.int32)
    sub, sub_total = g.heldout_loglik(theta[ids], sub_off, sub_words)
    assert sub.tobytes() == doc_ll[ids].tobytes()
    assert sub_total == _ordered_sum(sub)
    # offsets that do not start at zero address words from its first entry
    shifted, _ = g.heldout_loglik(theta, off + 7, words)
    assert shifted.tobytes() == doc_ll.tobytes()


def test_heldout_loglik_chunks():
    """1030 documents at K = 4096 cross the 1024-document chunk (32 MiB of
    staged theta): the same bits as the two halves called separately."""
    g, c, nw, nwsum = _shard("k4096_sparse")
    K, V, Dh = g.K, g.V, 1030
    rng = np.random.default_rng(6)
    lens = rng.integers(1, 4, Dh)
    off = np.zeros(Dh + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    theta = rng.dirichlet(np.full(K, 0.3), Dh)
    doc_ll, total = g.heldout_loglik(theta, off, words)
    h = Dh // 2
    a, ta = g.heldout_loglik(theta[:h], off[:h + 1], words[:off[h]])
    b, tb = g.heldout_loglik(theta[h:], off[h:], words[off[h]:])
    assert doc_ll[:h].tobytes() == a.tobytes() and doc_ll[h:].tobytes() == b.tobytes()
    assert total == _ordered_sum(doc_ll)
    ref = _reference(nw, nwsum, V, BETA, theta, off, words)
    assert np.all(np.abs(doc_ll - ref) <= _bars(ref, lens, K))


def _split(c, n_docs, seed):
    """A 30-document held-out corpus split into observed and scored halves."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 90, n_docs)
    lens[:3] = (0, 1, 2)
    off = np.zeros(n_docs + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    held = Corpus(off, rng.integers(0, c.num_types, int(off[-1])).astype(np.int32), c.num_types)
    return document_completion_split(held)


@pytest.mark.parametrize("name", ["k20_dense", "k300_padded", "k1500_sparse"])
def test_doc_completion_equals_the_old_route(name, oracle):
    g, c, nw, nwsum = _shard(name)
    obs, sc = _split(c, 30, 8)
    args = dict(n_iter=20, thin=4, burn_in=4, seed=7)
    doc_ll, total, theta = g.doc_completion(obs.doc_off, obs.words, sc.doc_off, sc.words, return_theta=True, **args)
    ref_theta = g.infer(obs.doc_off, obs.words, **args)
    assert theta.tobytes() == ref_theta.tobytes()
    plain, plain_total = g.doc_completion(obs.doc_off, obs.words, sc.doc_off, sc.words, **args)
    assert plain.tobytes() == doc_ll.tobytes() and plain_total == total
    given, given_total = g.heldout_loglik(ref_theta, sc.doc_off, sc.words)
    assert given.tobytes() == doc_ll.tobytes() and given_total == total
    ref = _reference(nw, nwsum, g.V, BETA, ref_theta, sc.doc_off, sc.words)
    bars = _bars(ref, np.diff(sc.doc_off), g.K)
    assert np.all(np.abs(doc_ll - ref) <= bars)
    ora = oracle.doc_completion_loglik(g.K, g.V, nw.astype(np.int32), nwsum.astype(np.int32), BETA, ref_theta,
                                       sc.doc_off, sc.words)
    print(f"{name}: |doc_completion - old route| {abs(total - ora):.3e} (bar {bars.sum():.3e})")
    assert abs(total - ora) <= bars.sum()
    assert total == _ordered_sum(doc_ll)


def test_heldout_errors():
    from ldagibbssampling_amd.sampler import GibbsSampler
    K, V = 20, 60
    c = _train_corpus(V, seed=2, n=12)
    off = np.array([0, 3, 3, 7], np.int64)
    words = np.array([1, 5, V - 1, 0, 2, 2, 9], np.int32)
    theta = _thetas(K, 3, 0)
    with GibbsSampler(K, V, c.doc_off, c.words, np.full(K, 0.5), BETA, seed=3) as g:
        g.sweep(1)
        ok, ok_total = g.heldout_loglik(theta, off, words)

        def still_works():
            again, t = g.heldout_loglik(theta, off, words)
            assert again.tobytes() == ok.tobytes() and t == ok_total
            d, _ = g.doc_completion(off, words, off, words, n_iter=4, thin=1, burn_in=1)
            assert d.shape == (3,)

        def refused(status, pattern, fn, *a, **kw):
            with pytest.raises(capi.LdaError, match=pattern) as e:
                fn(*a, **kw)
            assert e.value.status == status
            still_works()

        # null pointers (the Python faces never pass one): the raw entry points
        L, out, tot = g._L, np.zeros(3), C.c_double()
        p = lambda a: a.ctypes.data
        raw = [
            lambda: L.lda_heldout_loglik(None, 3, p(theta), p(off), p(words), p(out), None),
            lambda: L.lda_heldout_loglik(g._h, 3, None, p(off), p(words), p(out), None),
            lambda: L.lda_heldout_loglik(g._h, 3, p(theta), None, p(words), p(out), None),
            lambda: L.lda_heldout_loglik(g._h, 3, p(theta), p(off), None, p(out), None),
            lambda: L.lda_heldout_loglik(g._h, 3, p(theta), p(off), p(words), None, None),
            lambda: L.lda_doc_completion(None, 3, p(off), p(words), p(off), p(words), 4, 1, 1, 0, p(out), None, None),
            lambda: L.lda_doc_completion(g._h, 3, None, p(words), p(off), p(words), 4, 1, 1, 0, p(out), None, None),
            lambda: L.lda_doc_completion(g._h, 3, p(off), p(words), None, p(words), 4, 1, 1, 0, p(out), None, None),
            lambda: L.lda_doc_completion(g._h, 3, p(off), p(words), p(off), None, 4, 1, 1, 0, p(out), None, None),
            lambda: L.lda_doc_completion(g._h, 3, p(off), p(words), p(off), p(words), 4, 1, 1, 0, None, None, None),
        ]
        for call in raw:
            assert call() == -1
            assert b"null" in L.lda_last_error()
            still_works()
        # total may be null
        assert L.lda_heldout_loglik(g._h, 3, p(theta), p(off), p(words), p(out), None) == 0
        assert out.tobytes() == ok.tobytes()

        bad_off = np.array([0, 5, 3, 7], np.int64)
        refused(-1, "LDA_ERR_INVALID_ARG: .*monotone", g.heldout_loglik, theta, bad_off, words)
        refused(-1, "LDA_ERR_INVALID_ARG: .*monotone", g.doc_completion, off, words, bad_off, words)
        refused(-1, "LDA_ERR_INVALID_ARG: .*monotone", g.doc_completion, bad_off, words, off, words)
        for w_bad in (V, -1):
            bad = words.copy()
            bad[4] = w_bad
            refused(-1, "LDA_ERR_INVALID_ARG: .*word id", g.heldout_loglik, theta, off, bad)
            refused(-1, "LDA_ERR_INVALID_ARG: .*word id", g.doc_completion, off, words, off, bad)
            refused(-1, "LDA_ERR_INVALID_ARG: .*word id", g.doc_completion, off, bad, off, words)
        bad = theta.copy()
        bad[0, 0] = -0.25
        refused(-1, "LDA_ERR_INVALID_ARG: .*negative", g.heldout_loglik, bad, off, words)
        for v in (np.nan, np.inf):
            bad = theta.copy()
            bad[2, 4] = v
            refused(-1, "LDA_ERR_INVALID_ARG: .*non-finite", g.heldout_loglik, bad, off, words)
        bad = theta.copy()
        bad[1] = 0.0
        refused(-1, "LDA_ERR_INVALID_ARG: .*sums to zero", g.heldout_loglik, bad, off, words)
        # Dh = 0 succeeds
        e, t = g.heldout_loglik(np.zeros((0, K)), [0], [])
        assert e.shape == (0,) and t == 0.0
        e, t = g.doc_completion([0], [], [0], [])
        assert e.shape == (0,) and t == 0.0
        # a pending delta: sample() without apply()
        g.sample()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
            g.heldout_loglik(theta, off, words)
        assert e.value.status == -4
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
            g.doc_completion(off, words, off, words)
        assert e.value.status == -4
        g.apply()
        d, _ = g.heldout_loglik(theta, off, words)
        assert d.shape == (3,) and np.all(np.isfinite(d))


# ------------------------------------------------------------- model level
def _model(corpus, K, devices=None, iters=6, optimize=0, burnin=200, start=True):
    from ldagibbssampling_amd import topic_model as tm
    il = tm.InstanceList.fromCorpus(corpus)
    m = tm.ParallelTopicModel(K, 0.5 * K, BETA)
    m.setRandomSeed(13)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(iters)
    m.setOptimizeInterval(optimize)
    m.setBurninPeriod(burnin)
    if devices is not None:
        m.setDevices(devices)
    m.addInstances(il)
    if start:
        m.estimate()
    return m


def _held_instances(V, seed, n=12):
    """Held-out documents with out-of-vocabulary ids (V + 5, -3) among them."""
    from ldagibbssampling_amd import topic_model as tm
    rng = np.random.default_rng(seed)
    docs = []
    for L in [0, 1, 2, 33] + rng.integers(5, 80, n - 4).tolist():
        w = rng.integers(0, V, L).astype(np.int32)
        if L >= 5:
            w[1], w[L - 2] = V + 5, -3
        docs.append(tm.Instance(w))
    return docs


def test_model_evaluation_does_not_depend_on_the_shards():
    from ldagibbssampling_amd import topic_model as tm
    K, V = 20, 150
    c = _train_corpus(V, seed=8, n=60)
    one = _model(c, K, devices=[0])
    three = _model(c, K, devices=[0, 0, 0])
    assert one.numShards() == 1 and three.numShards() == 3
    np.testing.assert_array_equal(one.topicAssignments(), three.topicAssignments())
    held = _held_instances(V, 4)
    args = dict(numIterations=20, thinning=4, burnIn=4, seed=5)
    a = one.getHeldOutEvaluator().evaluate(held, **args)
    b = three.getHeldOutEvaluator().evaluate(held, **args)
    assert a.perDocument.tobytes() == b.perDocument.tobytes() and a.theta.tobytes() == b.theta.tobytes()
    assert a.logLikelihood == b.logLikelihood and a.tokens == b.tokens
    # the pieces of evaluate(): the split, the inferencer's theta, the scored halves
    obs_off, obs, sc_off, sc = tm.completion_split(held, V)
    assert a.tokens == len(sc) == sum((((x.data >= 0) & (x.data < V)).sum() + 1) // 2 for x in held)
    observed = [tm.Instance(obs[obs_off[d]:obs_off[d + 1]]) for d in range(len(held))]
    ref_theta = one.getInferencer().getSampledDistributions(observed, 20, 4, 4, seed=5)
    assert a.theta.tobytes() == ref_theta.tobytes()
    la, ta = one.heldOutLogLikelihood(a.theta, sc_off, sc)
    lb, tb = three.heldOutLogLikelihood(a.theta, sc_off, sc)
    assert la.tobytes() == lb.tobytes() == a.perDocument.tobytes() and ta == tb == a.logLikelihood
    assert a.logLikelihood == _ordered_sum(a.perDocument)
    assert a.perplexity == float(np.exp(-a.logLikelihood / a.tokens))
    # against numpy, from the model's counts
    nw, nwsum = one.typeTopicCounts()
    ref = _reference(nw.astype(np.float64), nwsum.astype(np.float64), V, BETA, a.theta, sc_off, sc)
    assert np.all(np.abs(a.perDocument - ref) <= _bars(ref, np.diff(sc_off), K))
    with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*word id"):
        three.heldOutLogLikelihood(a.theta, sc_off, np.where(sc == sc[0], V, sc))
    one.close()
    three.close()


def test_held_out_trace_leaves_training_unchanged():
    K, V = 20, 150
    c = _train_corpus(V, seed=9, n=60)
    held = _held_instances(V, 6)
    args = dict(numIterations=20, thinning=4, burnIn=4, seed=11)
    plain = _model(c, K, iters=40, optimize=10, burnin=10)
    traced = _model(c, K, iters=40, optimize=10, burnin=10, start=False)
    traced.setHeldOut(held, 20, **args)
    traced.estimate()
    assert plain.heldOutTrace() == []
    np.testing.assert_array_equal(traced.topicAssignments(), plain.topicAssignments())
    assert traced.alpha.tobytes() == plain.alpha.tobytes()
    assert traced.beta == plain.beta and traced.alphaSum == plain.alphaSum
    assert not np.all(traced.alpha == traced.alpha[0])           # the optimisation did run
    assert traced.llTrace() == plain.llTrace()
    trace = traced.heldOutTrace()
    assert [it for it, _ in trace] == [20, 40]
    res = traced.getHeldOutEvaluator().evaluate(held, **args)
    assert trace[-1][1] == res.logLikelihood / res.tokens
    assert trace[0][1] != trace[1][1] and all(np.isfinite(v) and v < 0 for _, v in trace)
    # interval 0 turns it off again
    traced.setHeldOut(held, 0)
    traced.setNumIterations(20)
    traced.estimate()
    assert traced.heldOutTrace() == []
    plain.close()
    traced.close()
