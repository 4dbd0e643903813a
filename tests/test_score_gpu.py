"""GPU checks of prediction scoring: lda_score_docs (k_doc_scores) and the
model-level ldatm_score_theta / ldatm_score / ldatm_score_top.

The checker is a numpy fp64 restatement: p = (nd + alpha) / (ndsum + A) from
counts(), then the textbook cosine / mean squared difference.

Tolerance (derived, not tuned): every sum in the kernel's formulas
    dot = sum_k c_k theta_q[k] + alpha . theta_q,
    n2  = sum_{c_k > 0} c_k (c_k + 2 alpha_k) + sum alpha^2
has non-negative terms, so each carries a relative error of at most
(terms) 2^-53 in whatever order it is added; a document contributes at most
Lmax terms and the constants K.  Cosine: rtol = 4 (Lmax + K + 16) 2^-53.
mse cancels, so its bar is absolute: atol = 8 (Lmax + K + 16) 2^-53 / K.
Everything else is exact: repeated calls, 1 vs 3 shards, docs=None vs the
same documents listed.
"""
import numpy as np
import pytest

from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def _bars(Lmax, K):
    return 4 * (Lmax + K + 16) * EPS, 8 * (Lmax + K + 16) * EPS / K


def _corpus(lengths, V, seed):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    return Corpus(off, words, V)


def _lengths(seed, n=40, empties=1):
    """The edge lengths the kernel can go wrong at (empty, 1, one wave's 64
    lanes, 65, several passes) among ordinary ones, shuffled."""
    rng = np.random.default_rng(seed)
    fixed = [0] * empties + [1, 64, 65, 150]
    rest = rng.integers(2, 120, n - len(fixed)).tolist()
    lens = np.array(fixed + rest, np.int64)
    rng.shuffle(lens)
    return lens


def _thetas(K, Q, seed):
    """Dirichlet draws, with a one-hot row and a row with zeros when Q allows."""
    rng = np.random.default_rng(seed)
    t = rng.dirichlet(np.full(K, 0.3), Q)
    if Q >= 2:
        t[1] = 0.0
        t[1, K // 3] = 1.0
    if Q >= 3:
        t[2, ::2] = 0.0
        t[2] /= t[2].sum()
    return np.ascontiguousarray(t)


def _probabilities(nd, ndsum, alpha):
    return (nd + alpha[None, :]) / (ndsum[:, None] + alpha.sum())


def _cosine(theta, p):
    return (theta @ p.T) / (np.linalg.norm(theta, axis=1)[:, None] * np.linalg.norm(p, axis=1)[None, :])


def _mse(theta, p):
    return ((theta[:, None, :] - p[None, :, :]) ** 2).mean(axis=2)


def _check(got, theta, p, metric, Lmax, K):
    rtol, atol = _bars(Lmax, K)
    if metric == "cosine":
        ref = _cosine(theta, p)
        err = np.abs(got - ref) / np.abs(ref)
        print(f"cosine K={K} Q={len(theta)} M={p.shape[0]}: max rel err {err.max():.3e} (bar {rtol:.3e})")
        assert np.all(err <= rtol), (err.max(), rtol)
    else:
        ref = _mse(theta, p)
        err = np.abs(got - ref)
        print(f"mse K={K} Q={len(theta)} M={p.shape[0]}: max abs err {err.max():.3e} (bar {atol:.3e})")
        assert np.all(err <= atol), (err.max(), atol)


CONFIGS = {
    # K = 20: the dense quarter-wave default
    "k20_dense": dict(K=20, sampler="dense", alpha=lambda K: np.full(K, 0.5)),
    # K = 300 pads to Kp = 512; alpha differs per topic
    "k300_padded": dict(K=300, sampler="dense", alpha=lambda K: 0.05 + 0.4 * np.arange(K) / K),
    # K = 1500: the sparse large-K layout, Kp = 2048 (32 KB of LDS histograms per block)
    "k1500_sparse": dict(K=1500, sampler="sparse", alpha=lambda K: np.full(K, 0.1)),
}
_cache = {}


def _shard(name):
    """One sampler per configuration after 2 sweeps, with its numpy reference
    (computed once, shared, never changed)."""
    if name not in _cache:
        from ldagibbssampling_amd.sampler import GibbsSampler
        cfg = CONFIGS[name]
        K = cfg["K"]
        c = _corpus(_lengths(11), 200, 3)
        alpha = cfg["alpha"](K)
        g = GibbsSampler(K, c.num_types, c.doc_off, c.words, alpha, 0.01, seed=9, sampler=cfg["sampler"])
        g.sweep(2)
        _, _, nd, ndsum = g.counts(with_nd=True)
        p = _probabilities(nd.astype(np.float64), ndsum.astype(np.float64), alpha)
        p.setflags(write=False)
        _cache[name] = (g, c, alpha, p)
    return _cache[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_score_docs_against_numpy(name):
    g, c, alpha, p = _shard(name)
    K, D = g.K, c.num_docs
    assert g.Kp == capi.padded_topics(K)
    lens = np.diff(c.doc_off)
    assert {0, 1, 64, 65, 150} <= set(lens.tolist())
    Lmax = int(lens.max())
    rng = np.random.default_rng(5)
    for Q in (1, 3, 17):
        theta = _thetas(K, Q, 100 + Q)
        for metric in ("cosine", "mse"):
            full = g.score_docs(theta, metric)
            assert full.shape == (Q, D)
            _check(full, theta, p, metric, Lmax, K)
            # a sub-range with doc_begin > 0: the same bits as the full call's columns
            sub = g.score_docs(theta, metric, doc_begin=7, num_docs=D - 12)
            np.testing.assert_array_equal(sub, full[:, 7:D - 5])
            # a shuffled list with a duplicate
            ids = rng.permutation(D)[:D - 3]
            ids[5] = ids[0]
            listed = g.score_docs(theta, metric, docs=ids)
            np.testing.assert_array_equal(listed, full[:, ids])
            _check(listed, theta, p[ids], metric, Lmax, K)
            # docs=None and the same documents listed
            np.testing.assert_array_equal(g.score_docs(theta, metric, docs=np.arange(D)), full)


def test_score_docs_chunks_queries_and_documents():
    """More than 1024 queries and more than 2^22 scores per query chunk: the
    call cuts both ways (two query chunks, the second ending in a partial
    tile; two document chunks copied into the caller's rows by pitch)."""
    from ldagibbssampling_amd.sampler import GibbsSampler
    K, D, Q = 20, 4200, 1030
    rng = np.random.default_rng(2)
    lens = rng.integers(0, 4, D)
    c = _corpus(lens, 50, 4)
    alpha = np.full(K, 0.5)
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, alpha, 0.01, seed=1) as g:
        g.sweep(1)
        _, _, nd, ndsum = g.counts(with_nd=True)
        p = _probabilities(nd.astype(np.float64), ndsum.astype(np.float64), alpha)
        theta = _thetas(K, Q, 8)
        got = g.score_docs(theta, "cosine")
        _check(got, theta, p, "cosine", int(lens.max()), K)
        ids = rng.permutation(D)
        np.testing.assert_array_equal(g.score_docs(theta, "cosine", docs=ids), got[:, ids])
        # a single small call gives the same bits as the chunked one
        np.testing.assert_array_equal(g.score_docs(theta[1025:1028], "cosine", docs=ids[:9]),
                                      got[1025:1028][:, ids[:9]])


def test_score_docs_repeats_and_leaves_state():
    g, c, alpha, p = _shard("k300_padded")
    theta = _thetas(g.K, 17, 1)
    z0 = g.z()
    counts0 = g.counts(with_nd=True)
    for metric in ("cosine", "mse"):
        a = g.score_docs(theta, metric)
        b = g.score_docs(theta, metric)
        assert a.tobytes() == b.tobytes()
    np.testing.assert_array_equal(g.z(), z0)
    for x, y in zip(g.counts(with_nd=True), counts0):
        np.testing.assert_array_equal(x, y)


def test_score_docs_errors():
    from ldagibbssampling_amd.sampler import GibbsSampler
    K = 20
    c = _corpus(_lengths(1, n=12), 60, 2)
    D = c.num_docs
    theta = _thetas(K, 3, 0)
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, 0.5), 0.01, seed=3) as g:
        g.sweep(1)
        ok = g.score_docs(theta)
        with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*metric") as e:
            g.score_docs(theta, metric=7)
        assert e.value.status == -1
        with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*document id"):
            g.score_docs(theta, docs=[0, D])
        with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*range"):
            g.score_docs(theta, doc_begin=1, num_docs=D)
        bad = theta.copy()
        bad[1] = 0.0
        with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*sums to zero"):
            g.score_docs(bad)
        bad = theta.copy()
        bad[2, 4] = np.nan
        with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*non-finite"):
            g.score_docs(bad)
        bad = theta.copy()
        bad[0, 0] = -0.25
        with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*negative"):
            g.score_docs(bad)
        # Q = 0 and M = 0 succeed
        assert g.score_docs(np.zeros((0, K))).shape == (0, D)
        assert g.score_docs(theta, docs=[]).shape == (3, 0)
        assert g.score_docs(theta, doc_begin=D, num_docs=0).shape == (3, 0)
        # a pending delta: sample() without apply()
        g.sample()
        with pytest.raises(capi.LdaError, match="LDA_ERR_STATE: .*pending") as e:
            g.score_docs(theta)
        assert e.value.status == -4
        g.apply()
        assert g.score_docs(theta).shape == ok.shape


# ------------------------------------------------------------- model level
def _model(corpus, K, devices=None, iters=6):
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


def _model_probabilities(m, D):
    return np.stack([m.getTopicProbabilities(d) for d in range(D)])


def test_score_instances_equals_infer_then_score():
    from ldagibbssampling_amd import topic_model as tm
    K = 20
    c = _corpus(_lengths(21), 120, 6)
    D = c.num_docs
    m = _model(c, K)
    rng = np.random.default_rng(4)
    held = [tm.Instance(rng.integers(0, 120, n).astype(np.int32)) for n in (30, 1, 80, 12)]
    # an out-of-vocabulary word id is dropped, as in ldatm_infer
    oov = tm.Instance(np.concatenate([held[0].data[:10], [120 + 5], held[0].data[10:]]).astype(np.int32))
    inf = m.getInferencer()
    scores, theta = inf.scoreInstances(held + [oov], 20, 4, 4, seed=5)
    ref_theta = inf.getSampledDistributions(held + [oov], 20, 4, 4, seed=5)
    assert theta.tobytes() == ref_theta.tobytes()
    clean_scores, clean_theta = inf.scoreInstances(held[:1], 20, 4, 4, seed=5)
    oov_scores, oov_theta = inf.scoreInstances([oov], 20, 4, 4, seed=5)
    assert oov_theta.tobytes() == clean_theta.tobytes() and oov_scores.tobytes() == clean_scores.tobytes()
    p = _model_probabilities(m, D)
    Lmax = int(np.diff(c.doc_off).max())
    assert scores.shape == (5, D)
    _check(scores, theta, p, "cosine", Lmax, K)
    mse, _ = inf.scoreInstances(held, 20, 4, 4, seed=5, docs=[3, 1, 3], metric="mse")
    _check(mse, theta[:4], p[[3, 1, 3]], "mse", Lmax, K)
    np.testing.assert_array_equal(m.scoreDistributions(theta), scores)
    m.close()


def test_scores_do_not_depend_on_the_shards():
    K = 20
    c = _corpus(_lengths(31, n=60), 150, 8)
    D = c.num_docs
    one = _model(c, K, devices=[0])
    three = _model(c, K, devices=[0, 0, 0])
    assert one.numShards() == 1 and three.numShards() == 3
    np.testing.assert_array_equal(one.topicAssignments(), three.topicAssignments())
    theta = _thetas(K, 5, 12)
    # a list that crosses the shard boundaries in non-monotone order, with a duplicate
    ids = np.random.default_rng(3).permutation(D)[:41]
    ids[7] = ids[2]
    for metric in ("cosine", "mse"):
        a = one.scoreDistributions(theta, metric=metric)
        b = three.scoreDistributions(theta, metric=metric)
        assert a.shape == (5, D) and a.tobytes() == b.tobytes()
        la = one.scoreDistributions(theta, docs=ids, metric=metric)
        lb = three.scoreDistributions(theta, docs=ids, metric=metric)
        assert la.tobytes() == lb.tobytes()
        np.testing.assert_array_equal(la, a[:, ids])
    with pytest.raises(capi.LdaError, match="LDA_ERR_INVALID_ARG: .*document id"):
        three.scoreDistributions(theta, docs=[0, D])
    ta, sa = one.topDocuments(theta, 7)
    tb, sb = three.topDocuments(theta, 7)
    np.testing.assert_array_equal(ta, tb)
    assert sa.tobytes() == sb.tobytes()
    one.close()
    three.close()


def test_top_documents_order_ties_and_padding():
    K = 20
    c = _corpus(_lengths(41, n=30, empties=3), 100, 9)
    D = c.num_docs
    assert int((np.diff(c.doc_off) == 0).sum()) == 3     # three equal scores per query
    m = _model(c, K, devices=[0, 0])
    theta = _thetas(K, 4, 2)
    empty = np.flatnonzero(np.diff(c.doc_off) == 0)
    # make the tie matter: a query equal to the empty documents' distribution
    # ranks all three first (cosine 1, mse 0)
    theta[3] = 1.0 / K
    for metric, sign in (("cosine", -1.0), ("mse", 1.0)):
        full = m.scoreDistributions(theta, metric=metric)
        ids, sc = m.topDocuments(theta, 5, metric=metric)
        assert ids.shape == (4, 5) and sc.shape == (4, 5)
        for q in range(4):
            order = np.lexsort((np.arange(D), sign * full[q]))    # score, then ascending id
            np.testing.assert_array_equal(ids[q], order[:5])
            np.testing.assert_array_equal(sc[q], full[q, order[:5]])
        np.testing.assert_array_equal(ids[3, :3], empty)
        assert sc[3, 0] == sc[3, 1] == sc[3, 2]
        # n > D pads with -1 / NaN
        ids, sc = m.topDocuments(theta, D + 3, metric=metric)
        for q in range(4):
            order = np.lexsort((np.arange(D), sign * full[q]))
            np.testing.assert_array_equal(ids[q, :D], order)
            np.testing.assert_array_equal(sc[q, :D], full[q, order])
        assert np.all(ids[:, D:] == -1) and np.all(np.isnan(sc[:, D:]))
    m.close()


def test_scores_survive_a_checkpoint(tmp_path):
    from ldagibbssampling_amd import topic_model as tm
    K = 20
    c = _corpus(_lengths(51), 90, 10)
    m = _model(c, K)
    theta = _thetas(K, 6, 3)
    before = {k: m.scoreDistributions(theta, metric=k) for k in ("cosine", "mse")}
    path = tmp_path / "model.bin"
    m.save(path)
    m.close()
    r = tm.ParallelTopicModel.load(path)
    for k, v in before.items():
        assert r.scoreDistributions(theta, metric=k).tobytes() == v.tobytes()
    r.close()
