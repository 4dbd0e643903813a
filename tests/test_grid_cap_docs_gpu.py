"""The one-wave-per-document kernels on the second and third trip of their
grid-stride loops ("Capped launchers").

Every kernel here is launched with at most B blocks of four waves, so one
pass covers P = 4 B documents (tokens for k_infer_init) and the wave that took
document j goes on to j + P, j + 2 P, ...  Each test runs n >= 2 P + 37 units
and asserts that before it calls the kernel, so some waves make three trips,
some two, and the last trip is ragged.  Where B is 8 x CUs the shapes follow
torch's multi_processor_count.

The training corpus holds triples (j, j + P, j + 2 P) = (a long document, an
empty one, a one-token one) for every stride in use and for the first wave,
a middle one and the last wave that can make three trips: whatever the long
document leaves in the wave's LDS histogram (a count, a retired -1 mark) shows
in the two documents behind it and cannot cancel.

References and bars are the ones of the modules that test each entry point
at small shapes (test_score_gpu, test_readout_gpu, test_diagnostics_gpu,
test_heldout_gpu, test_parity_gpu's 1e-9 and 1e-12); nothing is introduced
here.  At K = 2048 the numpy references that cost O(M K) per query or a sort
per document are evaluated on CHECKED documents only (the triples, both sides
of every pass boundary, the tail and 1,200 random ones); the kernel still
runs over all M.  Sums over documents (the diagnostics) are referenced in
full, block by block.
"""
import numpy as np
import pytest

import test_diagnostics_gpu as G
import test_heldout_gpu as H
import test_readout_gpu as R
import test_score_gpu as S
from ldagibbssampling_amd.corpus import document_completion_split

pytestmark = pytest.mark.gpu

V = 300
BETA = 0.01
LL_PASS = 4 * 1024            # k_ll_docs: lda_ctx::partial_blocks blocks
DOC_TOPICS_PASS = 4 * 4096    # launch_doc_topics
INFER_INIT_PASS = 4 * 8192    # launch_infer_init (tokens)
LTR_REDUCE_PASS = 4 * 8192    # launch_ltr_reduce
SCORE_CELLS = 1 << 22         # lda_score_docs: scores per chunk
READOUT_CELLS = 1 << 23       # lda_doc_counts / lda_doc_top_topics: int32 per chunk
HELDOUT_THETA_CELLS = 1 << 22
LONG, EMPTY, ONE = 1, 2, 3


def wave_pass():
    """Documents per pass of the kernels launched with 8 x CUs blocks."""
    import torch
    return 32 * torch.cuda.get_device_properties(0).multi_processor_count


def place_triples(D, strides):
    """{P: [j, ...]} with documents (j, j + P, j + 2 P) = (LONG, EMPTY, ONE)
    for every stride P and for wave 0, a middle wave and the last wave whose
    third trip exists (j = wave mod P; a wave's first free triple, found by
    backtracking, because the strides divide each other), and the roles."""
    want = []
    for P in sorted(set(strides), reverse=True):
        last = min(P - 1, D - 2 * P - 1)
        assert last >= 0, (D, P)
        for w in sorted({0, max(last // 2 - 1, 0), last}):
            want.append((P, w))
    role, chosen = {}, []

    def solve(i):
        if i == len(want):
            return True
        P, w = want[i]
        for j in range(w, D - 2 * P, P):
            new = {j: LONG, j + P: EMPTY, j + 2 * P: ONE}
            if all(role.get(d, r) == r for d, r in new.items()):
                added = [d for d in new if d not in role]
                role.update(new)
                chosen.append((P, j))
                if solve(i + 1):
                    return True
                chosen.pop()
                for d in added:
                    del role[d]
        return False

    assert solve(0), "no placement of the triples"
    triples = {}
    for P, j in chosen:
        triples.setdefault(P, []).append(j)
    return triples, role


class Layout:
    pass


_layout = None


def layout():
    """The training corpus (built once, never changed)."""
    global _layout
    if _layout is None:
        P = wave_pass()
        D = max(32805, 2 * P + 37)
        rng = np.random.default_rng(41)
        lens = rng.binomial(12, 1.0 / 3.0, D).astype(np.int64)       # 0..12, mean 4
        triples, role = place_triples(D, (LL_PASS, DOC_TOPICS_PASS, P))
        for d, r in role.items():
            lens[d] = {LONG: int(rng.integers(130, 701)), EMPTY: 0, ONE: 1}[r]
        lay = Layout()
        lay.c = S._corpus(lens, V, 43)
        lay.D, lay.P, lay.lens, lay.triples, lay.role = D, P, lens, triples, role
        lay.long = np.array(sorted(d for d, r in role.items() if r == LONG))
        # the documents the O(M K) references are evaluated at, at K = 2048
        near = [np.arange(max(b - 40, 0), min(b + 40, D)) for s in triples for b in (s, 2 * s)]
        lay.checked = np.unique(np.concatenate(
            [np.array(sorted(role)), np.arange(D - 80, D), np.arange(80), rng.choice(D, 1200, replace=False)] + near))
        lens.setflags(write=False)
        _layout = lay
    return _layout


def test_the_corpus_holds_the_triples():
    lay = layout()
    assert lay.D >= 2 * lay.P + 37 and lay.D >= 2 * DOC_TOPICS_PASS + 37 and lay.D >= 2 * LL_PASS + 37
    assert 100000 < lay.c.num_tokens < 170000 and lay.lens.max() <= 700
    rest = np.delete(lay.lens, sorted(lay.role))
    assert rest.min() == 0 and rest.max() <= 12 and 3.8 < rest.mean() < 4.2
    for P in {LL_PASS, DOC_TOPICS_PASS, lay.P}:
        last = min(P - 1, lay.D - 2 * P - 1)
        js = lay.triples[P]
        assert {j % P for j in js} >= {0, last}, (P, js)          # the grid's first wave and the last with three trips
        assert len(js) >= 3
        for j in js:
            assert 130 <= lay.lens[j] <= 700 and lay.lens[j + P] == 0 and lay.lens[j + 2 * P] == 1, (P, j)
    print({P: js for P, js in lay.triples.items()})


_shards = {}


def shard(K, kind):
    """One sampler per (K, sampler) over the corpus after 2 sweeps, with its
    alpha and z (fetched once, shared, never changed)."""
    if (K, kind) not in _shards:
        from ldagibbssampling_amd.sampler import GibbsSampler
        lay = layout()
        alpha = R.ALPHAS["asymmetric"](K)
        g = GibbsSampler(K, V, lay.c.doc_off, lay.c.words, alpha, BETA, seed=9, sampler=kind)
        g.sweep(2)
        z = g.z()
        z.setflags(write=False)
        _shards[(K, kind)] = (g, alpha, z)
    return _shards[(K, kind)]


_rows_cache = {}


def nd_rows(K, kind, ids=None):
    """numpy's topic counts (test_diagnostics_gpu.doc_counts) of the listed
    documents (None: all) under the shard's z."""
    key = (K, kind, None if ids is None else ids.tobytes())
    if key not in _rows_cache:
        lay = layout()
        z = shard(K, kind)[2]
        off = lay.c.doc_off
        if ids is None:
            nd = G.doc_counts(off, z, K)
        else:
            sub = np.zeros(len(ids) + 1, np.int64)
            np.cumsum(lay.lens[ids], out=sub[1:])
            tok = np.concatenate([np.arange(off[d], off[d + 1]) for d in ids]) if len(ids) else np.zeros(0, np.int64)
            nd = G.doc_counts(sub, z[tok], K)
        nd.setflags(write=False)
        _rows_cache[key] = nd
    return _rows_cache[key]


def checked(K):
    """(ids, all) of the documents a per-document reference is evaluated at."""
    lay = layout()
    return (None, np.arange(lay.D)) if K <= 300 else (lay.checked, lay.checked)


CONFIGS = [(20, "dense"), (2048, "sparse")]


# ------------------------------------------------------------ k_doc_scores
@pytest.mark.parametrize("Q", [3, 21])
@pytest.mark.parametrize("K,kind", CONFIGS)
def test_score_docs_past_two_passes(K, kind, Q):
    """Q = 3: the 4-wide tile; Q = 21: the 16-wide tile and a rest of 5."""
    lay = layout()
    g, alpha, z = shard(K, kind)
    M, P = lay.D, wave_pass()
    assert M > 2 * P and M >= 2 * P + 37
    assert Q * M <= SCORE_CELLS                  # one chunk holds all M documents
    key, ids = checked(K)
    nd = nd_rows(K, kind, key).astype(np.float64)
    p = S._probabilities(nd, lay.lens[ids].astype(np.float64), alpha)
    theta = S._thetas(K, Q, 100 + Q)
    Lmax = int(lay.lens.max())
    for metric in ("cosine", "mse"):
        got = g.score_docs(theta, metric)
        assert got.shape == (Q, M)
        step = 1 << 22 if K <= 300 else 400      # numpy's mse holds Q x step x K doubles at once
        for a in range(0, len(ids), step):
            S._check(got[:, ids[a:a + step]], theta, p[a:a + step], metric, Lmax, K)


# ------------------------------------------------------------ k_doc_counts
@pytest.mark.parametrize("K", [20, 300])
def test_doc_counts_past_two_passes(K):
    lay = layout()
    g, alpha, z = shard(K, "dense")
    P = wave_pass()
    chunk = min(lay.D, READOUT_CELLS // K)
    assert chunk > 2 * P and chunk >= 2 * P + 37   # the first chunk alone makes three trips
    nd = nd_rows(K, "dense")
    assert (nd[lay.long] > 0).sum(1).min() > min(K, 100) // 2     # the long documents touch most topics
    np.testing.assert_array_equal(g.doc_counts(), nd)


# -------------------------------------------------------- k_doc_top_topics
@pytest.mark.parametrize("K,kind,m", [(20, "dense", 3), (300, "dense", 3), (2048, "sparse", 3), (20, "dense", 25)])
def test_doc_top_topics_past_two_passes(K, kind, m):
    lay = layout()
    g, alpha, z = shard(K, kind)
    M, P = lay.D, wave_pass()
    assert min(M, READOUT_CELLS // (2 * m)) == M and M > 2 * P and M >= 2 * P + 37     # one chunk, three trips
    key, ids = checked(K)
    nd = nd_rows(K, kind, key)
    topics, cnt = g.doc_top_topics(m)
    assert topics.shape == (M, m)
    et, ec = R.expected_top_topics(nd, lay.lens[ids], alpha, R._seq_sum(alpha), m)
    np.testing.assert_array_equal(topics[ids], et)
    np.testing.assert_array_equal(cnt[ids], ec)
    if m > K:      # every topic retired in every document: the marks must be wiped for the next one
        assert np.all(topics[:, K:] == -1) and np.all(cnt[:, K:] == 0) and np.all(topics[:, :K] >= 0)


# ----------------------------------------------------- k_doc_diag, k_codoc
@pytest.mark.parametrize("K,kind,n,props", [(20, "dense", 7, G.MALLET_PROPS), (2048, "sparse", 2, (0.02, 0.1, 0.5))])
def test_topic_codocuments_past_two_passes(K, kind, n, props):
    lay = layout()
    g, alpha, z = shard(K, kind)
    D, P = lay.D, wave_pass()
    assert D > 2 * P and D >= 2 * P + 37
    # launch_doc_diag's rule: the block counters sit in LDS when they fit behind the histograms
    in_lds = 4 * g.Kp * 4 + K * (2 + len(props)) * 4 <= 64 * 1024
    assert in_lds == (K == 20)
    off, words = lay.c.doc_off, lay.c.words
    ids = g.top_words(n)[0]
    pres = G.presence(off, words, z, ids, V)
    want = np.concatenate([G.expected_codoc(pres[k:k + 128]) for k in range(0, K, 128)])
    stats_want = np.zeros((K, 2 + len(props)), np.int64)
    for a in range(0, D, 4096):                      # every statistic is a sum over documents
        b = min(a + 4096, D)
        stats_want += G.expected_doc_stats(G.doc_counts(off[a:b + 1], z[off[a]:off[b]], K), alpha, props)
    codoc, stats = g.topic_codocuments(ids, props)
    np.testing.assert_array_equal(stats, stats_want)
    np.testing.assert_array_equal(codoc, want)


# --------------------------------------------------------------- k_ll_docs
@pytest.mark.parametrize("K,kind", CONFIGS)
def test_log_likelihood_parts_past_two_passes(K, kind, oracle):
    lay = layout()
    g, alpha, z = shard(K, kind)
    assert lay.D > 2 * LL_PASS and lay.D >= 2 * LL_PASS + 37
    o = oracle.ExactSampler(K, V, lay.c.doc_off, lay.c.words, alpha, BETA, 9, z_init=z, kind=kind)
    o.apply()
    np.testing.assert_array_equal(o.z(), z)
    got, ref = g.log_likelihood_parts(), o.log_likelihood_parts()
    for a, b in zip(got, ref):
        print(f"K={K}: part {a!r} oracle {b!r} rel {abs(a - b) / abs(b):.3e}")
        assert abs(a - b) <= 1e-9 * abs(b), (a, b)


# ------------------------------------------------------------ k_doc_topics
@pytest.mark.parametrize("K", [20, 300])
def test_counts_with_nd_past_two_passes(K):
    lay = layout()
    g, alpha, z = shard(K, "dense")
    assert lay.D > 2 * DOC_TOPICS_PASS and lay.D >= 2 * DOC_TOPICS_PASS + 37
    _, _, nd, ndsum = g.counts(with_nd=True)
    np.testing.assert_array_equal(nd, nd_rows(K, "dense"))
    np.testing.assert_array_equal(ndsum, lay.lens)


# -------------------------------------------------------- k_doc_completion
_held_models = {}


def _held_model(K):
    if K not in _held_models:
        from ldagibbssampling_amd.sampler import GibbsSampler
        c = H._train_corpus(200)
        g = GibbsSampler(K, c.num_types, c.doc_off, c.words, 0.05 + 0.4 * np.arange(K) / K, H.BETA, seed=9)
        g.sweep(2)
        nw, nwsum, _, _ = g.counts()
        _held_models[K] = (g, nw.astype(np.float64), nwsum.astype(np.float64))
    return _held_models[K]


@pytest.mark.parametrize("K", [100, 256])
def test_heldout_loglik_past_two_passes(K):
    """K = 100: one chunk with a ragged third trip; K = 256: chunks of 2^22 /
    256 = 16,384 documents, two full trips on 256 CUs, then a second chunk."""
    g, nw, nwsum = _held_model(K)
    P = wave_pass()
    Dh = 2 * P + 37
    chunk = min(Dh, HELDOUT_THETA_CELLS // K)
    if K == 100:
        assert chunk == Dh and Dh > 2 * P
    else:
        assert 2 * P <= chunk < Dh
    rng = np.random.default_rng(K)
    lens = rng.integers(0, 6, Dh)
    lens[[0, P, 2 * P]] = (5, 0, 1)
    off = np.zeros(Dh + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = rng.integers(0, g.V, int(off[-1])).astype(np.int32)
    theta = H._thetas(K, Dh, 23)
    doc_ll, total = g.heldout_loglik(theta, off, words)
    ref = H._reference(nw, nwsum, g.V, H.BETA, theta, off, words)
    bars = H._bars(ref, lens, K)
    err = np.abs(doc_ll - ref)
    print(f"K={K}: max |delta_d| / bar {np.max(err[lens > 0] / bars[lens > 0]):.3e}")
    assert np.all(err <= bars)
    assert np.all(doc_ll[lens == 0] == 0.0) and np.all(doc_ll[lens > 0] < 0.0)
    assert total == H._ordered_sum(doc_ll)


# ------------------------------- k_infer_init, the accumulating k_doc_topics
_held = None


def held_out():
    """32,805 held-out documents of 0..12 tokens (mean 6): both the observed
    halves and the whole hold more than 2 x 32,768 + 37 tokens."""
    global _held
    if _held is None:
        rng = np.random.default_rng(77)
        lens = rng.binomial(12, 0.5, 2 * DOC_TOPICS_PASS + 37).astype(np.int64)
        lens[[0, DOC_TOPICS_PASS, 2 * DOC_TOPICS_PASS]] = (12, 0, 1)
        c = S._corpus(lens, V, 78)
        _held = (c,) + document_completion_split(c)
    return _held


INFER = dict(n_iter=4, burn_in=1, thin=1, seed=8)      # three accumulating k_doc_topics launches


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_infer_past_two_passes(kind, oracle):
    lay = layout()
    g, alpha, z = shard(20, kind)
    held = held_out()[0]
    assert held.num_docs >= 2 * DOC_TOPICS_PASS + 37 and held.num_tokens >= 2 * INFER_INIT_PASS + 37
    nw = g.counts()[0]
    assert np.all(nw.sum(1) > 0)                 # no token is dropped: the kernels see every one
    o = oracle.ExactSampler(20, V, lay.c.doc_off, lay.c.words, alpha, BETA, 9, z_init=z, kind=kind)
    o.apply()
    np.testing.assert_array_equal(o.counts()[0], nw)
    tg = g.infer(held.doc_off, held.words, **INFER)
    to = o.infer(held.doc_off, held.words, **INFER)
    np.testing.assert_allclose(tg, to, rtol=0, atol=1e-12)
    np.testing.assert_allclose(tg.sum(1), 1.0, atol=1e-12)


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_doc_completion_is_infer_then_heldout_loglik_past_two_passes(kind):
    g, alpha, z = shard(20, kind)
    held, obs, sc = held_out()
    Dh, P = held.num_docs, wave_pass()
    assert Dh >= 2 * DOC_TOPICS_PASS + 37 and obs.num_tokens >= 2 * INFER_INIT_PASS + 37
    assert min(Dh, HELDOUT_THETA_CELLS // 20) == Dh and Dh >= 2 * P + 37       # k_doc_completion: one chunk, three trips
    doc_ll, total, theta = g.doc_completion(obs.doc_off, obs.words, sc.doc_off, sc.words, return_theta=True, **INFER)
    ref_theta = g.infer(obs.doc_off, obs.words, **INFER)
    assert theta.tobytes() == ref_theta.tobytes()
    given, given_total = g.heldout_loglik(ref_theta, sc.doc_off, sc.words)
    assert given.tobytes() == doc_ll.tobytes() and given_total == total
    assert total == H._ordered_sum(doc_ll)


# ------------------------------------------- k_ltr_reduce, k_left_to_right
LTR_JOBS_PASS = 4 << 20       # launch_left_to_right: 2^20 blocks of four (document, particle) jobs
LTR_CELLS = 1 << 22           # lda_left_to_right: (particle, token) cells per chunk
LTR_DOCS = 1 << 20            # ... and documents per chunk


def _same_as_one_pass_calls(g, off, words, args, segments, one_pass_docs):
    """The documents [a, b) of each segment give the same bytes in a call that
    stays within one pass.  A draw is keyed by the token's index in the call,
    so those calls carry the earlier tokens in front, in documents of 4,096
    tokens (the longest lda_left_to_right takes)."""
    ll, total, tokens, tp = g.left_to_right(off, words, **args)
    lens = np.diff(off)
    assert tokens == off[-1] and total == H._ordered_sum(ll)
    assert np.all(ll[lens == 0] == 0.0) and np.all(ll[lens > 0] < 0.0) and np.all(tp > 0.0)
    assert segments[0][0] > 0 and segments[-1][1] == len(lens)
    for a, b in segments:
        front = np.arange(0, off[a], 4096, dtype=np.int64)
        sub_off = np.concatenate([front, off[a:b + 1]])
        assert len(sub_off) - 1 <= one_pass_docs
        sll, _, _, stp = g.left_to_right(sub_off, words[:off[b]], **args)
        assert sll[len(front):].tobytes() == ll[a:b].tobytes()
        assert stp[off[a]:].tobytes() == tp[off[a]:off[b]].tobytes()


def test_left_to_right_reduce_past_two_passes():
    """k_ltr_reduce's second and third trip against its first."""
    g, alpha, z = shard(20, "dense")
    P = LTR_REDUCE_PASS
    Dh = 2 * P + 37
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 3, Dh)
    lens[[P, 2 * P]] = (0, 2)
    off = np.zeros(Dh + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    assert Dh > 2 * P and 2 * int(off[-1]) <= LTR_CELLS and Dh <= LTR_DOCS      # one chunk
    args = dict(particles=2, resampling=False, seed=19, token_prob=True)
    _same_as_one_pass_calls(g, off, words, args, ((P, 2 * P - 64), (2 * P - 64, Dh)), P)


def test_left_to_right_jobs_past_two_passes():
    """k_left_to_right's job loop: 2^20 documents (one chunk) x 9 particles
    are more than two passes of 2^22 jobs; nine in ten documents are empty,
    so the tokens fit the chunk's cells."""
    g, alpha, z = shard(20, "dense")
    R, Dh = 9, LTR_DOCS
    rng = np.random.default_rng(6)
    lens = np.where(rng.random(Dh) < 0.1, rng.integers(1, 4, Dh), 0)
    off = np.zeros(Dh + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    assert Dh * R >= 2 * LTR_JOBS_PASS + 37 and R * int(off[-1]) <= LTR_CELLS and Dh <= LTR_DOCS
    one_pass = LTR_JOBS_PASS // R
    cut = one_pass - 64                                  # room for the documents in front
    args = dict(particles=R, resampling=False, seed=23, token_prob=True)
    _same_as_one_pass_calls(g, off, words, args, ((cut, 2 * cut), (2 * cut, Dh)), one_pass)
