"""One long-lived context driven the way a training run drives it: sweeps on
every path (one by one, graph-launched, split, sampled and applied by hand,
recounted), alpha and beta replaced along the way, z replaced, the stream
changed -- and between the state changes every read-only entry point of
GibbsSampler (lifecycle_probes.probe), the sized ones three times in a row at
a small size, their largest and another small one, in an order that changes
from checkpoint to checkpoint.

What is asserted, per sampler family (quarter-wave K = 20, dense K = 512,
sparse K = 300, large-K sparse K = 2048):

  A  the chain is untouched: after every state change and its probes z, nw,
     nwsum, nd, the sweep counter and the counts' checksum equal cpu_exact's,
     which saw the state changes and none of the probes;
  B  history does not matter: a context made afresh from (z, alpha, beta, the
     seed, the work ranges) gives, for every probe at its last size and in the
     reverse order, the same bytes as the long-lived context's last call.
     These calls are documented as bit-repeatable, so equality is the bar;
     no probe here is order-dependent by design (the escape-list order of
     lda_exchange_pack is, and is not a probe);
  C  after alpha and beta moved (and after z was replaced) the results equal
     the plain restatements evaluated at the current alpha and beta, each at
     the bar of the module it comes from (lifecycle_probes
     .check_against_references).

The counts of the first checkpoints hold another shard's tokens as well: the
creation's pending buffer receives them before the first apply, as an
all-reduce leaves them, and they give the held-out documents' rare word a
nonzero row.  lda_set_z re-seeds from the shard alone, so that row empties
again -- the one way a context's word totals change, which lda_infer's cached
totals have to follow.

Calls the API refuses, which are therefore not made: nearest_topics with more
than LDA_TOPIC_NEAREST_MAX = 64 topics (the largest call is min(K - 1, 64));
doc_top_topics' largest m is min(K, 16); set_count_update("recount") on the
sparse samplers (step 9 is dense only); probes between sample() and apply()
(all but word_cooccurrences and z answer LDA_ERR_STATE: that is
test_error_paths_leave_the_scratch_usable).

C compares the topic distances on sixteen rows of the matrix above K = 64
(lifecycle_probes.distance_rows) and the co-occurrence counts with one
restatement per word list, which no state change can alter; B compares every
cell of both at every checkpoint.

Then, smaller: two contexts alive at once, cross-model distances queued right
behind graph sweeps, the log-likelihood ticket ring, and the error paths.

On an MI355X the slowest case, sparse K = 2048 (14 checkpoints, 574 probe
calls on the long-lived context, 14 fresh contexts, 4 rounds of numpy
restatements), takes 5.6 s; the others 0.5 to 2.4 s.
"""
import ctypes as C

import numpy as np
import pytest

import lifecycle_probes as P
import test_topic_distances_gpu as TDG
import topic_distance_numpy as TD
from ldagibbssampling_amd import capi

pytestmark = pytest.mark.gpu

CASES = [("dense", 20), ("dense", 512), ("sparse", 300), ("sparse", 2048)]


def _alpha0(K):
    return np.full(K, 0.1)


def _foreign(K, Kp):
    """Another shard's counts as (cells of the exchange buffer, values): three
    tokens of the rare word under topic 1 and two under K - 1, four of the most
    frequent word under topic 0, with their nwsum cells."""
    u = P.unseen_word()
    common = int(np.bincount(P.train_corpus().words, minlength=P.V).argmax())
    cells, vals = [], []
    for w, k, n in ((u, 1, 3), (u, K - 1, 2), (common, 0, 4)):
        cells += [w * Kp + k, P.V * Kp + k]
        vals += [n, n]
    return np.array(cells, np.int64), np.array(vals, np.int32)


def _inject(g, foreign):
    """Add the foreign counts to g's pending exchange buffer (between the
    context's stream and torch's, both waited for)."""
    import torch
    g.synchronize()
    t = g.delta_tensor()
    cells, vals = foreign
    assert cells.max() < t.numel()
    t.index_add_(0, torch.as_tensor(cells, device=t.device), torch.as_tensor(vals, device=t.device))
    torch.cuda.synchronize()


def _make(kind, K, alpha, beta, z_init=None, foreign=None):
    from ldagibbssampling_amd.sampler import GibbsSampler
    c = P.train_corpus()
    g = GibbsSampler(K, P.V, c.doc_off, c.words, alpha, beta, seed=P.SEED, z_init=z_init,
                     tokens_per_range=P.TOKENS_PER_RANGE, sampler=kind)
    if foreign is not None:
        _inject(g, foreign)
    return g


def _oracle(oracle, kind, K, alpha, beta, z_init=None, foreign=None):
    c = P.train_corpus()
    o = oracle.ExactSampler(K, P.V, c.doc_off, c.words, alpha, beta, P.SEED, z_init=z_init, kind=kind)
    if foreign is not None:
        np.add.at(o.delta(), foreign[0], foreign[1])
    return o


def _fresh(g, kind, foreign):
    """A context made afresh from g's state, applied, at g's sweep counter."""
    f = _make(kind, g.K, g.alpha, g.beta, z_init=g.z(), foreign=foreign)
    f.sweep(0)
    f.sweep_index = g.sweep_index
    return f


def _chain_equal(g, o, oracle, what):
    """Assertion A."""
    np.testing.assert_array_equal(g.z(), o.z(), err_msg=what)
    for a, b in zip(g.counts(with_nd=True), o.counts(with_nd=True)):
        np.testing.assert_array_equal(a, b, err_msg=what)
    assert g.sweep_index == o.sweep_index, what
    onw, onwsum = o.counts()[:2]
    assert g.counts_checksum() == oracle.counts_checksum(onw, onwsum), what


class _Life:
    """The long-lived context g, its mirror o and the bookkeeping of one case."""

    def __init__(self, oracle, kind, K):
        self.oracle, self.kind, self.K = oracle, kind, K
        self.alpha, self.beta = _alpha0(K), P.BETA0
        self.g = _make(kind, K, self.alpha, self.beta)
        self.foreign = _foreign(K, self.g.Kp)
        _inject(self.g, self.foreign)
        self.o = _oracle(oracle, kind, K, self.alpha, self.beta, foreign=self.foreign)
        self.env = dict(cp=-1, what=f"{kind} K={K}", label="", max_count=P.train_corpus().num_tokens + 16)
        self.ran = set()            # (checkpoint, probe, size index)
        self.adjacent = set()       # (probe, the probe right after it), across the case
        self.labels = []

    def both(self, call, *a):
        getattr(self.g, call)(*a)
        getattr(self.o, call)(*a)

    def set_alpha_beta(self, alpha, beta):
        self.alpha, self.beta = alpha, beta
        self.both("set_alpha_beta", alpha, beta)

    def checkpoint(self, label, refs=False):
        """Every probe on g, then A, B and (refs) C."""
        env, g = self.env, self.g
        env["cp"] += 1
        env["label"] = label
        cp = env["cp"]
        self.labels.append(label)
        what = f"{env['what']} checkpoint {cp} ({label})"
        base = P.ORDER_A if cp % 2 == 0 else P.ORDER_B
        shift = (3 * (cp // 2)) % len(base)
        order = base[shift:] + base[:shift]
        results, last = {}, {}
        for prev, name in zip((None,) + order, order):
            if prev is not None:
                self.adjacent.add((prev, name))
            for i in (range(3) if name in P.SIZED else (0,)):
                results[name, i] = P.probe(g, env, name, i)
                self.ran.add((cp, name, i))
            last[name] = P.as_bytes(results[name, 2 if name in P.SIZED else 0])
        _chain_equal(g, self.o, self.oracle, what + ": the chain after the probes")
        f = _fresh(g, self.kind, self.foreign)
        try:
            for name in dict.fromkeys(reversed(order)):
                assert P.as_bytes(P.probe(f, env, name, 2)) == last[name], \
                    f"{what}: {name} depends on the context's history"
        finally:
            f.close()
        if refs:
            P.check_against_references(g, self.o, env, results)
        _chain_equal(g, self.o, self.oracle, what + ": the chain at the end of the checkpoint")

    def coverage(self):
        """(missing, summary): every (probe, size) at every checkpoint, every
        shared-scratch adjacency in the case."""
        cps = len(self.labels)
        want = {(cp, n, i) for cp in range(cps) for n in P.SIZED for i in range(3)}
        want |= {(cp, n, 0) for cp in range(cps) for n in P.UNSIZED}
        missing = sorted(want - self.ran) + sorted(set(P.CHAINS) - self.adjacent)
        summary = (f"{self.env['what']}: {cps} checkpoints {self.labels}; {len(self.ran)} probe calls of "
                   f"{len(want)}; {len(self.adjacent)} different adjacencies, chains "
                   f"{sorted(set(P.CHAINS) & self.adjacent)}; missing {missing}")
        return missing, summary


@pytest.mark.parametrize("kind,K", CASES)
def test_lifecycle(oracle, kind, K):
    import torch
    L = _Life(oracle, kind, K)
    g, o = L.g, L.o
    rng = np.random.default_rng(1000 + K)
    try:
        assert g.Kp == capi.padded_topics(K)
        # 1. the first apply (the creation's counts and the other shard's), one sweep
        L.both("sweep", 0)
        L.checkpoint("1: sweep(0)")
        L.both("sweep", 1)
        L.checkpoint("1: sweep(1)")
        # 2. three sweeps in one call (dense: one graph), the probes right behind them
        L.both("sweep", 3)
        L.checkpoint("2: sweep(3)")
        # 3. a sweep by hand
        L.both("sample")
        L.both("apply")
        L.checkpoint("3: sample, apply")
        # 4. the optimiser's alpha and beta with nothing pending
        L.set_alpha_beta(rng.gamma(0.5, 0.4, K) + 0.01, P.BETA0 * 3)
        L.checkpoint("4: set_alpha_beta", refs=True)
        L.both("sweep", 2)
        L.checkpoint("4: sweep(2)", refs=True)
        # 5. ... and between sample and apply
        L.both("sample")
        L.set_alpha_beta(rng.gamma(0.5, 0.4, K) + 0.01, P.BETA0 * 3 / 5)
        L.both("apply")
        L.checkpoint("5: sample, set_alpha_beta, apply")
        L.both("sweep", 1)
        L.checkpoint("5: sweep(1)", refs=True)
        # 6. a split sweep, part by part (cpu_exact: the same sweep, unsplit)
        g.set_exchange_parts(3)
        for part in range(3):
            g.sample_part(part)
        g.apply()
        o.sample()
        o.apply()
        L.checkpoint("6: three parts, apply")
        g.set_exchange_parts(1)
        L.both("sweep", 1)
        L.checkpoint("6: one part, sweep(1)")
        # 7. z replaced: the current topics shuffled within each document; the
        # other shard's counts are gone with the re-seeding
        z = g.z()
        off = P.train_corpus().doc_off
        for d in range(g.D):
            z[off[d]:off[d + 1]] = rng.permutation(z[off[d]:off[d + 1]])
        g.set_z(z)
        L.foreign = None
        sweep_index = o.sweep_index
        L.o = o = _oracle(oracle, kind, K, L.alpha, L.beta, z_init=z)
        o.sweep_index = sweep_index
        L.both("sweep", 0)
        L.checkpoint("7: set_z, sweep(0)")
        L.both("sweep", 2)
        L.checkpoint("7: sweep(2)", refs=True)
        # 8. another stream
        stream = torch.cuda.Stream()
        g.set_stream(stream.cuda_stream)
        L.both("sweep", 2)
        L.checkpoint("8: set_stream, sweep(2)")
        g.set_stream(None)
        L.both("sweep", 1)
        L.checkpoint("8: own stream, sweep(1)")
        # 9. the recount and back (the dense samplers)
        if kind == "dense":
            g.set_count_update("recount")
            L.both("sweep", 2)
            L.checkpoint("9: recount, sweep(2)")
            g.set_count_update("delta")
            L.both("sweep", 1)
            L.checkpoint("9: delta, sweep(1)")
        missing, summary = L.coverage()
        print(summary)
        assert not missing, summary
    finally:
        L.g.close()


# ------------------------------------------------- two contexts alive at once
def _final_sizes(ctx, env):
    """Every probe at its largest and its last size."""
    out = {}
    for name in dict.fromkeys(P.ORDER_A):
        for i in ((1, 2) if name in P.SIZED else (0,)):
            out[name, i] = P.as_bytes(P.probe(ctx, env, name, i))
    return out


def test_two_contexts_alive_at_once():
    """A quarter-wave K = 20 and a large-K sparse K = 2048 context over the
    same V, their calls alternated, with the process-wide chunk sizes of
    lda_left_to_right and lda_word_cooccurrences made small meanwhile: each
    gives what it gives alone."""
    env = dict(cp=0, max_count=P.train_corpus().num_tokens + 16)
    shapes = [("dense", 20), ("sparse", 2048)]
    alone = []
    for kind, K in shapes:
        with _make(kind, K, _alpha0(K), P.BETA0) as g:
            g.sweep(2)
            alone.append(_final_sizes(g, env))
    lib = capi.load()
    a, b = (_make(kind, K, _alpha0(K), P.BETA0) for kind, K in shapes)
    try:
        lib.lda_debug_ltr_chunk_cells(8)
        lib.lda_debug_cooc_chunk_tokens(16)
        for _ in range(2):
            a.sweep(1)
            b.sweep(1)
        for name in dict.fromkeys(P.ORDER_A):
            for i in ((1, 2) if name in P.SIZED else (0,)):
                got = [P.as_bytes(P.probe(ctx, env, name, i)) for ctx in (a, b)]
                for j in range(2):
                    assert got[j] == alone[j][name, i], (shapes[j], name, i)
    finally:
        lib.lda_debug_ltr_chunk_cells(0)
        lib.lda_debug_cooc_chunk_tokens(0)
        a.close()
        b.close()


# --------------------- cross-model distances queued right behind graph sweeps
def test_cross_model_distances_right_after_the_other_models_sweeps():
    """a.topic_distances(other=b) and a.nearest_topics(other=b) issued right
    after b.sweep(3) (a graph launch on b's stream, no synchronize) equal the
    same calls after b.synchronize(), byte for byte, and numpy on
    b.counts()."""
    a = _make("dense", 20, _alpha0(20), P.BETA0)
    b = _make("dense", 64, _alpha0(64), 0.05)
    try:
        a.sweep(2)
        b.sweep(1)
        for x, y in ((a, b), (b, a)):
            for metric in P.METRICS:
                y.sweep(3)
                early = x.topic_distances(metric, other=y)
                y.synchronize()
                assert x.topic_distances(metric, other=y).tobytes() == early.tobytes(), metric
                want = TDG._restate(x, y, metric)
                TDG._close(early, want, metric, f"K={x.K} against K={y.K} right after sweep(3)")
                y.sweep(3)
                topics, values = x.nearest_topics(5, metric, other=y)
                y.synchronize()
                later = x.nearest_topics(5, metric, other=y)
                assert later[0].tobytes() == topics.tobytes() and later[1].tobytes() == values.tobytes(), metric
                et, ev = TD.expected_nearest(x.topic_distances(metric, other=y), 5, metric, False)
                np.testing.assert_array_equal(topics, et)
                assert values.tobytes() == ev.tobytes()
    finally:
        a.close()
        b.close()


# ------------------------------------------------------- the LL ticket ring
@pytest.mark.parametrize("kind,K", [("dense", 20), ("sparse", 300)])
def test_log_likelihood_ticket_ring(kind, K):
    """Twenty tickets over twenty sweeps, none collected, the blocking
    lda_log_likelihood_parts recorded beside each: the newest 16 collect to
    exactly those values, the 4 overwritten ones answer LDA_ERR_STATE, and so
    does any ticket collected twice."""
    lib = capi.load()
    collect = lambda t, a, b: lib.lda_log_likelihood_collect(g._h, t, C.byref(a), C.byref(b))   # noqa: E731
    with _make(kind, K, _alpha0(K), P.BETA0) as g:
        tickets, blocking = [], []
        for _ in range(20):
            g.sweep(1)
            t = C.c_int64()
            capi.check(lib.lda_log_likelihood_enqueue(g._h, C.byref(t)), "lda_log_likelihood_enqueue")
            tickets.append(t.value)
            blocking.append(g.log_likelihood_parts())
        assert len(set(tickets)) == 20 and len(set(blocking)) == 20
        a, b = C.c_double(), C.c_double()
        for t in tickets[:4]:
            assert collect(t, a, b) == -4, f"overwritten ticket {t}"
            assert b"ticket" in lib.lda_last_error()
        for t, want in zip(tickets[4:], blocking[4:]):
            assert collect(t, a, b) == 0, (t, lib.lda_last_error())
            assert (a.value, b.value) == want, t
        for t in tickets:
            assert collect(t, a, b) == -4, f"ticket {t} collected twice"
        # the ring goes on
        g.sweep(1)
        t = C.c_int64()
        capi.check(lib.lda_log_likelihood_enqueue(g._h, C.byref(t)), "lda_log_likelihood_enqueue")
        want = g.log_likelihood_parts()
        assert collect(t.value, a, b) == 0 and (a.value, b.value) == want


# ------------------------------------------------------------ the error paths
def _refusals(g):
    """(probe, [a call that fails its argument check, its status]) per family."""
    K, D, lib = g.K, g.D, g._L
    off, words = P.held_subset(1)
    bad_words = words.copy()
    bad_words[4] = P.V
    theta = P.held_thetas(K, 1)
    neg = theta.copy()
    neg[2, 1] = -0.5
    twice = P.word_lists(K, 1).copy()
    twice[1, :2] = 7
    big = P.word_lists(K, 1).copy()
    big[0, 0] = P.V
    i32 = lambda *s: np.zeros(s, np.int32)      # noqa: E731
    f64 = lambda *s: np.zeros(s, np.float64)    # noqa: E731
    p = lambda a: a.ctypes.data                 # noqa: E731
    raw = lambda status: capi.check(status, "raw call")     # noqa: E731
    return [
        ("infer", -1, lambda: g.infer(off, bad_words, **P.INFER)),
        ("score_docs", -1, lambda: g.score_docs(P.score_thetas(K, 1), "cosine", docs=[0, D])),
        ("top_words", -1, lambda: raw(lib.lda_top_words(g._h, capi.TOP_WORDS_MAX + 1, p(i32(K, 65)), p(i32(K, 65))))),
        ("doc_top_topics", -1, lambda: g.doc_top_topics(3, docs=[2, -1])),
        ("doc_counts", -1, lambda: g.doc_counts(doc_begin=D, num_docs=1)),
        ("codocuments", -1, lambda: g.topic_codocuments(twice, P.PROPS[1])),
        ("codocuments", -1, lambda: g.topic_codocuments(P.word_lists(K, 1), (0.5, 0.1))),
        ("word_stats", -1, lambda: g.topic_word_stats(big)),
        ("cooccurrences", -1, lambda: g.word_cooccurrences(P.word_lists(K, 1), 3, off, bad_words)),
        ("topic_distances", -1, lambda: raw(lib.lda_topic_distances(g._h, None, 7, p(f64(K, K))))),
        ("nearest_topics", -1, lambda: raw(lib.lda_topic_nearest(g._h, None, 2, capi.TOPIC_NEAREST_MAX + 1,
                                                                 p(i32(K, 65)), p(f64(K, 65))))),
        ("heldout", -1, lambda: g.heldout_loglik(neg, off, words)),
        ("doc_completion", -1, lambda: g.doc_completion(off, words, off, bad_words, **P.COMPLETION)),
        ("left_to_right", -1, lambda: g.left_to_right(off, bad_words, 2)),
        ("left_to_right", -5, lambda: g.left_to_right(off, words, capi.LTR_MAX_PARTICLES + 1)),
        ("ll", -4, lambda: raw(lib.lda_log_likelihood_collect(g._h, 999, None, None))),
        ("histograms", -1, lambda: g.doc_topic_histograms(max_len=g.max_doc_length() - 1)),
        ("histograms", -1, lambda: g.count_histogram(0)),
    ]


@pytest.mark.parametrize("kind,K", [("dense", 20), ("sparse", 2048)])
def test_error_paths_leave_the_scratch_usable(kind, K):
    """Per probe family a call that fails its argument check, then the valid
    call: it gives what a context made afresh gives.  Then every family
    between sample() and apply() (LDA_ERR_STATE, but for z, the counts and
    lda_word_cooccurrences, which read no pending state), and after apply()
    the same comparison again."""
    env = dict(cp=0, max_count=P.train_corpus().num_tokens + 16)
    g = _make(kind, K, _alpha0(K), P.BETA0)
    try:
        g.sweep(2)
        f = _fresh(g, kind, None)
        want = {name: P.as_bytes(P.probe(f, env, name, 2)) for name in dict.fromkeys(P.ORDER_A)}
        f.close()
        seen = set()
        for name, status, call in _refusals(g):
            P.probe(g, env, name, 1)                  # the largest call's leftovers lie under the refusal
            with pytest.raises(capi.LdaError) as e:
                call()
            assert e.value.status == status, (name, str(e.value))
            assert P.as_bytes(P.probe(g, env, name, 2)) == want[name], f"{name} after a refused call"
            seen.add(name)
        assert seen == set(P.SIZED + P.UNSIZED) - {"state", "mallet"}       # these two take no argument to refuse
        # a pending delta
        cooc = P.as_bytes(P.probe(g, env, "cooccurrences", 2))
        g.sample()
        for name in dict.fromkeys(P.ORDER_A):
            if name in ("state", "cooccurrences"):
                continue
            with pytest.raises(capi.LdaError) as e:
                P.probe(g, env, name, 2)
            assert e.value.status == -4, (name, str(e.value))
        with pytest.raises(capi.LdaError) as e:
            g.counts_checksum()
        assert e.value.status == -4
        assert P.as_bytes(P.probe(g, env, "cooccurrences", 2)) == cooc
        g.apply()
        f = _fresh(g, kind, None)
        try:
            for name in dict.fromkeys(reversed(P.ORDER_A)):
                assert P.as_bytes(P.probe(g, env, name, 2)) == P.as_bytes(P.probe(f, env, name, 2)), \
                    f"{name} after the pending delta was refused and applied"
        finally:
            f.close()
    finally:
        g.close()
