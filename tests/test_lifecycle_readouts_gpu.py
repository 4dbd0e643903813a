"""test_lifecycle_gpu.py's long-lived context, for the six readout families
that came after it: top documents, phrases, relevance, topic co-occurrence,
groups and the sub-corpus table, document neighbours
(lifecycle_readout_probes.probe), with top_words, topic_distances and
doc_counts beside them as the other users of the ro_* scratch.

The state changes are steps 1 to 9 of test_lifecycle (sweeps one by one, graph
launched, split, by hand, recounted; alpha, beta and z replaced; the stream
changed), on the same four sampler families and the same corpus.  After each,
a checkpoint calls every probe three times in a row (a small size, the largest
the API takes, another small one) in ORDER_A or ORDER_B rotated by
3 (cp // 2); a probe an order names twice must repeat its bytes.  Every second
checkpoint ends with lda_subcorpus_release, so the sub-corpus table is made
afresh at one checkpoint and reused, holding the last checkpoint's counts, at
the next.  Asserted:

  A  the chain is untouched: z, the counts, the sweep counter and the checksum
     equal cpu_exact's, which saw none of the probes;
  B  history does not matter: a context made afresh from (z, alpha, beta, the
     seed) gives for every probe at its last size, called in the reverse
     order, the same bytes.  DESIGN.md 9i to 9n document every one of these
     calls as bit-repeatable (integer atomics, ordered fp64 chains), so
     equality is the bar for all of them;
  C  at the checkpoints after set_alpha_beta (twice: with nothing pending and
     between sample and apply), after set_z and after the recount sweeps (the
     dense samplers) the results equal the numpy restatements at the current
     alpha and beta (lifecycle_readout_probes.check_against_references).

Each case ends with the coverage assertion: every (checkpoint, probe, size)
ran and every adjacency of lifecycle_readout_probes.CHAINS occurred.

Then: every new entry point refuses a pending delta and finds its scratch
usable afterwards; two contexts alive at once with the six process-wide hooks
made small; lda_subcorpus_merge between two contexts.

On an MI355X the slowest case, sparse K = 2048 (14 checkpoints, 602 probe
calls on the long-lived context, 14 fresh contexts, 3 rounds of numpy
restatements of 0.7 s each), takes 6.5 s, against 5.4 s for the same case of
test_lifecycle_gpu.py in the same run (7.6 s against 6.2 s inside the whole
suite); the others 0.7 to 2.4 s.  With
lda_topic_cooccurrence asked for one, all and two K x K tables at K = 2048 as
at the other shapes the case took 7.9 s, nearly half of it spent zeroing,
copying and comparing 32 MiB tables, so above capi.MAX_TOPICS_DENSE the
requests are none, all and one (lifecycle_readout_probes.cooc_stats); no size,
adjacency or checkpoint was cut.
"""
import time

import numpy as np
import pytest

import group_topics_numpy as GN
import lifecycle_probes as P
import lifecycle_readout_probes as R
import test_readout_gpu as TR
from ldagibbssampling_amd import capi
from test_lifecycle_gpu import CASES, _chain_equal, _foreign, _fresh, _make, _oracle

pytestmark = pytest.mark.gpu


def _alpha0(K):
    return np.full(K, 0.1)


def _env(what=""):
    return dict(cp=0, what=what, label="", max_count=P.train_corpus().num_tokens + 16)


class _Life:
    """The long-lived context g, its mirror o and the bookkeeping of one case."""

    def __init__(self, oracle, kind, K):
        self.oracle, self.kind, self.K = oracle, kind, K
        self.alpha, self.beta = _alpha0(K), P.BETA0
        self.foreign = _foreign(K, capi.padded_topics(K))
        self.g = _make(kind, K, self.alpha, self.beta, foreign=self.foreign)
        self.o = _oracle(oracle, kind, K, self.alpha, self.beta, foreign=self.foreign)
        self.env = _env(f"{kind} K={K}")
        self.env["cp"] = -1
        self.ran = set()            # (checkpoint, probe, size index)
        self.adjacent = set()       # (probe, the probe right after it), across the case
        self.labels = []
        self.refs = 0

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
        base = R.ORDER_A if cp % 2 == 0 else R.ORDER_B
        shift = (3 * (cp // 2)) % len(base)
        order = base[shift:] + base[:shift]
        results, last = {}, {}
        for prev, name in zip((None,) + order, order):
            if prev is not None:
                self.adjacent.add((prev, name))
            for i in (range(3) if name in R.SIZED else (0,)):
                res = R.probe(g, env, name, i)
                if (name, i) in results:
                    assert P.as_bytes(res) == P.as_bytes(results[name, i]), f"{what}: {name} size {i} does not repeat"
                results[name, i] = res
                self.ran.add((cp, name, i))
            last[name] = P.as_bytes(results[name, 2 if name in R.SIZED else 0])
        _chain_equal(g, self.o, self.oracle, what + ": the chain after the probes")
        f = _fresh(g, self.kind, self.foreign)
        try:
            for name in dict.fromkeys(reversed(order)):
                assert P.as_bytes(R.probe(f, env, name, 2)) == last[name], \
                    f"{what}: {name} depends on the context's history"
        finally:
            f.close()
        if refs:
            R.check_against_references(g, env, results)
            self.refs += 1
        if cp % 2:
            g.subcorpus_release()
        _chain_equal(g, self.o, self.oracle, what + ": the chain at the end of the checkpoint")

    def coverage(self):
        """(missing, summary): every (probe, size) at every checkpoint, every
        shared-scratch adjacency in the case."""
        cps = len(self.labels)
        want = {(cp, n, i) for cp in range(cps) for n in R.SIZED for i in range(3)}
        want |= {(cp, n, 0) for cp in range(cps) for n in R.UNSIZED}
        missing = sorted(want - self.ran) + sorted(set(R.CHAINS) - self.adjacent)
        summary = (f"{self.env['what']}: {cps} checkpoints {self.labels}, {self.refs} of them against numpy; "
                   f"{len(self.ran)} probe calls of {len(want)}; {len(self.adjacent)} different adjacencies, chains "
                   f"{sorted(set(R.CHAINS) & self.adjacent)}; missing {missing}")
        return missing, summary


@pytest.mark.parametrize("kind,K", CASES)
def test_lifecycle_readouts(oracle, kind, K):
    import torch
    t0 = time.perf_counter()
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
        L.checkpoint("4: sweep(2)")
        # 5. ... and between sample and apply
        L.both("sample")
        L.set_alpha_beta(rng.gamma(0.5, 0.4, K) + 0.01, P.BETA0 * 3 / 5)
        L.both("apply")
        L.checkpoint("5: sample, set_alpha_beta, apply", refs=True)
        L.both("sweep", 1)
        L.checkpoint("5: sweep(1)")
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
        L.checkpoint("7: set_z, sweep(0)", refs=True)
        L.both("sweep", 2)
        L.checkpoint("7: sweep(2)")
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
            L.checkpoint("9: recount, sweep(2)", refs=True)
            g.set_count_update("delta")
            L.both("sweep", 1)
            L.checkpoint("9: delta, sweep(1)")
        missing, summary = L.coverage()
        print(summary)
        print(f"{kind} K={K}: {time.perf_counter() - t0:.1f} s")
        assert not missing, summary
    finally:
        L.g.close()


# ------------------------------------------------------------ a pending delta
def _refused(g, other):
    """Every new entry point as (name, call); `other` is an applied context of
    g's shape with a sub-corpus table."""
    K, D = g.K, g.D
    q = R.doc_queries(K, 1)
    groups, G = R.doc_groups(2)
    phrases = [np.array([1, 2], np.int32)]
    return [
        ("lda_topic_top_docs", lambda: g.topic_top_docs(3)),
        ("lda_topic_phrases", lambda: g.topic_phrases(5)),
        ("lda_phrase_counts", lambda: g.phrase_counts([0], phrases)),
        ("lda_phrase_lookup", lambda: g.phrase_counts([0], phrases, with_first=True)),
        ("lda_relevant_words", lambda: g.relevant_words(3, R.LAMBDAS[2])),
        ("lda_salient_words", lambda: g.salient_words(30)),
        ("lda_word_rows", lambda: g.word_rows(R.word_ids(2))),
        ("lda_topic_cooccurrence", lambda: g.topic_cooccurrence(R.cooc_stats(K, 2))),
        ("lda_group_topics", lambda: g.group_topics(groups, G)),
        ("lda_subcorpus_count", lambda: g.subcorpus_count(R.masks(2)[0])),
        ("lda_subcorpus_count", lambda: g.subcorpus_count(R.masks(2)[1], accumulate=True)),
        ("lda_subcorpus_merge", lambda: g.subcorpus_merge(other)),
        ("lda_subcorpus_merge", lambda: other.subcorpus_merge(g)),
        ("lda_subcorpus_top_words", lambda: g.subcorpus_top_words(3)),
        ("lda_doc_distances", lambda: g.doc_distances("cosine", **q)),
        ("lda_doc_nearest", lambda: g.nearest_docs(2, "hellinger", **q)),
        ("lda_doc_neighbors", lambda: g.doc_neighbors(2, "jensen_shannon", docs=[0, D - 1])),
    ]


@pytest.mark.parametrize("kind,K", [("dense", 20), ("sparse", 2048)])
def test_pending_delta_is_refused_and_scratch_survives(kind, K):
    """Between sample() and apply() every new entry point, lda_subcorpus_merge
    on either side included, answers LDA_ERR_STATE and names the pending
    delta, with the largest call's leftovers in its scratch; after apply() each
    probe at its largest size gives what a context made afresh gives."""
    env = _env(f"{kind} K={K}")
    g = _make(kind, K, _alpha0(K), P.BETA0)
    try:
        g.sweep(2)
        other = _fresh(g, kind, None)
        try:
            other.subcorpus_count(R.masks(1)[0])
            for name in dict.fromkeys(R.ORDER_A):
                R.probe(g, env, name, 1)
            table = P.as_bytes(other.subcorpus_top_words(5))
            g.sample()
            for where, call in _refused(g, other):
                with pytest.raises(capi.LdaError) as e:
                    call()
                assert e.value.status == -4, (where, str(e.value))
                assert str(e.value).startswith(where + ": LDA_ERR_STATE"), str(e.value)
                assert "pending delta" in str(e.value), str(e.value)
            assert P.as_bytes(other.subcorpus_top_words(5)) == table          # the refused merge added nothing
        finally:
            other.close()
        g.apply()
        env["cp"] = 1                                                         # another state: other phrases
        got = {name: P.as_bytes(R.probe(g, env, name, 1)) for name in dict.fromkeys(R.ORDER_A)}
        f = _fresh(g, kind, None)
        try:
            for name in dict.fromkeys(reversed(R.ORDER_A)):
                assert P.as_bytes(R.probe(f, env, name, 1)) == got[name], \
                    f"{name} after the pending delta was refused and applied"
        finally:
            f.close()
    finally:
        g.close()


# ------------------------------------------------- two contexts and the hooks
def _final_sizes(ctx, env):
    """Every probe at its largest and its last size."""
    out = {}
    for name in dict.fromkeys(R.ORDER_A):
        for i in ((1, 2) if name in R.SIZED else (0,)):
            out[name, i] = P.as_bytes(R.probe(ctx, env, name, i))
    return out


def _set_hooks(lib, on):
    lib.lda_debug_topic_docs_chunk_docs(37 if on else 0)          # D = 120: four chunks, the last of 9
    lib.lda_debug_relevance_slab_rows(64 if on else 0)            # V = 400: seven slabs, the last of 16 rows
    lib.lda_debug_phrase_table_slots(64 if on else 0)             # many passes
    lib.lda_debug_doc_nearest_chunk(64 if on else 0, 3 if on else 0)      # two candidate chunks, 3 queries a chunk
    lib.lda_debug_topic_cooccurrence_global(1 if on else 0)
    lib.lda_debug_group_topics_global(1 if on else 0)


def test_two_contexts_and_hooks():
    """A quarter-wave K = 20 and a large-K sparse K = 2048 context over the
    same V, their calls alternated, with the six process-wide hooks of the new
    families made small meanwhile: each gives what it gives alone with the
    hooks off (every one of these results is specified as independent of the
    chunking and of the accumulation path).  Then lda_subcorpus_merge: two
    contexts of one shape and state count disjoint masks, and the merged table
    is one context's count of the union; after the source's release the merge
    answers LDA_ERR_STATE."""
    env = _env()
    shapes = [("dense", 20), ("sparse", 2048)]
    alone = []
    for kind, K in shapes:
        with _make(kind, K, _alpha0(K), P.BETA0) as g:
            g.sweep(2)
            alone.append(_final_sizes(g, env))
    lib = capi.load()
    a, b = (_make(kind, K, _alpha0(K), P.BETA0) for kind, K in shapes)
    try:
        _set_hooks(lib, True)
        for _ in range(2):
            a.sweep(1)
            b.sweep(1)
        for name in dict.fromkeys(R.ORDER_A):
            for i in ((1, 2) if name in R.SIZED else (0,)):
                got = [P.as_bytes(R.probe(ctx, env, name, i)) for ctx in (a, b)]
                for j in range(2):
                    assert got[j] == alone[j][name, i], (shapes[j], name, i)
    finally:
        _set_hooks(lib, False)
        a.close()
        b.close()
    # the merge
    first, second = R.masks(2)
    union = (first | second).astype(np.uint8)
    assert first.any() and second.any() and not (first & second).any()
    for kind, K in shapes:
        a, b = (_make(kind, K, _alpha0(K), P.BETA0) for _ in range(2))
        try:
            a.sweep(2)
            b.sweep(2)
            assert np.array_equal(a.z(), b.z())
            a.subcorpus_count(first)
            b.subcorpus_count(second)
            before = P.as_bytes(b.subcorpus_top_words(capi.TOP_WORDS_MAX))
            a.subcorpus_merge(b)
            merged = P.as_bytes(a.subcorpus_top_words(capi.TOP_WORDS_MAX))
            assert P.as_bytes(b.subcorpus_top_words(capi.TOP_WORDS_MAX)) == before        # the source is unchanged
            b.subcorpus_count(union)
            assert P.as_bytes(b.subcorpus_top_words(capi.TOP_WORDS_MAX)) == merged, (kind, K)
            c = P.train_corpus()
            sub = GN.subcorpus_table(a.z(), c.words, c.doc_off, P.V, K, union)           # numpy's recount of the union
            assert merged == P.as_bytes(TR.expected_top_words(sub, capi.TOP_WORDS_MAX) + (sub.sum(axis=0),)), (kind, K)
            b.subcorpus_release()
            with pytest.raises(capi.LdaError) as e:
                a.subcorpus_merge(b)
            assert e.value.status == -4 and "without a table" in str(e.value), str(e.value)
            assert P.as_bytes(a.subcorpus_top_words(capi.TOP_WORDS_MAX)) == merged        # and added nothing
        finally:
            a.close()
            b.close()
