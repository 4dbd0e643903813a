"""The inputs, the probes and the plain restatements of test_lifecycle_gpu.py.

A probe is one read-only entry point of GibbsSampler (or a few that belong
together) called with fixed arguments; a sized probe has three argument sets,
index 0 a small call, 1 its largest, 2 another small one, so that a grow-only
scratch buffer is grown and then reused by a smaller call.  probe(ctx, env,
name, i) returns the call's results as a tuple; as_bytes() turns it into the
bytes two contexts are compared by.

The restatements are the existing modules' own (imported, with their bars);
this module only adds the integer ones no module exports: the alpha
statistics, the count histogram and Mallet's packed rows, all from counts().
"""
import ctypes as C

import numpy as np

import coherence_numpy as CN
import ltr_numpy as LN
import test_diagnostics as TDIAG
import test_diagnostics_gpu as DG
import test_heldout_gpu as TH
import test_left_to_right_gpu as TL
import test_readout_gpu as TR
import test_score_gpu as TS
import test_topic_distances_gpu as TDG
import topic_distance_numpy as TD
from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus, document_completion_split, synthetic_lda

V = 400
TOKENS_PER_RANGE = 200
SEED = 20
BETA0 = 0.01
LONG_DOC = 40              # five documents merged: ~250 tokens, then four empty ones
INFER = dict(n_iter=12, thin=3, burn_in=3, seed=9)
COMPLETION = dict(n_iter=12, thin=3, burn_in=3, seed=5)
LTR_SEED = 11
LTR_PARTICLES = (1, 4, 2)
TOP_WORDS_N = (1, 64, 3)
SCORE_Q = (1, 9, 2)
LIST_N = (1, 10, 2)
PROPS = ((), DG.MALLET_PROPS, (0.1, 0.5))
HELD_SUBSETS = ((5,), tuple(range(12)), (3, 0))        # 1, 12 and 2 documents
METRICS = TDG.METRICS
SIZED = ("top_words", "doc_top_topics", "doc_counts", "score_docs", "heldout", "doc_completion", "left_to_right",
         "infer", "codocuments", "word_stats", "cooccurrences", "nearest_topics")
UNSIZED = ("state", "ll", "histograms", "mallet", "topic_distances")
# two orders; each checkpoint takes one of them, rotated.  A holds the chains
# that share scratch (ro_*: top_words -> topic_distances -> nearest_topics;
# held_inv: heldout -> left_to_right -> heldout; dg_* / cc_*: codocuments ->
# word_stats -> cooccurrences), B other neighbours for the same buffers
ORDER_A = ("state", "top_words", "topic_distances", "nearest_topics", "infer", "heldout", "left_to_right", "heldout",
           "doc_completion", "score_docs", "codocuments", "word_stats", "cooccurrences", "doc_top_topics",
           "doc_counts", "ll", "histograms", "mallet")
ORDER_B = ("cooccurrences", "heldout", "doc_counts", "top_words", "left_to_right", "score_docs", "nearest_topics",
           "doc_top_topics", "infer", "word_stats", "topic_distances", "codocuments", "doc_completion", "mallet",
           "state", "histograms", "ll")
CHAINS = (("top_words", "topic_distances"), ("topic_distances", "nearest_topics"), ("heldout", "left_to_right"),
          ("left_to_right", "heldout"), ("codocuments", "word_stats"), ("word_stats", "cooccurrences"))

_cache = {}


def train_corpus():
    """synthetic_lda's 120 documents of about 50 tokens over 400 types, with
    documents made empty (the first, the last and four in the middle, their
    tokens joined to a neighbour: document LONG_DOC holds five documents'
    tokens); some word types have no token."""
    if "train" not in _cache:
        c = synthetic_lda(num_docs=120, num_types=V, num_topics=30, doc_len=None, mean_len=50, min_len=0,
                          max_len=300, seed=77)
        off = c.doc_off.copy()
        off[1] = off[0]
        off[LONG_DOC + 1:LONG_DOC + 5] = off[LONG_DOC + 5]
        off[-2] = off[-1]
        c = Corpus(off, c.words, V)
        lens = np.diff(off)
        assert (lens == 0).sum() >= 6 and lens[0] == 0 and lens[-1] == 0 and 200 <= lens[LONG_DOC] <= 300
        assert c.num_tokens > 25 * TOKENS_PER_RANGE                 # several work ranges
        _cache["train"] = c
    return _cache["train"]


def unseen_word():
    """The smallest word type without a training token."""
    tot = np.bincount(train_corpus().words, minlength=V)
    assert (tot == 0).any()
    return int(np.flatnonzero(tot == 0)[0])


def held_out():
    """12 short held-out documents over the same V: document 0 is empty,
    document 3 holds unseen_word() in the middle, the others hold training
    types only."""
    if "held" not in _cache:
        rng = np.random.default_rng(5)
        seen = np.flatnonzero(np.bincount(train_corpus().words, minlength=V))
        lens = [0, 1, 2, 7, 3, 5, 8, 13, 17, 4, 9, 20]
        docs = [rng.choice(seen, n).astype(np.int32) for n in lens]
        docs[3][3] = unseen_word()
        _cache["held"] = docs
    return _cache["held"]


def held_subset(i):
    docs = [held_out()[d] for d in HELD_SUBSETS[i]]
    off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return off, np.concatenate(docs).astype(np.int32)


def held_split(i):
    off, words = held_subset(i)
    return document_completion_split(Corpus(off, words, V))


def host_corpus():
    """The held-out documents with one token outside the alphabet (-1), as
    lda_word_cooccurrences takes a host corpus."""
    off, words = held_subset(1)
    words = words.copy()
    words[off[7] + 2] = -1
    return off, words


def doc_args(i, D):
    """The documents of the i-th call of a per-document probe: one document
    (the long one), all, a list of five with a repeat and two empty ones."""
    if i == 0:
        return dict(doc_begin=LONG_DOC, num_docs=1), np.array([LONG_DOC])
    if i == 1:
        return dict(), np.arange(D)
    ids = np.array([LONG_DOC + 1, 7, LONG_DOC, 7, D - 1])
    return dict(docs=ids), ids


def word_lists(K, i):
    """K lists of LIST_N[i] different words drawn once from a seeded rng, some
    slots empty (-1)."""
    key = ("lists", K, i)
    if key not in _cache:
        n = LIST_N[i]
        rng = np.random.default_rng(1000 * K + n)
        ids = np.argsort(rng.random((K, V)), axis=1)[:, :n].astype(np.int32)
        ids[::5, (n - 1) // 2] = -1
        _cache[key] = np.ascontiguousarray(ids)
    return _cache[key]


def held_thetas(K, i):
    key = ("theta", K)
    if key not in _cache:
        _cache[key] = np.random.default_rng(K + 3).dirichlet(np.full(K, 0.3), 12)
    return np.ascontiguousarray(_cache[key][list(HELD_SUBSETS[i])])


def score_thetas(K, i):
    return TS._thetas(K, SCORE_Q[i], 100 + SCORE_Q[i])


def nearest_n(K, i):
    """1, the largest the API takes (LDA_TOPIC_NEAREST_MAX), 2."""
    return (1, min(K - 1, capi.TOPIC_NEAREST_MAX), 2)[i]


def nearest_metric(env, i):
    return METRICS[(env["cp"] + i) % 4]


def top_topics_m(K, i):
    return (1, min(K, 16), 2)[i]


COOC_CALLS = (("own", 0), ("own", 5), ("host", 0), ("host", 3))


def probe(ctx, env, name, i=2):
    """One probe's results as a tuple (i: the size index of a sized probe)."""
    K, D = ctx.K, ctx.D
    if name == "state":
        return (ctx.z(),) + tuple(ctx.counts(with_nd=True)) + (ctx.counts_checksum(), ctx.sweep_index,
                                                               ctx.max_doc_length(), ctx.row_stats())
    if name == "ll":
        t = C.c_int64()
        capi.check(ctx._L.lda_log_likelihood_enqueue(ctx._h, C.byref(t)), "lda_log_likelihood_enqueue")
        blocking = ctx.log_likelihood_parts()
        a, b = C.c_double(), C.c_double()
        capi.check(ctx._L.lda_log_likelihood_collect(ctx._h, t.value, C.byref(a), C.byref(b)),
                   "lda_log_likelihood_collect")
        assert (a.value, b.value) == blocking, "the collected ticket differs from the blocking call"
        return blocking
    if name == "histograms":
        return tuple(ctx.doc_topic_histograms()) + (ctx.count_histogram(env["max_count"]),)
    if name == "mallet":
        return ctx.mallet_packed()
    if name == "topic_distances":
        return tuple(ctx.topic_distances(m) for m in METRICS)
    if name == "top_words":
        return ctx.top_words(TOP_WORDS_N[i])
    if name == "doc_top_topics":
        return ctx.doc_top_topics(top_topics_m(K, i), **doc_args(i, D)[0])
    if name == "doc_counts":
        return (ctx.doc_counts(**doc_args(i, D)[0]),)
    if name == "score_docs":
        th, ids = score_thetas(K, i), doc_args(2, D)[1]
        return (ctx.score_docs(th, "cosine"), ctx.score_docs(th, "mse", docs=ids),
                ctx.score_docs(th, "cosine", docs=ids), ctx.score_docs(th, "mse", doc_begin=3, num_docs=D - 10))
    if name == "heldout":
        off, words = held_subset(i)
        return ctx.heldout_loglik(held_thetas(K, i), off, words)
    if name == "doc_completion":
        obs, sc = held_split(i)
        return ctx.doc_completion(obs.doc_off, obs.words, sc.doc_off, sc.words, return_theta=True, **COMPLETION)
    if name == "left_to_right":
        off, words = held_subset(i)
        out = ()
        for resampling in (True, False):
            out += ctx.left_to_right(off, words, LTR_PARTICLES[i], resampling, seed=LTR_SEED, token_prob=True, z=True)
        return out
    if name == "infer":
        off, words = held_subset(i)
        return (ctx.infer(off, words, **INFER),)
    if name == "codocuments":
        return ctx.topic_codocuments(word_lists(K, i), PROPS[i])
    if name == "word_stats":
        return ctx.topic_word_stats(word_lists(K, i))
    if name == "cooccurrences":
        out = ()
        hoff, hwords = host_corpus()
        for where, window in COOC_CALLS:
            out += ctx.word_cooccurrences(word_lists(K, i), window, *((hoff, hwords) if where == "host" else ()))
        return out
    if name == "nearest_topics":
        return ctx.nearest_topics(nearest_n(K, i), nearest_metric(env, i))
    raise KeyError(name)


def as_bytes(result):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in result)


# ------------------------------------------------------------ restatements
def alpha_statistics(nd, lens):
    """(docLengthCounts[L + 1], topicDocCounts[K, L + 1]) of lda_doc_topic_histograms."""
    L = int(lens.max())
    K = nd.shape[1]
    td = np.zeros((K, L + 1), np.int32)
    for k in range(K):
        td[k] = np.bincount(nd[:, k], minlength=L + 1)
    td[:, 0] = 0
    return np.bincount(lens, minlength=L + 1).astype(np.int32), td


def count_histogram(nw, max_count):
    h = np.bincount(nw.reshape(-1), minlength=max_count + 1).astype(np.int32)
    h[0] = 0
    return h


def mallet_packed(nw):
    """typeTopicCounts as Mallet packs it: per word min(K, total) cells, the
    nonzero (count << bits) | topic descending, then zeros."""
    Vn, K = nw.shape
    bits = (K - 1).bit_length()
    rows, off = [], np.zeros(Vn + 1, np.int64)
    topics = np.arange(K, dtype=np.int64)
    for w in range(Vn):
        live = nw[w] > 0
        cells = np.sort((nw[w, live].astype(np.int64) << bits) | topics[live])[::-1]
        row = np.zeros(min(K, int(nw[w].sum())), np.int32)
        row[:len(cells)] = cells
        rows.append(row)
        off[w + 1] = off[w] + len(row)
    return np.concatenate(rows), off, bits


def cooc_presence(where, window):
    """coherence_numpy.presence of the training or the host corpus (it depends
    on the corpus and the window alone: computed once)."""
    key = ("pres", where, window)
    if key not in _cache:
        off, words = host_corpus() if where == "host" else (train_corpus().doc_off, train_corpus().words)
        _cache[key] = CN.presence(off, words, window)
    return _cache[key]


def expected_cooccurrences(K, i, where, window):
    """coherence_numpy.cooccurrences of word_lists(K, i): the call reads
    neither z nor the counts, so one restatement serves every checkpoint."""
    key = ("cooc", K, i, where, window)
    if key not in _cache:
        off, words = host_corpus() if where == "host" else (train_corpus().doc_off, train_corpus().words)
        _cache[key] = CN.cooccurrences(word_lists(K, i), off, words, window, pres=cooc_presence(where, window))
    return _cache[key]


def distance_rows(K):
    """Every topic up to K = 64, else sixteen: the edges of the first and the
    last 64-topic tile and twelve seeded ones (test_topic_distances_gpu
    ._rows_to_check's choice, taken at a smaller K to keep numpy short)."""
    if K <= 64:
        return np.arange(K)
    last = 64 * ((K - 1) // 64)
    fixed = [0, 63, last, K - 1]
    rest = np.setdiff1d(np.arange(K), fixed)
    return np.array(fixed + np.random.default_rng(K).choice(rest, 12, replace=False).tolist())


def check_against_references(g, o, env, results):
    """Assertion C: g's results (results[name, i]) against the plain
    restatements at the current alpha and beta, on g.counts() and g.z(), each
    at the bar its own module states."""
    K, D = g.K, g.D
    alpha, beta = g.alpha, g.beta
    c = train_corpus()
    z = g.z()
    nw, nwsum, nd, ndsum = g.counts(with_nd=True)
    lens = np.diff(c.doc_off)
    nwf, nwsumf = nw.astype(np.float64), nwsum.astype(np.float64)
    what = f"{env['what']} checkpoint {env['cp']} ({env['label']})"
    # log likelihood: the oracle's, 1e-9 relative
    for got, want in zip(results["ll", 0], o.log_likelihood_parts()):
        assert abs(got - want) <= 1e-9 * max(abs(want), 1.0), (what, got, want)
    # held-out likelihood by document completion
    for i in range(3):
        off, words = held_subset(i)
        doc_ll, total = results["heldout", i]
        ref = TH._reference(nwf, nwsumf, V, beta, held_thetas(K, i), off, words)
        bars = TH._bars(ref, np.diff(off), K)
        assert np.all(np.abs(doc_ll - ref) <= bars), (what, i, doc_ll, ref, bars)
        assert total == TH._ordered_sum(doc_ll)
        # doc_completion: infer's theta, then heldout_loglik of it
        obs, sc = held_split(i)
        cll, ctotal, theta = results["doc_completion", i]
        want = o.infer(obs.doc_off, obs.words, n_iter=COMPLETION["n_iter"], burn_in=COMPLETION["burn_in"],
                       thin=COMPLETION["thin"], seed=COMPLETION["seed"])
        np.testing.assert_allclose(theta, want, rtol=0, atol=1e-12, err_msg=what)
        ref = TH._reference(nwf, nwsumf, V, beta, theta, sc.doc_off, sc.words)
        assert np.all(np.abs(cll - ref) <= TH._bars(ref, np.diff(sc.doc_off), K)), (what, i)
        assert ctotal == TH._ordered_sum(cll)
    # left to right: p from the returned topics (every position without
    # resampling, each document's last scored one with it), 1e-11
    phi = LN.phi_table(nw, nwsum, beta)
    for i in range(3):
        off, words = held_subset(i)
        skip = LN.skipped(nw, words)
        res = results["left_to_right", i]
        for j, resampling in enumerate((True, False)):
            doc_ll, total, tokens, tp, zz = res[5 * j:5 * j + 5]
            assert tokens == int((~skip).sum()) and total == TL._ordered_sum(doc_ll), what
            assert np.all(zz[:, skip] == -1) and np.all((zz[:, ~skip] >= 0) & (zz[:, ~skip] < K)), what
            assert np.all((tp == 0) == skip), what
            ref = TL._phat_from_z(phi, alpha, off, words, skip, zz, upto_last=resampling)
            at = ref > 0
            assert at.any() or not (~skip).any()
            np.testing.assert_allclose(tp[at], ref[at], rtol=1e-11, atol=0.0, err_msg=f"{what} size {i}")
    # top topics and document counts, exactly
    for i in range(3):
        ids = doc_args(i, D)[1]
        m = top_topics_m(K, i)
        topics, cnt = results["doc_top_topics", i]
        et, ec = TR.expected_top_topics(nd[ids], lens[ids], alpha, TR._seq_sum(alpha), m)
        np.testing.assert_array_equal(topics, et, err_msg=what)
        np.testing.assert_array_equal(cnt, ec, err_msg=what)
        np.testing.assert_array_equal(results["doc_counts", i][0], nd[ids], err_msg=what)
    # scores
    p = TS._probabilities(nd.astype(np.float64), ndsum.astype(np.float64), alpha)
    Lmax, ids = int(lens.max()), doc_args(2, D)[1]
    for i in range(3):
        th = score_thetas(K, i)
        cos_all, mse_ids, cos_ids, mse_range = results["score_docs", i]
        TS._check(cos_all, th, p, "cosine", Lmax, K)
        TS._check(mse_ids, th, p[ids], "mse", Lmax, K)
        TS._check(cos_ids, th, p[ids], "cosine", Lmax, K)
        TS._check(mse_range, th, p[3:D - 7], "mse", Lmax, K)
    # topic distances, and the nearest topics of the device's own matrix
    rows = distance_rows(K)
    matrices = dict(zip(METRICS, results["topic_distances", 0]))
    for metric in METRICS:
        want = TD.topic_distances(nw, nwsum, beta, metric=metric, rows=rows, squared_hellinger=True)
        TDG._close(matrices[metric][rows], want, metric, what)
    for i in range(3):
        metric = nearest_metric(env, i)
        topics, values = results["nearest_topics", i]
        et, ev = TD.expected_nearest(matrices[metric], nearest_n(K, i), metric, True)
        np.testing.assert_array_equal(topics, et, err_msg=what)
        assert values.tobytes() == ev.tobytes(), what
    # inference: the oracle's
    for i in range(3):
        off, words = held_subset(i)
        want = o.infer(off, words, n_iter=INFER["n_iter"], burn_in=INFER["burn_in"], thin=INFER["thin"],
                       seed=INFER["seed"])
        np.testing.assert_allclose(results["infer", i][0], want, rtol=0, atol=1e-12, err_msg=what)
    # the integer readouts
    for i in range(3):
        ids, cnt = results["top_words", i]
        ei, ec = TR.expected_top_words(nw, TOP_WORDS_N[i])
        np.testing.assert_array_equal(ids, ei, err_msg=what)
        np.testing.assert_array_equal(cnt, ec, err_msg=what)
    nd64 = DG.doc_counts(c.doc_off, z, K)
    np.testing.assert_array_equal(nd64, nd)
    dl, td, ch = results["histograms", 0]
    edl, etd = alpha_statistics(nd, lens)
    np.testing.assert_array_equal(dl, edl, err_msg=what)
    np.testing.assert_array_equal(td, etd, err_msg=what)
    np.testing.assert_array_equal(ch, count_histogram(nw, env["max_count"]), err_msg=what)
    rows_m, off_m, bits = results["mallet", 0]
    er, eo, eb = mallet_packed(nw)
    assert bits == eb
    np.testing.assert_array_equal(off_m, eo, err_msg=what)
    np.testing.assert_array_equal(rows_m, er, err_msg=what)
    for i in range(3):
        lists = word_lists(K, i)
        codoc, stats = results["codocuments", i]
        want_codoc = DG.expected_codoc(DG.presence(c.doc_off, c.words, z, lists, V))
        want_stats = DG.expected_doc_stats(nd64, alpha, PROPS[i])
        np.testing.assert_array_equal(codoc, want_codoc, err_msg=what)
        np.testing.assert_array_equal(stats, want_stats, err_msg=what)
        counts, totals, shares, sumsq = results["word_stats", i]
        ecounts, etotals, eshares, esumsq = DG.expected_word_stats(nw, nwsum, lists, beta)
        np.testing.assert_array_equal(counts, ecounts, err_msg=what)
        np.testing.assert_array_equal(totals, etotals, err_msg=what)
        np.testing.assert_array_equal(sumsq, esumsq, err_msg=what)
        np.testing.assert_allclose(shares, eshares, rtol=1e-13, atol=0, err_msg=what)
        assert np.all(shares[lists < 0] == 0)
        if len(PROPS[i]) >= 7:
            # the eleven columns from the device's statistics and from numpy's
            # (test_diagnostics.restate, rtol = atol = 1e-12), on some topics;
            # restate divides by a listed word's total, so the words without
            # a token stand as empty slots there
            sel = distance_rows(K)
            listed = np.where(etotals > 0, lists, -1)
            cols = lambda sh, cd, st: TDIAG.restate(V, beta, nwsum[sel], td[sel], listed[sel], counts[sel],  # noqa: E731
                                                    totals[sel], sh[sel], sumsq[sel], cd[sel], st[sel])
            np.testing.assert_allclose(cols(shares, codoc, stats), cols(eshares, want_codoc, want_stats),
                                       rtol=1e-12, atol=1e-12, err_msg=what)
        res = results["cooccurrences", i]
        for j, (where, window) in enumerate(COOC_CALLS):
            want, units = expected_cooccurrences(K, i, where, window)
            np.testing.assert_array_equal(res[2 * j], want, err_msg=f"{what} {where} window {window}")
            assert res[2 * j + 1] == units
