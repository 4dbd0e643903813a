"""The probes and the restatements of test_lifecycle_readouts_gpu.py: the six
readout families that came after lifecycle_probes' list -- top documents,
phrases, relevance, topic co-occurrence, groups and the sub-corpus table,
document neighbours -- on lifecycle_probes' corpus, with the three older probes
that use the same ro_* scratch (top_words, topic_distances, doc_counts, taken
from lifecycle_probes unchanged).

As there, a probe is one entry point (or a few that belong together) called
with fixed arguments, a sized probe has three argument sets (0 a small call, 1
the largest the API takes at this shape, 2 another small one), probe(ctx, env,
name, i) returns a tuple and lifecycle_probes.as_bytes() the bytes two contexts
are compared by.

Two probes depend on more than the context's state.  phrase_counts asks for
the phrases that topic_phrases returned at the same size: topic_phrases leaves
them in env["phrases"] under (K, env["cp"], i), and phrase_counts calls
topic_phrases itself where the order has not yet done so at this checkpoint.
The document metric rotates with env["cp"], as nearest_metric does.

test_lifecycle_readouts.py (no device) asserts that these arguments select
what they are meant to select on this corpus.
"""
import numpy as np

import doc_neighbors_numpy as DN
import group_topics_numpy as GN
import lifecycle_probes as P
import relevance_numpy as RN
import test_doc_neighbors_gpu as TDN
import test_readout_gpu as TR
import test_relevance_gpu as TRG
import topic_cooccurrence_numpy as TCN
import topic_docs_numpy as TDOC
import topic_phrases_numpy as TPN
from ldagibbssampling_amd import capi

V = P.V
OLD = ("top_words", "topic_distances", "doc_counts")          # lifecycle_probes' own, the other users of ro_*
NEW_SIZED = ("topic_top_docs", "topic_phrases", "phrase_counts", "relevant_words", "salient_words", "word_rows",
             "topic_cooccurrence", "group_topics", "subcorpus", "doc_distances", "nearest_docs", "doc_neighbors")
SIZED = NEW_SIZED + ("top_words", "doc_counts")
UNSIZED = ("topic_distances",)

TOP_DOCS_N = (1, capi.TOPIC_DOCS_MAX, 3)                      # 128 > D = 120: empty slots
TOP_DOCS_SMOOTHING = (0.0, 10.0, 0.5)
TOP_DOCS_MIN_TOKENS = (1, 1, 60)
PHRASES_N = (1, capi.PHRASES_MAX, 5)
PHRASE_ARGS = ((2, 3, 1), (2, capi.PHRASE_LEN_MAX, 1), (2, 8, 2))     # (min_len, max_len, min_count)
ABSENT_QUERIES = 4                                            # per kind, from the first listed phrases
RELEVANT_N = (1, capi.TOP_WORDS_MAX, 3)                       # batches of 8, 1 and 8 lambdas
LAMBDAS = ((0.6,), tuple(j / 10 for j in range(11)), (0.0, 1.0))
SALIENT_N = (1, capi.SALIENT_WORDS_MAX, 30)
COOC_STATS = (("codocs",), capi.TOPIC_COOC_STATS, ("overlap", "product"))
COOC_STATS_LARGE_K = ((), capi.TOPIC_COOC_STATS, ("overlap",))        # above MAX_TOPICS_DENSE: see cooc_stats
COOC_THRESHOLDS = ((1, 1, 0.0), (10, 2, 0.05), (60, 3, 0.1))  # (min_tokens, min_count, min_prop)
GROUP_STATS = (("present",), capi.GROUP_TOPICS_STATS, ("shares",))
GROUP_THRESHOLDS = ((1, 1, 0.0), (10, 2, 0.05), (60, 2, 0.05))
SUB_N = (1, capi.TOP_WORDS_MAX, 3)
DOC_Q = (1, 70, 2)                                            # 70 crosses the 64-wide query tile
DOC_N = (1, capi.DOC_NEAREST_MAX, 2)
NEAREST_MIN_TOKENS = (1, 2, 60)
NEIGHBOR_MIN_TOKENS = (1, 60, 2)                              # 60 leaves fewer than 64 candidates: exhausted lists
DOC_METRICS = tuple(m for m in P.METRICS if m in capi.DOC_METRICS)

# two orders, as lifecycle_probes has them.  A holds the chains over shared
# scratch (ro_lists: top_words -> subcorpus -> topic_distances -> subcorpus;
# rv_*: relevant_words -> salient_words -> word_rows -> relevant_words; ph_*:
# topic_phrases -> phrase_counts; dn_*: doc_distances -> nearest_docs ->
# doc_neighbors, and doc_counts -> doc_neighbors), B other neighbours
ORDER_A = ("top_words", "subcorpus", "topic_distances", "subcorpus", "relevant_words", "salient_words", "word_rows",
           "relevant_words", "topic_phrases", "phrase_counts", "doc_distances", "nearest_docs", "doc_neighbors",
           "doc_counts", "doc_neighbors", "topic_top_docs", "topic_cooccurrence", "group_topics")
ORDER_B = ("group_topics", "doc_neighbors", "relevant_words", "topic_cooccurrence", "subcorpus", "phrase_counts",
           "top_words", "nearest_docs", "word_rows", "topic_top_docs", "salient_words", "doc_distances",
           "topic_distances", "topic_phrases", "doc_counts")
CHAINS = (("top_words", "subcorpus"), ("subcorpus", "topic_distances"), ("topic_distances", "subcorpus"),
          ("relevant_words", "salient_words"), ("salient_words", "word_rows"), ("word_rows", "relevant_words"),
          ("topic_phrases", "phrase_counts"), ("doc_distances", "nearest_docs"), ("nearest_docs", "doc_neighbors"),
          ("doc_counts", "doc_neighbors"))

_cache = {}


# ------------------------------------------------------------------ inputs
def word_ids(i):
    """One word (the most frequent), every id (unseen_word() among them), five
    with a repeat."""
    if i == 0:
        return np.array([int(np.bincount(P.train_corpus().words, minlength=V).argmax())], np.int32)
    if i == 1:
        return np.arange(V, dtype=np.int32)
    return np.array([5, P.unseen_word(), 5, V - 1, 0], np.int32)


def doc_groups(i):
    """(doc_group[D], G): one group of every document; every document its own
    group (the empty documents' groups stay empty); three groups with every
    seventh document at -1, group 2 holding only documents of fewer than 60
    tokens, so that GROUP_THRESHOLDS[2] leaves it empty."""
    lens = np.diff(P.train_corpus().doc_off)
    D = len(lens)
    if i == 0:
        return np.zeros(D, np.int32), 1
    if i == 1:
        return np.arange(D, dtype=np.int32), D
    g = (np.arange(D) % 3).astype(np.int32)
    g[(g == 2) & (lens >= GROUP_THRESHOLDS[2][0])] = 0
    g[::7] = -1
    return g, 3


def masks(i):
    """(the mask of the first count, the mask accumulated onto it or None):
    no document, then documents 1, 4, 7, ... on top; every document; every
    third document, then 1, 4, 7, ... on top."""
    D = P.train_corpus().num_docs
    d = np.arange(D)
    third, other = (d % 3 == 0).astype(np.uint8), (d % 3 == 1).astype(np.uint8)
    return ((np.zeros(D, np.uint8), other), (np.ones(D, np.uint8), None), (third, other))[i]


def doc_queries(K, i):
    """The query rows of the document probes as keyword arguments: one count
    row, 70 count rows (row 3 all zero: the prior alone), two theta rows (the
    first half zeros, the second not normalised)."""
    key = ("queries", K, i)
    if key not in _cache:
        rng = np.random.default_rng(7000 + 10 * K + i)
        if i < 2:
            counts = rng.integers(0, 6, (DOC_Q[i], K)).astype(np.int32)
            if i == 1:
                counts[3] = 0
            _cache[key] = dict(counts=counts)
        else:
            th = rng.dirichlet(np.full(K, 0.2), DOC_Q[i])
            th[0, :K // 2] = 0.0
            th[0] /= th[0].sum()
            th[1] *= 3.0
            _cache[key] = dict(theta=th)
    return _cache[key]


def cooc_stats(K, i):
    """The K x K tables lda_topic_cooccurrence is asked for: one, all, two.
    Above capi.MAX_TOPICS_DENSE (K = 2048: 32 MiB a table, zeroed, copied and
    compared at every checkpoint) none, all, one: the three layouts of tc_buf
    still differ, and two tables beside the global-atomics path stay covered
    at K = 300 and K = 512."""
    return (COOC_STATS_LARGE_K if K > capi.MAX_TOPICS_DENSE else COOC_STATS)[i]


def doc_metric(env, i):
    return DOC_METRICS[(env["cp"] + i) % len(DOC_METRICS)]


def nearest_skip(i, D):
    """nearest_docs' skip: none, one document per query with every fifth at
    -1, none."""
    if i != 1:
        return None
    skip = np.arange(DOC_Q[1], dtype=np.int64) % D
    skip[::5] = -1
    return skip


def neighbor_docs(i, D):
    """(the docs= argument, the listed ids): doc_args' documents."""
    ids = P.doc_args(i, D)[1]
    return (None if i == 1 else ids), ids


def phrase_queries(K, res, max_len):
    """(topics[Q], phrases) for phrase_counts from a topic_phrases result:
    every listed phrase, then ABSENT_QUERIES of them under the next topic and
    ABSENT_QUERIES extended by their own first word (where max_len allows);
    one made-up query where nothing was listed."""
    words, lens = res[0], res[1]
    listed = [(int(k), words[k, j, :lens[k, j]]) for k, j in zip(*np.nonzero(lens > 0))]
    topics = [k for k, _ in listed]
    phrases = [ph for _, ph in listed]
    for k, ph in listed[:ABSENT_QUERIES]:
        topics.append((k + 1) % K)
        phrases.append(ph)
        if len(ph) < max_len:
            topics.append(k)
            phrases.append(np.append(ph, ph[0]))
    if not topics:
        topics, phrases = [0], [np.array([0, 1], np.int32)]
    return np.array(topics, np.int32), phrases


def _topic_phrases(ctx, env, i):
    res = ctx.topic_phrases(PHRASES_N[i], *PHRASE_ARGS[i])
    env.setdefault("phrases", {})[ctx.K, env["cp"], i] = res
    return res


# ------------------------------------------------------------------ probes
def probe(ctx, env, name, i=2):
    """One probe's results as a tuple (i: the size index of a sized probe)."""
    K, D = ctx.K, ctx.D
    if name in OLD:
        return P.probe(ctx, env, name, i)
    if name == "topic_top_docs":
        return ctx.topic_top_docs(TOP_DOCS_N[i], TOP_DOCS_SMOOTHING[i], TOP_DOCS_MIN_TOKENS[i])
    if name == "topic_phrases":
        return _topic_phrases(ctx, env, i)
    if name == "phrase_counts":
        res = env.get("phrases", {}).get((K, env["cp"], i))
        if res is None:
            res = _topic_phrases(ctx, env, i)
        min_len, max_len, _ = PHRASE_ARGS[i]
        topics, phrases = phrase_queries(K, res, max_len)
        return ctx.phrase_counts(topics, phrases, min_len, max_len, with_first=True)
    if name == "relevant_words":
        return ctx.relevant_words(RELEVANT_N[i], LAMBDAS[i])
    if name == "salient_words":
        return ctx.salient_words(SALIENT_N[i])
    if name == "word_rows":
        return ctx.word_rows(word_ids(i))
    if name == "topic_cooccurrence":
        out = ctx.topic_cooccurrence(cooc_stats(K, i), *COOC_THRESHOLDS[i])
        return (out["docs_used"], out["tokens"], out["present"]) + tuple(out[s] for s in cooc_stats(K, i))
    if name == "group_topics":
        groups, G = doc_groups(i)
        out = ctx.group_topics(groups, G, GROUP_STATS[i], *GROUP_THRESHOLDS[i])
        return (out["group_docs"], out["group_tokens"], out["tokens"]) + tuple(out[s] for s in GROUP_STATS[i])
    if name == "subcorpus":
        first, second = masks(i)
        ctx.subcorpus_count(first)
        out = ctx.subcorpus_top_words(SUB_N[i])
        if second is not None:
            ctx.subcorpus_count(second, accumulate=True)
            out += ctx.subcorpus_top_words(SUB_N[i])
        return out
    if name == "doc_distances":
        return (ctx.doc_distances(doc_metric(env, i), **doc_queries(K, i), **P.doc_args(i, D)[0]),)
    if name == "nearest_docs":
        return ctx.nearest_docs(DOC_N[i], doc_metric(env, i), skip=nearest_skip(i, D),
                                min_tokens=NEAREST_MIN_TOKENS[i], **doc_queries(K, i))
    if name == "doc_neighbors":
        return ctx.doc_neighbors(DOC_N[i], doc_metric(env, i), docs=neighbor_docs(i, D)[0],
                                 min_tokens=NEIGHBOR_MIN_TOKENS[i])
    raise KeyError(name)


# ------------------------------------------------------------ restatements
def _equal(got, want, what):
    assert len(got) == len(want), what
    for j, (a, e) in enumerate(zip(got, want)):
        a, e = np.asarray(a), np.asarray(e)
        assert a.dtype == e.dtype and a.shape == e.shape, (what, j, a.dtype, e.dtype, a.shape, e.shape)
        np.testing.assert_array_equal(a, e, err_msg=f"{what}, output {j}")


def expected_phrase_counts(table, topics, phrases):
    """(counts, first) of lda_phrase_lookup from topic_phrases_numpy's table."""
    hits = [table.get((int(k), tuple(int(w) for w in ph)), (0, -1)) for k, ph in zip(topics, phrases)]
    return np.array([h[0] for h in hits], np.int64), np.array([h[1] for h in hits], np.int64)


def expected_subcorpus(z, K, i):
    """subcorpus' tuple: the top-words restatement over a numpy recount of the
    masked documents, after the first count and after the accumulated one."""
    c = P.train_corpus()
    first, second = masks(i)
    sub = GN.subcorpus_table(z, c.words, c.doc_off, V, K, first)
    out = TR.expected_top_words(sub, SUB_N[i]) + (sub.sum(axis=0).astype(np.int64),)
    if second is not None:
        sub = sub + GN.subcorpus_table(z, c.words, c.doc_off, V, K, second)
        out += TR.expected_top_words(sub, SUB_N[i]) + (sub.sum(axis=0).astype(np.int64),)
    return out


def check_relevant(got, nw, nwsum, beta, n, lambdas, what):
    """lda_relevant_words' arrays against relevance_numpy's tables, at
    test_relevance_gpu's bars applied slot by slot.  That module compares ids
    with the restatement's after asserting that the fixture holds no two
    unequal-input keys within relevance_numpy.GAP of each other; a sampled
    chain does hold such pairs (two words whose keys agree to the last bit
    through different counts), so here the same rule is applied to the list
    itself: the listed words are candidates, as many as there are up to n and
    each once; their counts and totals are exact and logprob / loglift within
    TOL; two neighbours of identical inputs stand in id order, any other two
    are not out of order by more than GAP, and no word left out beats the last
    listed one by more than GAP.  Wherever the restatement's keys are further
    apart than GAP this is the restatement's list exactly."""
    ids, cnt, tot, lp, ll = got
    nw = np.asarray(nw, np.int64)
    K = nw.shape[1]
    lam = np.asarray(lambdas, np.float64)
    tw, _, logprob, logtp = RN.tables(nw, nwsum, beta)
    for a, dtype in zip(got, (np.int32, np.int32, np.int64, np.float64, np.float64)):
        assert a.dtype == dtype and a.shape == (lam.size, K, n), what
    live = ids >= 0
    listed = np.minimum(n, (nw > 0).sum(axis=0))
    assert np.all(live == (np.arange(n)[None, None, :] < listed[None, :, None])), what
    assert np.all(ids[~live] == -1), what
    w = np.where(live, ids, 0)
    kk = np.arange(K)[None, :, None]
    c = nw[w, kk]
    assert np.all(c[live] > 0), what
    distinct = np.sort(np.where(live, ids, -1 - np.arange(n)), axis=2)
    assert np.all(distinct[:, :, 1:] != distinct[:, :, :-1]), what
    np.testing.assert_array_equal(cnt, np.where(live, c, 0), err_msg=what)
    np.testing.assert_array_equal(tot, np.where(live, tw[w], 0), err_msg=what)
    TRG._close(lp, np.where(live, logprob[w, kk], 0.0), what + " logprob")
    TRG._close(ll, np.where(live, logprob[w, kk] - logtp[w], 0.0), what + " loglift")
    m = 1.0 - lam
    key = logprob[w, kk] - m[:, None, None] * logtp[w]
    both = live[:, :, 1:]
    same = (c[:, :, :-1] == c[:, :, 1:]) & ((tw[w][:, :, :-1] == tw[w][:, :, 1:]) | (lam == 1.0)[:, None, None])
    assert np.all(ids[:, :, :-1][both & same] < ids[:, :, 1:][both & same]), what + ": equal keys out of id order"
    with np.errstate(invalid="ignore"):
        d = key[:, :, :-1] - key[:, :, 1:]
    assert np.all(d[both & ~same] > -RN.GAP), (what, float(d[both & ~same].min()))
    full_lists = np.nonzero((nw > 0).sum(axis=0) > n)[0]
    for l in range(lam.size):
        left = np.where(nw > 0, logprob - m[l] * logtp[:, None], -np.inf)
        left[w[l].T, np.arange(K)[None, :]] = np.where(live[l].T, -np.inf, left[w[l].T, np.arange(K)[None, :]])
        best, last = left.max(axis=0)[full_lists], key[l, full_lists, n - 1]
        assert np.all(best <= last + RN.GAP), (what, l)


def check_salient(got, nw, nwsum, n, what):
    """lda_salient_words' arrays, by check_relevant's rule: identical inputs
    are identical rows of nw, and GAP is relative, as check_saliency_gaps
    takes it."""
    ids, tot, sal, dist = got
    nw = np.asarray(nw, np.int64)
    tw, esal, edist = RN.saliency(nw, nwsum)
    for a, dtype in zip(got, (np.int32, np.int64, np.float64, np.float64)):
        assert a.dtype == dtype and a.shape == (n,), what
    listed = min(n, int((tw > 0).sum()))
    assert np.all(ids[:listed] >= 0) and np.all(ids[listed:] == -1) and len(set(ids[:listed].tolist())) == listed, what
    w = ids[:listed]
    assert np.all(tw[w] > 0), what
    np.testing.assert_array_equal(tot, np.append(tw[w], np.zeros(n - listed, np.int64)), err_msg=what)
    TRG._close(sal, np.append(esal[w], np.zeros(n - listed)), what + " saliency")
    TRG._close(dist, np.append(edist[w], np.zeros(n - listed)), what + " distinctiveness")
    same = (nw[w[:-1]] == nw[w[1:]]).all(axis=1)
    assert np.all(w[:-1][same] < w[1:][same]), what + ": equal saliencies out of id order"
    rel = (esal[w[:-1]] - esal[w[1:]]) / np.abs(esal[w[:-1]])
    assert np.all(rel[~same] > -RN.GAP), (what, float(rel[~same].min()) if (~same).any() else 0.0)
    if listed == n and (tw > 0).sum() > n:
        left = np.where(tw > 0, esal, -np.inf)
        left[w] = -np.inf
        assert (left.max() - esal[w[-1]]) / abs(esal[w[-1]]) <= RN.GAP, what


def check_against_references(g, env, results):
    """Assertion C: g's results (results[name, i]) against the numpy
    restatements at the current alpha and beta, on g.z(), g.counts() and
    g.doc_counts(), each at the bar of the module it comes from: integers and
    selections exactly (tie order included); logprob, loglift, saliency and
    distinctiveness within test_relevance_gpu.TOL, relative, and their orders
    wherever the restatement's own keys are further apart than its GAP
    (check_relevant); the document distances within
    test_doc_neighbors_gpu.TOL, absolute, Hellinger by its square, and the
    document selections as np.lexsort of the device's own matrix, bit for bit."""
    K, D = g.K, g.D
    alpha, beta = g.alpha, g.beta
    c = P.train_corpus()
    off, lens = c.doc_off, np.diff(c.doc_off)
    z = g.z()
    nw, nwsum = g.counts()[:2]
    nd = g.doc_counts()
    np.testing.assert_array_equal(nd, TDOC.doc_topic_counts(z, off, K))
    what = f"{env['what']} checkpoint {env['cp']} ({env['label']})"
    for i in range(3):
        at = f"{what} size {i}"
        # the older users of ro_*
        _equal(results["top_words", i], TR.expected_top_words(nw, P.TOP_WORDS_N[i]), at + " top_words")
        np.testing.assert_array_equal(results["doc_counts", i][0], nd[P.doc_args(i, D)[1]], err_msg=at)
        # top documents
        _equal(results["topic_top_docs", i],
               TDOC.expected_topic_docs(z, off, K, TOP_DOCS_N[i], TOP_DOCS_SMOOTHING[i], TOP_DOCS_MIN_TOKENS[i]),
               at + " topic_top_docs")
        # phrases, and the lookups of the listed ones and of the absent ones
        min_len, max_len, min_count = PHRASE_ARGS[i]
        res = results["topic_phrases", i]
        want = TPN.expected_topic_phrases(c.words, z, off, K, PHRASES_N[i], min_len, max_len, min_count)
        _equal(res[:6], want[:6], at + " topic_phrases")
        assert res[6] == want[6], at
        topics, phrases = phrase_queries(K, res, max_len)
        table, _ = TPN.phrase_table(c.words, z, off, min_len, max_len)
        _equal(results["phrase_counts", i], expected_phrase_counts(table, topics, phrases), at + " phrase_counts")
        # word rows
        ids = word_ids(i)
        _equal(results["word_rows", i], (nw[ids], nw.astype(np.int64).sum(axis=1)[ids]), at + " word_rows")
        # topic co-occurrence
        mt, mc, mp = COOC_THRESHOLDS[i]
        e = TCN.expected_cooccurrence(z, off, K, mt, mc, mp, cooc_stats(K, i))
        got = results["topic_cooccurrence", i]
        assert got[0] == e["docs_used"], at
        _equal(got[1:], (e["tokens"], e["present"]) + tuple(e[s] for s in cooc_stats(K, i)),
               at + " topic_cooccurrence")
        # groups
        groups, G = doc_groups(i)
        mt, mc, mp = GROUP_THRESHOLDS[i]
        e = GN.expected_group_topics(z, off, K, groups, G, mt, mc, mp, GROUP_STATS[i])
        _equal(results["group_topics", i],
               (e["group_docs"], e["group_tokens"], e["tokens"]) + tuple(e[s] for s in GROUP_STATS[i]),
               at + " group_topics")
        # the sub-corpus table's top words
        _equal(results["subcorpus", i], expected_subcorpus(z, K, i), at + " subcorpus")
        check_salient(results["salient_words", i], nw, nwsum, SALIENT_N[i], at + " salient_words")
        check_relevant(results["relevant_words", i], nw, nwsum, beta, RELEVANT_N[i], LAMBDAS[i],
                       at + " relevant_words")
    # the document calls
    rows = DN.rows_from_counts(nd, alpha)
    for i in range(3):
        at = f"{what} size {i}"
        metric = doc_metric(env, i)
        q = doc_queries(K, i)
        qrows = DN.rows_from_counts(q["counts"], alpha) if "counts" in q else q["theta"]
        ids = P.doc_args(i, D)[1]
        TDN._close(results["doc_distances", i][0], DN.distances(qrows, rows[ids], metric, squared_hellinger=True),
                   metric, at + " doc_distances")
        matrix = g.doc_distances(metric, **q)                       # every document: the selection's own values
        if i == 1:
            assert matrix.tobytes() == results["doc_distances", i][0].tobytes(), at
        TDN._same(results["nearest_docs", i],
                  DN.nearest(matrix, DOC_N[i], metric, lengths=lens, min_tokens=NEAREST_MIN_TOKENS[i],
                             skip=nearest_skip(i, D)), at + " nearest_docs")
        ids = neighbor_docs(i, D)[1]
        own = g.doc_distances(metric, counts=nd[ids])
        TDN._close(own, DN.distances(rows[ids], rows, metric, squared_hellinger=True), metric, at + " neighbours' rows")
        TDN._same(results["doc_neighbors", i],
                  DN.nearest(own, DOC_N[i], metric, lengths=lens, min_tokens=NEIGHBOR_MIN_TOKENS[i], skip=ids),
                  at + " doc_neighbors")
