"""The brute-force restatement of lda_topic_top_docs in numpy (no device).

nd comes from np.add.at over z; the weight of (document d, topic k) is
    (nd[d, k] + smoothing) / (L_d + float(K) * smoothing)
in float64 with float(K) * smoothing formed first -- the header's expression,
one IEEE rounding per operation, which numpy computes with the same bits.  The
candidates of a topic are the documents with nd[d, k] > 0 and L_d >= min_tokens;
np.lexsort((ids, -w)) orders them by weight descending, equal weights by
ascending id, and the first n are kept.  Integer outputs only, so everything
that is compared against this is compared exactly.
"""
import numpy as np


def doc_topic_counts(z, doc_off, K):
    doc_off = np.asarray(doc_off, np.int64)
    D = len(doc_off) - 1
    nd = np.zeros((D, K), np.int64)
    doc = np.repeat(np.arange(D), np.diff(doc_off))
    np.add.at(nd, (doc, np.asarray(z, np.int64)), 1)
    return nd


def weights(K, smoothing, counts, lengths):
    ks = float(K) * float(smoothing)
    with np.errstate(invalid="ignore"):      # a padded slot at smoothing 0 is 0 / 0: never read
        return (np.asarray(counts, np.float64) + float(smoothing)) / (np.asarray(lengths, np.float64) + ks)


def expected_topic_docs(z, doc_off, K, n, smoothing=0.0, min_tokens=1):
    """(docs int64 [K, n], counts int32 [K, n], lengths int32 [K, n]), padded
    with -1 / 0 / 0."""
    doc_off = np.asarray(doc_off, np.int64)
    nd = doc_topic_counts(z, doc_off, K)
    lens = np.diff(doc_off)
    docs = np.full((K, n), -1, np.int64)
    cnt = np.zeros((K, n), np.int32)
    ln = np.zeros((K, n), np.int32)
    long_enough = lens >= min_tokens
    for k in range(K):
        ids = np.nonzero((nd[:, k] > 0) & long_enough)[0]
        if len(ids) == 0:
            continue
        w = weights(K, smoothing, nd[ids, k], lens[ids])
        order = ids[np.lexsort((ids, -w))][:n]
        docs[k, :len(order)] = order
        cnt[k, :len(order)] = nd[order, k]
        ln[k, :len(order)] = lens[order]
    return docs, cnt, ln


def has_tie(K, smoothing, docs, counts, lengths):
    """Some topic's selection holds two adjacent equal weights, and within
    every such run the ids ascend."""
    w = weights(K, smoothing, counts, lengths)
    valid = (docs[:, :-1] >= 0) & (docs[:, 1:] >= 0)
    eq = valid & (w[:, :-1] == w[:, 1:])
    assert np.all(docs[:, 1:][eq] > docs[:, :-1][eq]), "equal weights out of id order"
    return bool(eq.any())
