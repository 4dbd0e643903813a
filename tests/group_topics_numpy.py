"""The numpy restatement of lda_group_topics, of the kinds of prevalence built
on it and of the sub-corpus topic words.  Every GPU expectation
of test_group_topics_gpu.py comes from here; test_group_topics.py checks it
against an example worked by hand.

doc_group[d] in [-1, G).  A document is used when its group is >= 0 and
L_d >= min_tokens.  Topic k is present in it when n_dk >= min_count and
float64(n_dk) >= float64(min_prop) * float64(L_d): one fp64 product and one
compare, as the kernel does it.  Over the used documents of group g:
group_docs[g] = their number, group_tokens[g] = sum L_d, tokens[g, k] = sum
n_dk, present[g, k] = documents with k present, shares[g, k] = sum of
floor(n_dk * 2^32 / L_d), in Python integers.

Sub-corpus words: sub[w, k] = tokens of word w with topic k in the documents
whose mask entry is nonzero; per topic the words by (count descending, word
ascending), zero counts left out, -1 / 0 past the last; totals[k] = column sum.
"""
import math

import numpy as np

STATS = ("present", "shares")
KINDS = ("tokens", "documents", "mean", "lift")


def expected_group_topics(z, doc_off, K, doc_group, G, min_tokens=10, min_count=2, min_prop=0.05, stats=STATS):
    """The dict GibbsSampler.group_topics returns, document by document."""
    z = np.asarray(z)
    doc_off = np.asarray(doc_off, np.int64)
    out = {"group_docs": np.zeros(G, np.int64), "group_tokens": np.zeros(G, np.int64),
           "tokens": np.zeros((G, K), np.int64)}
    if "present" in stats:
        out["present"] = np.zeros((G, K), np.int64)
    shares = [[0] * K for _ in range(G)] if "shares" in stats else None
    for d in range(len(doc_off) - 1):
        g = int(doc_group[d])
        L = int(doc_off[d + 1] - doc_off[d])
        if g < 0 or L < min_tokens:
            continue
        out["group_docs"][g] += 1
        out["group_tokens"][g] += L
        nd = np.bincount(z[doc_off[d]:doc_off[d + 1]], minlength=K).astype(np.int64)
        ks = np.nonzero(nd)[0]
        c = nd[ks]
        out["tokens"][g, ks] += c
        if "present" in out:
            here = (c >= min_count) & (c.astype(np.float64) >= np.float64(min_prop) * np.float64(L))
            out["present"][g, ks[here]] += 1
        if shares is not None:
            for k, n in zip(ks.tolist(), c.tolist()):
                shares[g][k] += (n << 32) // L
    if shares is not None:
        out["shares"] = np.array(shares, dtype=np.uint64).reshape(G, K)
    return out


def finish(kind, group_docs, group_tokens, tokens, present=None, shares=None):
    """ldatm_group_prevalence_finish, cell by cell in Python: every integer
    becomes a float once, then one rounding per operation."""
    tokens = np.asarray(tokens)
    G, K = tokens.shape
    gd = [int(x) for x in group_docs]
    gt = [int(x) for x in group_tokens]
    T = [[int(x) for x in row] for row in tokens]
    nk = [sum(T[g][k] for g in range(G)) for k in range(K)]
    n_all = sum(gt)
    out = np.full((G, K), np.nan)
    for g in range(G):
        for k in range(K):
            if kind == "tokens":
                if gt[g]:
                    out[g, k] = float(T[g][k]) / float(gt[g])
            elif kind == "documents":
                if gd[g]:
                    out[g, k] = float(int(present[g][k])) / float(gd[g])
            elif kind == "mean":
                if gd[g]:
                    out[g, k] = float(int(shares[g][k])) / (4294967296.0 * float(gd[g]))
            elif kind == "lift":
                if gt[g] and nk[k] and n_all:
                    out[g, k] = -math.inf if T[g][k] == 0 else \
                        math.log((float(T[g][k]) / float(gt[g])) / (float(nk[k]) / float(n_all)))
            else:
                raise ValueError(kind)
    return out


def top_topics(matrix, n):
    """Per row its n largest finite values, larger first, equal values by
    smaller id; -1 / NaN past the last."""
    matrix = np.asarray(matrix, np.float64)
    G, K = matrix.shape
    ids = np.full((G, n), -1, np.int32)
    values = np.full((G, n), np.nan)
    for g in range(G):
        cand = [k for k in range(K) if math.isfinite(matrix[g, k])]
        cand.sort(key=lambda k: (-matrix[g, k], k))
        for i, k in enumerate(cand[:n]):
            ids[g, i] = k
            values[g, i] = matrix[g, k]
    return ids, values


def subcorpus_table(z, words, doc_off, V, K, mask):
    """sub[V, K] int64 of the masked documents, by np.add.at."""
    doc_off = np.asarray(doc_off, np.int64)
    keep = np.repeat(np.asarray(mask) != 0, np.diff(doc_off))
    sub = np.zeros((V, K), np.int64)
    np.add.at(sub, (np.asarray(words, np.int64)[keep], np.asarray(z, np.int64)[keep]), 1)
    return sub


def table_top_words(sub, n):
    """(word_ids[K, n], counts[K, n]) int32 and totals[K] int64 of a [V, K]
    table: a stable sort on (-count, word), zero counts left out."""
    sub = np.asarray(sub, np.int64)
    V, K = sub.shape
    ids = np.full((K, n), -1, np.int32)
    cnt = np.zeros((K, n), np.int32)
    for k in range(K):
        order = np.lexsort((np.arange(V), -sub[:, k]))          # by -count, then word
        order = order[sub[order, k] > 0][:n]
        ids[k, :len(order)] = order
        cnt[k, :len(order)] = sub[order, k]
    return ids, cnt, sub.sum(axis=0).astype(np.int64)


def same_floats(a, b):
    """Equal bit for bit up to the kind of a NaN: the same NaN positions and
    identical values (signed infinities included) elsewhere."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
