"""The numpy restatement of lda_topic_cooccurrence and of the measures built on
it.  Every GPU expectation of test_topic_cooccurrence_gpu.py
comes from here; test_topic_cooccurrence.py checks it against an example worked
by hand.

A document is used when L_d >= min_tokens.  Topic k is present in it when
n_dk >= min_count and float64(n_dk) >= float64(min_prop) * float64(L_d): one
fp64 product and one compare, as the kernel does it.  Over the used documents:
docs_used, tokens[k] = sum n_dk, present[k] = documents with k present,
codocs[k, l] = documents with both present, overlap[k, l] = sum min(n_dk, n_dl),
product[k, l] = sum n_dk n_dl; overlap and product over every nonzero topic.
"""
import math

import numpy as np

STATS = ("codocs", "overlap", "product")


def expected_cooccurrence(z, doc_off, K, min_tokens=10, min_count=2, min_prop=0.05, stats=STATS):
    """The dict GibbsSampler.topic_cooccurrence returns, document by document."""
    z = np.asarray(z)
    doc_off = np.asarray(doc_off, np.int64)
    out = {"docs_used": 0, "tokens": np.zeros(K, np.int64), "present": np.zeros(K, np.int64)}
    for s in stats:
        out[s] = np.zeros((K, K), np.int64)
    for d in range(len(doc_off) - 1):
        L = int(doc_off[d + 1] - doc_off[d])
        if L < min_tokens:
            continue
        out["docs_used"] += 1
        nd = np.bincount(z[doc_off[d]:doc_off[d + 1]], minlength=K).astype(np.int64)
        ks = np.nonzero(nd)[0]
        c = nd[ks]
        out["tokens"][ks] += c
        here = (c >= min_count) & (c.astype(np.float64) >= np.float64(min_prop) * np.float64(L))
        out["present"][ks[here]] += 1
        if "codocs" in out:
            out["codocs"][np.ix_(ks[here], ks[here])] += 1
        if "overlap" in out:
            out["overlap"][np.ix_(ks, ks)] += np.minimum.outer(c, c)
        if "product" in out:
            out["product"][np.ix_(ks, ks)] += np.multiply.outer(c, c)
    return out


def doc_topic_counts(z, doc_off, K):
    """nd[D, K] int64, the dense table the device never builds."""
    doc_off = np.asarray(doc_off, np.int64)
    D = len(doc_off) - 1
    nd = np.zeros((D, K), np.int64)
    np.add.at(nd, (np.repeat(np.arange(D), np.diff(doc_off)), np.asarray(z, np.int64)), 1)
    return nd


def finish(measure, docs_used, tokens, present, table):
    """ldatm_topic_correlation_finish, cell by cell in Python: ints stay exact
    (Pearson's three terms are Python ints), each becomes a float once."""
    K = len(tokens)
    D = int(docs_used)
    N = [int(x) for x in tokens]
    Cp = [int(x) for x in present]
    T = [[int(x) for x in row] for row in np.asarray(table)]
    out = np.full((K, K), np.nan)
    for k in range(K):
        for l in range(K):
            t = T[k][l]
            if measure in ("pmi", "npmi"):
                if Cp[k] == 0 or Cp[l] == 0:
                    continue
                if t == 0:
                    out[k, l] = -1.0 if measure == "npmi" else -math.inf
                elif measure == "npmi" and t == D:
                    out[k, l] = 1.0
                else:
                    pmi = math.log(float(D) * float(t) / (float(Cp[k]) * float(Cp[l])))
                    out[k, l] = pmi / -math.log(float(t) / float(D)) if measure == "npmi" else pmi
            elif measure == "jaccard":
                u = Cp[k] + Cp[l] - t
                if u:
                    out[k, l] = float(t) / float(u)
            elif measure == "overlap":
                u = N[k] + N[l] - t
                if u:
                    out[k, l] = float(t) / float(u)
            elif measure == "cosine":
                if T[k][k] and T[l][l]:
                    out[k, l] = float(t) / (math.sqrt(float(T[k][k])) * math.sqrt(float(T[l][l])))
            elif measure == "pearson":
                cov = D * t - N[k] * N[l]
                vk, vl = D * T[k][k] - N[k] * N[k], D * T[l][l] - N[l] * N[l]
                if vk and vl:
                    out[k, l] = float(cov) / math.sqrt(float(vk) * float(vl))
            else:
                raise ValueError(measure)
    return out


def partners(matrix, n):
    """Per row its n largest finite off-diagonal values, larger first, equal
    values by smaller id; -1 / NaN past the last."""
    matrix = np.asarray(matrix, np.float64)
    K = matrix.shape[0]
    ids = np.full((K, n), -1, np.int32)
    values = np.full((K, n), np.nan)
    for k in range(K):
        cand = [l for l in range(K) if l != k and math.isfinite(matrix[k, l])]
        cand.sort(key=lambda l: (-matrix[k, l], l))
        for i, l in enumerate(cand[:n]):
            ids[k, i] = l
            values[k, i] = matrix[k, l]
    return ids, values


def same_floats(a, b):
    """Equal bit for bit up to the kind of a NaN: the same NaN positions and
    identical values (signed infinities included) elsewhere."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
