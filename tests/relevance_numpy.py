"""Brute-force numpy restatement of lda_relevant_words, lda_salient_words,
lda_word_rows and ParallelTopicModel.prepareVis (lda_mi355x.h),
from the dense nw [V, K] and nwsum [K].  Every expectation of test_relevance.py
and test_relevance_gpu.py comes from here.  All fp64, one rounding per
operation, with the header's expressions:

    tw[w]        = sum_k nw[w, k]                       N = sum_k nwsum[k]
    logprob(w,k) = log((nw[w,k] + beta) / (nwsum[k] + V beta))
    logtp(w)     = log(tw[w] / N)
    loglift(w,k) = logprob(w,k) - logtp(w)
    key(w,k,l)   = logprob(w,k) - (1.0 - lambda_l) * logtp(w)

numpy's log is the host libm's, the device's is not: values are compared within
a tolerance, and orders only where the restatement's own keys are further
apart than that (check_key_gaps / check_saliency_gaps)."""
import numpy as np

GAP = 1e-7


def tables(nw, nwsum, beta):
    """(tw int64 [V], N, logprob [V, K], logtp [V]); logprob is NaN where
    nw = 0 (no candidate), logtp where tw = 0."""
    nw = np.asarray(nw, np.int64)
    V, K = nw.shape
    tw = nw.sum(axis=1)
    N = int(np.asarray(nwsum, np.int64).sum())
    vbeta = float(V) * float(beta)
    with np.errstate(divide="ignore", invalid="ignore"):
        logprob = np.log((nw.astype(np.float64) + float(beta)) / (np.asarray(nwsum, np.float64)[None, :] + vbeta))
        logtp = np.log(tw.astype(np.float64) / float(N))
    logprob = np.where(nw > 0, logprob, np.nan)
    logtp = np.where(tw > 0, logtp, np.nan)
    return tw, N, logprob, logtp


def keys(logprob_col, logtp, lam):
    """key(w, k, lambda) of one topic's column: one product, one difference."""
    m = 1.0 - float(lam)
    return logprob_col - m * logtp


def expected_relevant(nw, nwsum, beta, n, lambdas):
    """(word_ids, counts int32, totals int64, logprob, loglift float64), each
    [L, K, n]: per lambda and topic the words with nw > 0 by key descending,
    equal keys by ascending id; -1 / 0 / 0 / 0.0 / 0.0 past the last."""
    nw = np.asarray(nw, np.int64)
    V, K = nw.shape
    lam = np.atleast_1d(np.asarray(lambdas, np.float64))
    tw, _, logprob, logtp = tables(nw, nwsum, beta)
    shape = (lam.size, K, n)
    ids = np.full(shape, -1, np.int32)
    cnt = np.zeros(shape, np.int32)
    tot = np.zeros(shape, np.int64)
    lp = np.zeros(shape, np.float64)
    ll = np.zeros(shape, np.float64)
    for k in range(K):
        cand = np.nonzero(nw[:, k] > 0)[0]
        for l, x in enumerate(lam):
            key = keys(logprob[cand, k], logtp[cand], x)
            best = cand[np.lexsort((cand, -key))][:n]
            m = best.size
            ids[l, k, :m] = best
            cnt[l, k, :m] = nw[best, k]
            tot[l, k, :m] = tw[best]
            lp[l, k, :m] = logprob[best, k]
            ll[l, k, :m] = logprob[best, k] - logtp[best]
    return ids, cnt, tot, lp, ll


def check_key_gaps(nw, nwsum, beta, lambdas, gap=GAP):
    """The precondition of an order comparison against the device: among a
    topic's candidates, any two keys adjacent in the order either come from
    identical (nw, tw) inputs (at lambda = 1: identical nw) or differ by more
    than `gap`.  Returns the smallest such difference; raises AssertionError
    on a fixture that breaks it."""
    nw = np.asarray(nw, np.int64)
    tw, _, logprob, logtp = tables(nw, nwsum, beta)
    smallest = np.inf
    for k in range(nw.shape[1]):
        cand = np.nonzero(nw[:, k] > 0)[0]
        for x in np.atleast_1d(np.asarray(lambdas, np.float64)):
            key = keys(logprob[cand, k], logtp[cand], x)
            o = cand[np.lexsort((cand, -key))]
            ks = np.sort(key)[::-1]
            same = nw[o[:-1], k] == nw[o[1:], k]
            if x != 1.0:
                same &= tw[o[:-1]] == tw[o[1:]]
            d = (ks[:-1] - ks[1:])[~same]
            if d.size:
                smallest = min(smallest, float(d.min()))
                assert d.min() > gap, f"topic {k}, lambda {x}: adjacent keys {d.min():.3g} apart"
    return smallest


def distinctiveness(nw, nwsum):
    """(tw, N, dist [V]): sum over k with nw > 0 of q log(q / p_k), q = nw / tw,
    p_k = nwsum[k] / N; 0.0 for a word without tokens."""
    nw = np.asarray(nw, np.int64)
    tw = nw.sum(axis=1)
    N = int(np.asarray(nwsum, np.int64).sum())
    p = np.asarray(nwsum, np.float64) / float(N)
    dist = np.zeros(nw.shape[0], np.float64)
    for w in np.nonzero(tw > 0)[0]:
        ks = np.nonzero(nw[w] > 0)[0]
        q = nw[w, ks].astype(np.float64) / float(tw[w])
        dist[w] = float(np.sum(q * np.log(q / p[ks])))
    return tw, N, dist


def saliency(nw, nwsum):
    tw, N, dist = distinctiveness(nw, nwsum)
    return tw, (tw.astype(np.float64) / float(N)) * dist, dist


def expected_salient(nw, nwsum, n):
    """(word_ids int32 [n], totals int64, saliency, distinctiveness float64):
    the words with tw > 0 by saliency descending, equal values by ascending
    id; -1 / 0 / 0.0 / 0.0 past the last."""
    tw, sal, dist = saliency(nw, nwsum)
    cand = np.nonzero(tw > 0)[0]
    best = cand[np.lexsort((cand, -sal[cand]))][:n]
    ids = np.full(n, -1, np.int32)
    tot = np.zeros(n, np.int64)
    s = np.zeros(n, np.float64)
    d = np.zeros(n, np.float64)
    m = best.size
    ids[:m], tot[:m], s[:m], d[:m] = best, tw[best], sal[best], dist[best]
    return ids, tot, s, d


def check_saliency_gaps(nw, nwsum, n, gap=GAP):
    """Among the top n + 1 saliencies, two adjacent ones either come from
    identical rows or differ by more than `gap` relative to the larger."""
    nw = np.asarray(nw, np.int64)
    tw, sal, _ = saliency(nw, nwsum)
    cand = np.nonzero(tw > 0)[0]
    o = cand[np.lexsort((cand, -sal[cand]))][:n + 1]
    smallest = np.inf
    for a, b in zip(o[:-1], o[1:]):
        if np.array_equal(nw[a], nw[b]):
            continue
        rel = (sal[a] - sal[b]) / abs(sal[a])
        smallest = min(smallest, float(rel))
        assert rel > gap, f"saliency of words {a} and {b} {rel:.3g} apart (relative)"
    return smallest


def classical_mds(dist):
    """(x, y): B = -1/2 J D^2 J, eigh, the two largest eigenvalues' vectors
    times sqrt(max(eigenvalue, 0)); each axis's entry of largest magnitude
    (lowest index on a tie) positive; K = 1: zeros, K = 2: y zeros."""
    D = np.asarray(dist, np.float64)
    K = D.shape[0]
    out = [np.zeros(K), np.zeros(K)]
    if K == 1:
        return out[0], out[1]
    J = np.eye(K) - np.ones((K, K)) / K
    vals, vecs = np.linalg.eigh(-0.5 * J.dot(D ** 2).dot(J))
    top = np.argsort(vals)[::-1]
    for axis in range(min(2, K - 1)):
        j = top[axis]
        a = vecs[:, j] * np.sqrt(max(vals[j], 0.0))
        big = np.abs(a)
        if a[np.nonzero(big == big.max())[0][0]] < 0:
            a = -a
        out[axis] = a
    return out[0], out[1]


def vis_lambdas(step):
    lam = [min(1.0, i * step) for i in range(int(np.floor(1.0 / step + 1e-9)) + 1)]
    if lam[-1] < 1.0:
        lam.append(1.0)
    return np.array(lam, np.float64)


def pairwise(x, y):
    p = np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], axis=1)
    return np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))


def expected_vis(nw, nwsum, beta, R, step, js, names=None):
    """prepareVis' dict from the dense table and the K x K Jensen-Shannon
    matrix `js`.  names[w]: the term's text (None: the id)."""
    nw = np.asarray(nw, np.int64)
    V, K = nw.shape
    nwsum = np.asarray(nwsum, np.int64)
    N = int(nwsum.sum())
    tw = nw.sum(axis=1)
    term = (lambda w: str(int(w))) if names is None else (lambda w: str(names[int(w)]))
    order = sorted(range(K), key=lambda k: (-int(nwsum[k]), k))
    rank = {k: i + 1 for i, k in enumerate(order)}
    x, y = classical_mds(js)
    lam = vis_lambdas(step)
    ids, cnt, tot, lp, ll = expected_relevant(nw, nwsum, beta, R, lam)
    sal_ids, sal_tot, _, _ = expected_salient(nw, nwsum, R)
    tinfo = {"Term": [], "Category": [], "Freq": [], "Total": [], "logprob": [], "loglift": []}
    used = set()
    for i, w in enumerate(sal_ids):
        if w < 0:
            continue
        used.add(int(w))
        row = (term(w), "Default", int(sal_tot[i]), int(sal_tot[i]), float(R - i), float(R - i))
        for key, v in zip(tinfo, row):
            tinfo[key].append(v)
    for k in order:
        seen = []
        for l in range(lam.size):
            for i in range(R):
                w = int(ids[l, k, i])
                if w >= 0 and w not in seen:
                    seen.append(w)
                    row = (term(w), "Topic%d" % rank[k], int(nw[w, k]), int(tw[w]), float(lp[l, k, i]),
                           float(ll[l, k, i]))
                    for key, v in zip(tinfo, row):
                        tinfo[key].append(v)
        used.update(seen)
    table = {"Term": [], "Topic": [], "Freq": []}
    for w in sorted(used):
        for k in order:
            if nw[w, k] >= 1:
                table["Term"].append(term(w))
                table["Topic"].append(rank[k])
                table["Freq"].append(float(nw[w, k]) / float(tw[w]))
    return {
        "mdsDat": {"x": [float(x[k]) for k in order], "y": [float(y[k]) for k in order],
                   "topics": list(range(1, K + 1)), "cluster": [1] * K,
                   "Freq": [100.0 * float(nwsum[k]) / float(N) for k in order]},
        "tinfo": tinfo,
        "token.table": table,
        "R": R,
        "lambda.step": float(step),
        "plot.opts": {"xlab": "PC1", "ylab": "PC2"},
        "topic.order": [k + 1 for k in order],
    }


def fixture(V, K, tokens, seed=20261021):
    """The seeded recipe of the GPU tests: word ~ p proportional to
    1 / (1 + id), z = word mod K with probability 0.7, else uniform.  Returns
    (words int32, z int32)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / (1.0 + np.arange(V))
    words = rng.choice(V, size=tokens, p=p / p.sum()).astype(np.int32)
    z = np.where(rng.random(tokens) < 0.7, words % K, rng.integers(0, K, tokens)).astype(np.int32)
    return words, z


def counts_of(words, z, V, K):
    nw = np.zeros((V, K), np.int64)
    np.add.at(nw, (words, z), 1)
    return nw, nw.sum(axis=0)
