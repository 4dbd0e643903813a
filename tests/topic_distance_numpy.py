"""numpy restatement of lda_topic_distances / lda_topic_nearest
(include/lda_mi355x.h), straight from the definitions.

    phi_k(w) = (nw[w, k] + beta) / (nwsum[k] + V beta)

per side, each with its own beta and nwsum; p = a topic of side A (a row of the
result), q = a topic of side B (a column).  The direct forms, not the
decomposed ones the device sums:

    cosine            sum p q / (sqrt(sum p^2) sqrt(sum q^2))
    hellinger         sqrt(max(0, 1 - sum sqrt(p) sqrt(q)))
    jensen_shannon    (1/2) sum p ln(p / m) + (1/2) sum q ln(q / m), m = (p + q) / 2
    kullback_leibler  sum p ln(p / q)

Everything is fp64; `rows` restricts the result to some topics of side A so
that a big shape costs seconds.
"""
import numpy as np

COSINE, HELLINGER, JS, KL = 0, 1, 2, 3
METRICS = {"cosine": COSINE, "hellinger": HELLINGER, "jensen_shannon": JS, "kullback_leibler": KL}


def phi(nw, nwsum, beta):
    """[V, K] fp64 smoothed topics, one per column."""
    nw = np.asarray(nw, dtype=np.float64)
    V = nw.shape[0]
    return (nw + beta) / (np.asarray(nwsum, dtype=np.float64)[None, :] + V * beta)


def topic_distances(nw_a, nwsum_a, beta_a, nw_b=None, nwsum_b=None, beta_b=None, metric=JS, rows=None,
                    squared_hellinger=False):
    """The [len(rows), K2] matrix (rows None: every topic of side A).  Side B
    None: side A itself.  squared_hellinger returns 1 - sum sqrt(p) sqrt(q)
    clipped at 0 instead of its root."""
    metric = METRICS.get(metric, metric)
    P = phi(nw_a, nwsum_a, beta_a)
    Q = P if nw_b is None else phi(nw_b, nwsum_b, beta_b)
    if P.shape[0] != Q.shape[0]:
        raise ValueError("the two sides differ in V")
    rows = np.arange(P.shape[1]) if rows is None else np.asarray(rows)
    out = np.zeros((len(rows), Q.shape[1]), np.float64)
    if metric == COSINE:
        qn = np.sqrt((Q * Q).sum(axis=0))
    elif metric == HELLINGER:
        sq = np.sqrt(Q)
    elif metric in (JS, KL):
        lq = np.log(Q)
    else:
        raise ValueError("unknown metric")
    for i, a in enumerate(rows):
        p = P[:, a:a + 1]                                   # [V, 1]
        if metric == COSINE:
            out[i] = (p * Q).sum(axis=0) / (np.sqrt((p * p).sum()) * qn)
        elif metric == HELLINGER:
            h2 = np.maximum(0.0, 1.0 - (np.sqrt(p) * sq).sum(axis=0))
            out[i] = h2 if squared_hellinger else np.sqrt(h2)
        elif metric == JS:
            lm = np.log(0.5 * (p + Q))
            out[i] = 0.5 * (p * (np.log(p) - lm)).sum(axis=0) + 0.5 * (Q * (lq - lm)).sum(axis=0)
        else:
            out[i] = (p * (np.log(p) - lq)).sum(axis=0)
    return out


def expected_nearest(matrix, n, metric, self_mode):
    """(topics int32 [K, n], values fp64 [K, n]) of lda_topic_nearest from a
    matrix: value ascending (cosine descending), equal values by ascending
    id, the row's own topic left out in self mode, -1 / NaN past the last
    candidate."""
    metric = METRICS.get(metric, metric)
    matrix = np.asarray(matrix, dtype=np.float64)
    K, K2 = matrix.shape
    topics = np.full((K, n), -1, np.int32)
    values = np.full((K, n), np.nan, np.float64)
    ids = np.arange(K2)
    for a in range(K):
        row = matrix[a] + 0.0                               # -0.0 orders as 0.0
        key = -row if metric == COSINE else row
        order = np.lexsort((ids, key))
        if self_mode:
            order = order[order != a]
        order = order[:n]
        topics[a, :len(order)] = order
        values[a, :len(order)] = matrix[a, order]
    return topics, values
