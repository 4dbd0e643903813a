"""numpy restatement of lda_doc_distances / lda_doc_nearest / lda_doc_neighbors
(lda_mi355x.h): the rows from doc_counts and alpha, the three
metrics by the header's expressions with plain numpy sums, the selection by
np.lexsort((ids, values)).  It is the yardstick of test_doc_neighbors_gpu.py
and is itself checked on a hand-worked example in test_doc_neighbors.py."""
import numpy as np

COSINE, HELLINGER, JS = 0, 1, 2
METRICS = {"cosine": COSINE, "hellinger": HELLINGER, "jensen_shannon": JS}


def _metric(metric) -> int:
    return METRICS[metric] if isinstance(metric, str) else int(metric)


def rows_from_counts(counts, alpha) -> np.ndarray:
    """p[d, k] = (n_dk + alpha_k) / (L_d + A), L_d the row's total, A the sum
    of alpha added in topic order."""
    c = np.atleast_2d(np.asarray(counts, np.int64))
    a = np.asarray(alpha, np.float64)
    A = 0.0
    for x in a:
        A += float(x)
    return (c.astype(np.float64) + a[None, :]) / (c.sum(axis=1).astype(np.float64) + A)[:, None]


def _xlogx(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > 0, x * np.log(np.where(x > 0, x, 1.0)), 0.0)


def distances(q, p, metric, squared_hellinger: bool = False) -> np.ndarray:
    """values[i, j] between query row q[i] and candidate row p[j]."""
    m = _metric(metric)
    q = np.atleast_2d(np.asarray(q, np.float64))
    p = np.atleast_2d(np.asarray(p, np.float64))
    out = np.zeros((len(q), len(p)), np.float64)
    for i, qi in enumerate(q):
        if m == COSINE:
            S = (p * qi[None, :]).sum(axis=1)
            out[i] = S / np.sqrt((p * p).sum(axis=1) * (qi * qi).sum())
        elif m == HELLINGER:
            S = ((np.sqrt(p) - np.sqrt(qi)[None, :]) ** 2).sum(axis=1)
            h2 = np.minimum(1.0, S / 2.0)
            out[i] = h2 if squared_hellinger else np.sqrt(h2)
        elif m == JS:
            s = p + qi[None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                S = np.where(s > 0, s * np.log(np.where(s > 0, s, 2.0) / 2.0), 0.0).sum(axis=1)
            out[i] = np.maximum(0.0, 0.5 * ((_xlogx(p).sum(axis=1) + _xlogx(qi).sum()) - S))
        else:
            raise ValueError(metric)
    return out + 0.0


def nearest(values, n, metric, ids=None, lengths=None, min_tokens=1, skip=None):
    """(doc ids int64 [Q, n], values fp64 [Q, n]) selected from a [Q, M] matrix
    of values: value ascending (cosine: descending), equal values by ascending
    id; candidates need lengths[j] >= min_tokens and ids[j] != skip[q]; -1 /
    NaN past the last candidate.  The values returned are the matrix's bits."""
    m = _metric(metric)
    v = np.atleast_2d(np.asarray(values, np.float64))
    Q, M = v.shape
    ids = np.arange(M, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    ok = np.ones(M, bool) if lengths is None else np.asarray(lengths) >= min_tokens
    out_ids = np.full((Q, n), -1, np.int64)
    out_vals = np.full((Q, n), np.nan, np.float64)
    for q in range(Q):
        keep = ok if skip is None else ok & (ids != int(skip[q]))
        cid, cv = ids[keep], v[q][keep]
        order = np.lexsort((cid, -cv if m == COSINE else cv))[:n]
        out_ids[q, :len(order)] = cid[order]
        out_vals[q, :len(order)] = cv[order]
    return out_ids, out_vals
