#!/usr/bin/env python3
"""Latency of the nearest documents (run by hand on the GPU; not
bench.py).  Two routes to the 10 nearest training documents of Q training
documents, per metric:

  (a) what there was before lda_doc_neighbors:
      cosine          docCounts() -- the D x K table to the host -- then theta
                      of the queries and topDocuments(theta, 11): every score
                      through the host, the best kept there; the query itself
                      (rank 0) dropped;
      Hellinger       docCounts(), then numpy: one BLAS product of sqrt(theta),
                      1 - BC, argpartition and a sort of the best;
      Jensen-Shannon  docCounts(), then numpy row by row (a logarithm per
                      topic and pair); timed on --rows queries and scaled by
                      Q / rows where the whole would take minutes
                      (`a_extrapolated`: true);
  (b) ParallelTopicModel.documentNeighbors(10, docs=queries): rows built and
      neighbours selected on the device, 16 Q n bytes back.

Inputs:
  small  the reference's own scale: D = 2000, K = 500, every document a query;
  big    D = 1e5, K = 512, 1024 query documents.
Medians of --reps calls after a warm one, the routes alternating, the host
clock around calls that end in a device wait.  Recorded per metric and shape:
a / b, the bytes each route brings to the host, the largest disagreement of the
routes' values (Hellinger by its square), the share of equal ids, and
b_not_slower_than_a; and the pair terms per second of route (b)'s whole call
(Q D K over its time: rows, pairs and selection together).  Writes one JSON
line to profiles/doc_neighbors/latency.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

METRICS = ("cosine", "hellinger", "jensen_shannon")
N = 10


def _alternate(fns, reps):
    """Median and minimum wall time of each fn, called in turn reps times
    after one warm call each (code objects, scratch growth)."""
    for fn in fns:
        fn()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            t[i].append(time.perf_counter() - t0)
    return [(float(np.median(x)), float(np.min(x))) for x in t]


def _theta(nd, alpha):
    return (nd.astype(np.float64) + alpha[None, :]) / (nd.sum(axis=1, dtype=np.float64) + alpha.sum())[:, None]


def _best(values, queries, largest):
    """(ids, values) [Q, N] of each row's best N columns, the query's own
    column left out; by value, ties by id."""
    v = values.copy()
    v[np.arange(len(queries)), queries] = -np.inf if largest else np.inf
    key = -v if largest else v
    part = np.argpartition(key, N, axis=1)[:, :N + 1]
    pk = np.take_along_axis(key, part, axis=1)
    order = np.lexsort((part, pk), axis=1)[:, :N]
    ids = np.take_along_axis(part, order, axis=1)
    return ids, np.take_along_axis(v, ids, axis=1)


def route_a(m, metric, queries, rows=None):
    """Route (a) for the first `rows` queries (None: all)."""
    q = queries if rows is None else queries[:rows]
    theta = _theta(m.docCounts(), m.alpha)
    if metric == "cosine":
        ids, vals = m.topDocuments(theta[q], N + 1, "cosine")
        keep = ids != q[:, None]
        sel = np.argsort(~keep, axis=1, kind="stable")[:, :N]      # the first N that are not the query itself
        return np.take_along_axis(ids, sel, axis=1), np.take_along_axis(vals, sel, axis=1)
    if metric == "hellinger":
        r = np.sqrt(theta)
        h2 = np.maximum(0.0, 1.0 - r[q] @ r.T)
        ids, v = _best(h2, q, False)
        return ids, np.sqrt(v)
    ent = np.einsum("dk,dk->d", theta, np.log(theta))
    js = np.empty((len(q), len(theta)), np.float64)
    for i, d in enumerate(q):
        s = theta[d][None, :] + theta
        js[i] = np.maximum(0.0, 0.5 * (ent[d] + ent - np.einsum("dk,dk->d", s, np.log(0.5 * s))))
    return _best(js, q, False)


def measure(m, queries, reps, rows):
    K, D, Q = m.numTopics, len(m.data), len(queries)
    rec = {"K": K, "docs": D, "queries": Q, "n": N, "reps": reps, "shards": m.numShards()}
    for metric in METRICS:
        part = rows if metric == "jensen_shannon" and Q * D * K > 1e9 else None   # minutes a call on the host
        a_ids, a_vals = route_a(m, metric, queries, part)
        b_ids, b_vals = m.documentNeighbors(N, docs=queries, metric=metric)
        n = len(a_ids)
        pa, pb = (a_vals ** 2, b_vals[:n] ** 2) if metric == "hellinger" else (a_vals, b_vals[:n])
        err = float(np.max(np.abs(pa - pb)))
        fns = [lambda: route_a(m, metric, queries, part), lambda: m.documentNeighbors(N, docs=queries, metric=metric)]
        (ta, ta_min), (tb, tb_min) = _alternate(fns, reps)
        scale = 1.0 if part is None else Q / part
        a_bytes = 4 * D * K + (8 * Q * D if metric == "cosine" else 0)
        rec[metric] = {"bytes_to_host_route_a": a_bytes, "bytes_to_host_route_b": 16 * Q * N,
                       "max_abs_difference": err, "ids_equal_share": float(np.mean(a_ids == b_ids[:n])),
                       "a_s": ta * scale, "a_min_s": ta_min * scale, "a_extrapolated": part is not None,
                       "a_queries_timed": n, "b_s": tb, "b_min_s": tb_min, "a_over_b": ta * scale / tb,
                       "b_not_slower_than_a": tb <= ta * scale, "b_pair_terms_per_s": Q * D * K / tb}
        print(f"D={D} K={K} {metric}: {rec[metric]}", file=sys.stderr, flush=True)
    rec["b_not_slower_than_a"] = all(rec[x]["b_not_slower_than_a"] for x in METRICS)
    return rec


def model(D, K, V, L, iters, seed):
    from ldagibbssampling_amd import topic_model as tm
    from ldagibbssampling_amd.corpus import Corpus
    rng = np.random.default_rng(seed)
    lens = rng.integers(max(1, L // 2), L + L // 2 + 1, D)
    off = np.zeros(D + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    # documents of 8 "own" word bands each, so that the trained rows differ
    band = rng.integers(0, 64, (D, 8))
    pick = np.repeat(np.arange(D), lens)
    words = (band[pick, rng.integers(0, 8, len(pick))] * (V // 64) + rng.integers(0, V // 64, len(pick))).astype(np.int32)
    m = tm.ParallelTopicModel(K, 0.1 * K, 0.01)
    m.setRandomSeed(seed)
    m.setTopicDisplay(0, 0)
    m.setNumIterations(iters)
    m.setOptimizeInterval(0)
    m.setDevices([0])
    m.addInstances(tm.InstanceList.fromCorpus(Corpus(off, words, V)))
    m.estimate()
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--big", action="store_true", help="the big input only")
    ap.add_argument("--small", action="store_true", help="the small input only")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=16, help="queries of Jensen-Shannon's route (a) where it is extrapolated")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "doc_neighbors", "latency.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("doc_neighbors_latency.py needs an MI355X")
    rec = {"tool": "doc_neighbors_latency", "device": torch.cuda.get_device_name(0)}
    shapes = (("small", dict(D=2000, K=500, V=6400, L=80), None), ("big", dict(D=100_000, K=512, V=64_000, L=100), 1024))
    for name, shape, nq in shapes:
        if (name == "small" and args.big) or (name == "big" and args.small):
            continue
        m = model(iters=args.iters, seed=20261021, **shape)
        D = shape["D"]
        queries = np.arange(D) if nq is None else np.sort(np.random.default_rng(1).choice(D, nq, replace=False))
        rec[name] = measure(m, queries.astype(np.int64), args.reps, args.rows)
        m.close()
    rec["b_not_slower_than_a"] = all(rec[x]["b_not_slower_than_a"] for x in ("small", "big") if x in rec)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
