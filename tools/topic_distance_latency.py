#!/usr/bin/env python3
"""Latency of the topic distances (run by hand on the GPU; not
bench.py).  Two routes to the same K x K matrix of a model against itself,
checked to agree within 1e-9 before they are timed:

  (a) the only route before lda_topic_distances: counts() -- the V x K table
      to the host -- then numpy in fp64: phi, and per metric the fastest host
      form there is -- cosine, Hellinger and Kullback-Leibler are one BLAS
      product of transformed tables (P^T Q, sqrt(P)^T sqrt(Q), P^T ln Q);
      Jensen-Shannon has no such form (a logarithm per word and pair) and goes
      row by row;
  (b) GibbsSampler.topic_distances(metric): computed on the device, 8 K^2
      bytes back.

Inputs:
  small  V = 3000, K = 100: a synthetic LDA corpus of 1980 documents after
         --sweeps sweeps;
  big    V = 1e5, K = 512: a synthetic shard of 1e5 documents of 100 tokens
         (tools/diagnostics_latency.py's).
At the big shape Jensen-Shannon's route (a) is timed on --rows rows and scaled
by K / rows (`a_extrapolated`: true); the rows it computes are the ones
compared with route (b).  Medians of --reps calls, the routes alternating, the
host clock around calls that end in a device wait.  Also timed:
nearest_topics(10) per metric (K x 10 ids and values back) and one sampler
sweep of the same shard, for scale.  Writes one JSON line to
profiles/topic_distances/latency.json.
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

METRICS = ("cosine", "hellinger", "jensen_shannon", "kullback_leibler")


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


def host_distances(nw, nwsum, beta, metric, rows=None):
    """Route (a) after counts(): the matrix (or its first `rows` rows) in fp64."""
    V, K = nw.shape
    P = (nw.astype(np.float64) + beta) / (nwsum.astype(np.float64)[None, :] + V * beta)
    A = P if rows is None else P[:, :rows]
    if metric == "cosine":
        norm = np.sqrt(np.einsum("wk,wk->k", P, P))
        return (A.T @ P) / (norm[:A.shape[1], None] * norm[None, :])
    if metric == "hellinger":
        R = np.sqrt(P)
        return np.sqrt(np.maximum(0.0, 1.0 - R[:, :A.shape[1]].T @ R))
    L = np.log(P)
    H = np.einsum("wk,wk->k", P, L)                                   # sum p ln p per topic
    if metric == "kullback_leibler":
        return H[:A.shape[1], None] - A.T @ L
    out = np.empty((A.shape[1], K), np.float64)
    for a in range(A.shape[1]):                                       # Jensen-Shannon: no product form
        S = P[:, a:a + 1] + P
        out[a] = 0.5 * (H[a] + H - np.einsum("wk,wk->k", S, np.log(0.5 * S)))
    return out


def measure(g, reps, rows):
    K, V = g.K, g.V
    rec = {"K": K, "V": V, "docs": g.D, "tokens": g.N, "reps": reps}

    def sweep():
        g.sweep(1)
        g.synchronize()      # lda_sweep returns when the sweep is enqueued

    (ts, ts_min), (tc, _) = _alternate([sweep, lambda: g.counts()], reps)
    rec.update(sweep_s=ts, sweep_min_s=ts_min, counts_copy_s=tc)
    heavy = K * K * V > 1e9
    for metric in METRICS:
        part = rows if heavy and metric == "jensen_shannon" else None
        a = host_distances(*g.counts()[:2], g.beta, metric, part)
        b = g.topic_distances(metric)
        n = a.shape[0]
        # Hellinger by its square: the root magnifies the rounding of 1 - sum near 0
        pa, pb = (a * a, b[:n] * b[:n]) if metric == "hellinger" else (a, b[:n])
        off = ~np.eye(n, K, dtype=bool)      # the device sets the diagonal; the host sums it
        err = float(np.max(np.abs(pa - pb)[off]))
        assert err <= 1e-9, f"the routes disagree: {metric} by {err:.3e}"
        fns = [lambda: host_distances(*g.counts()[:2], g.beta, metric, part), lambda: g.topic_distances(metric),
               lambda: g.nearest_topics(10, metric)]
        (ta, ta_min), (tb, tb_min), (tn, tn_min) = _alternate(fns, reps)
        scale = 1.0 if part is None else K / part
        rec[metric] = {"bytes_to_host_route_a": 4 * V * K + 4 * K, "bytes_to_host_route_b": 8 * K * K,
                       "bytes_to_host_nearest_10": 12 * K * 10, "max_abs_difference": err,
                       "a_host_numpy_s": ta * scale, "a_min_s": ta_min * scale, "a_extrapolated": part is not None,
                       "a_rows_timed": n, "b_device_s": tb, "b_min_s": tb_min,
                       "b_not_slower_than_a": tb <= ta * scale, "a_over_b": ta * scale / tb,
                       "nearest_10_s": tn, "nearest_10_min_s": tn_min, "b_over_sweep": tb / ts}
    rec["b_not_slower_than_a"] = all(rec[m]["b_not_slower_than_a"] for m in METRICS)
    return rec


def small_shard(args):
    from ldagibbssampling_amd.corpus import synthetic_lda
    from ldagibbssampling_amd.sampler import GibbsSampler
    K = 100
    c = synthetic_lda(num_docs=2200, num_types=3000, num_topics=K, doc_len=None, mean_len=80, min_len=10,
                      max_len=300, seed=20261015, k_true=min(K, 50))
    perm = np.random.default_rng(0).permutation(c.num_docs)
    train = c.subset(np.sort(perm[c.num_docs // 10:]))
    g = GibbsSampler(K, c.num_types, train.doc_off, train.words, np.full(K, 10.0 / K), 0.01, seed=1)
    g.sweep(args.sweeps)
    return g


def big_shard(args):
    from ldagibbssampling_amd.sampler import GibbsSampler
    V, K, L, D = args.big_types, args.big_topics, args.big_len, args.big_docs
    rng = np.random.default_rng(5)
    off = np.arange(D + 1, dtype=np.int64) * L
    words = rng.integers(0, V, D * L, dtype=np.int32)
    own = rng.integers(0, K, (D, 8), dtype=np.int32)
    z = np.take_along_axis(own, rng.integers(0, 8, (D, L)), axis=1).reshape(-1).astype(np.int32)
    g = GibbsSampler(K, V, off, words, np.full(K, 0.1), 0.01, seed=1, z_init=z)
    g.apply()
    g.sweep(2)
    return g


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--big", action="store_true", help="the big input only")
    ap.add_argument("--small", action="store_true", help="the small input only")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=8, help="rows of Jensen-Shannon's route (a) at the big shape")
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--big-types", type=int, default=100_000)
    ap.add_argument("--big-topics", type=int, default=512)
    ap.add_argument("--big-len", type=int, default=100)
    ap.add_argument("--big-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topic_distances", "latency.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("topic_distance_latency.py needs an MI355X")
    rec = {"tool": "topic_distance_latency", "device": torch.cuda.get_device_name(0)}
    for name, make in (("small", small_shard), ("big", big_shard)):
        if (name == "small" and args.big) or (name == "big" and args.small):
            continue
        g = make(args)
        rec[name] = measure(g, args.reps, args.rows)
        g.close()
    if "big" in rec:
        rec["b_not_slower_than_a"] = rec["big"]["b_not_slower_than_a"]
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
