#!/usr/bin/env python3
"""Latency of the top documents per topic (run by hand on the GPU; not
bench.py).  Two routes to the same arrays, compared equal before anything is
timed:

  (a) the route before lda_topic_top_docs: z() -- every topic assignment to
      the host -- then the numpy restatement: the D x K counts (np.bincount,
      faster than the np.add.at of tests/topic_docs_numpy.py, so (a) is
      flattered, not (b)), the weights (n_dk + s) / (L_d + K s) and per topic
      np.lexsort((ids, -w)) over the candidates, cut at n;
  (b) GibbsSampler.topic_top_docs(n, s): selected on the device, 16 K n bytes
      back.

Inputs:
  small  the training corpus of tests/test_perplexity.py (_corpus_split(100)):
         1980 documents, V = 3000, K = 100, after --sweeps sweeps;
  big    a synthetic shard, V = 1e5, K = 512, 1e5 documents of 100 tokens
         (uniformly random word ids; each document draws from 8 topics).
Both at n = 10 and n = 100, smoothing 10 (printTopicDocuments' default).
Medians of --reps calls, the routes alternating, the host clock around calls
that end in a device wait; the copy of z alone is timed beside them.  Writes
one JSON line to profiles/topic_docs/latency.json.
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

SMOOTHING = 10.0


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


def host_topic_docs(z, doc_off, K, n, smoothing, min_tokens=1):
    """(docs[K, n] int64, counts[K, n], lengths[K, n] int32) from z on the host."""
    D = len(doc_off) - 1
    lens = np.diff(doc_off)
    doc = np.repeat(np.arange(D, dtype=np.int64), lens)
    nd = np.bincount(doc * K + z, minlength=D * K).reshape(D, K)
    ks = float(K) * float(smoothing)
    denom = lens.astype(np.float64) + ks
    docs = np.full((K, n), -1, np.int64)
    cnt = np.zeros((K, n), np.int32)
    ln = np.zeros((K, n), np.int32)
    ok = lens >= min_tokens
    for k in range(K):
        col = nd[:, k]
        ids = np.flatnonzero((col > 0) & ok)
        if len(ids) == 0:
            continue
        w = (col[ids].astype(np.float64) + float(smoothing)) / denom[ids]
        order = ids[np.lexsort((ids, -w))][:n]
        docs[k, :len(order)] = order
        cnt[k, :len(order)] = col[order]
        ln[k, :len(order)] = lens[order]
    return docs, cnt, ln


def part(g, doc_off, reps):
    out = {"docs": g.D, "tokens": g.N, "K": g.K, "Kp": g.Kp, "smoothing": SMOOTHING, "reps": reps,
           "z_bytes_to_host_route_a": 4 * g.N}
    for n in (10, 100):
        route_a = lambda: host_topic_docs(g.z(), doc_off, g.K, n, SMOOTHING)
        route_b = lambda: g.topic_top_docs(n, SMOOTHING)
        a, b = route_a(), route_b()
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the routes disagree"
        copy_only = lambda: g.z()
        (ta, ta_min), (tb, tb_min), (tc, tc_min) = _alternate([route_a, route_b, copy_only], reps)
        out[f"n{n}"] = {"a_z_host_select_s": ta, "a_min_s": ta_min, "b_topic_top_docs_s": tb, "b_min_s": tb_min,
                        "a_z_copy_only_s": tc, "a_copy_share": tc / ta, "result_bytes_to_host_route_b": 16 * g.K * n,
                        "b_not_slower_than_a": tb <= ta, "a_over_b": ta / tb}
    return out


def small_part(args):
    from ldagibbssampling_amd.corpus import synthetic_lda
    from ldagibbssampling_amd.sampler import GibbsSampler
    K = 100
    c = synthetic_lda(num_docs=2200, num_types=3000, num_topics=K, doc_len=None, mean_len=80, min_len=10,
                      max_len=300, seed=20261015, k_true=min(K, 50))
    perm = np.random.default_rng(0).permutation(c.num_docs)
    train = c.subset(np.sort(perm[c.num_docs // 10:]))
    with GibbsSampler(K, c.num_types, train.doc_off, train.words, np.full(K, 10.0 / K), 0.01, seed=1) as g:
        g.sweep(args.sweeps)
        out = part(g, train.doc_off, args.reps)
    out["sweeps"] = args.sweeps
    return out


def big_part(args):
    from ldagibbssampling_amd.sampler import GibbsSampler
    V, K, L, D = args.big_types, args.big_topics, args.big_len, args.big_docs
    rng = np.random.default_rng(5)
    off = np.arange(D + 1, dtype=np.int64) * L
    words = rng.integers(0, V, D * L, dtype=np.int32)
    own = rng.integers(0, K, (D, 8), dtype=np.int32)
    z = np.take_along_axis(own, rng.integers(0, 8, (D, L)), axis=1).reshape(-1).astype(np.int32)
    with GibbsSampler(K, V, off, words, np.full(K, 0.1), 0.01, seed=1, z_init=z) as g:
        g.apply()
        return part(g, off, args.reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--big", action="store_true", help="the big input only")
    ap.add_argument("--small", action="store_true", help="the small input only")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--big-types", type=int, default=100_000)
    ap.add_argument("--big-topics", type=int, default=512)
    ap.add_argument("--big-len", type=int, default=100)
    ap.add_argument("--big-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topic_docs", "latency.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("topic_docs_latency.py needs an MI355X")
    rec = {"tool": "topic_docs_latency", "device": torch.cuda.get_device_name(0)}
    if not args.big:
        rec["small"] = small_part(args)
    if not args.small:
        rec["big"] = big_part(args)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
