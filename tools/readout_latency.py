#!/usr/bin/env python3
"""Latency of the model readouts (run by hand on the GPU; not bench.py).  Two
routes to the same arrays, checked equal before they are timed:

  top words, per topic the n = 7 (and 64) heaviest words
    (a) the route before lda_top_words: counts() -- the V x K table to the
        host -- then a host selection (numpy: np.partition of the unique keys
        count << 32 | 0xFFFFFFFF - word per topic, then a sort of the n kept;
        cheaper than the stable_sort of every nonzero word that
        displayTopWords ran, so (a) is flattered, not (b));
    (b) GibbsSampler.top_words(n): selected on the device, 8 K n bytes back.
  document topics, the 10 heaviest topics of every document
    (a) the route before lda_doc_top_topics: z() -- every topic assignment to
        the host -- then counts per document and a selection per document
        (numpy, chunks of documents);
    (b) GibbsSampler.doc_top_topics(10).

Inputs:
  small  the training corpus of tests/test_perplexity.py (_corpus_split(100)):
         1980 documents, V = 3000, K = 100, after --sweeps sweeps;
  big    a synthetic shard, V = 1e5, K = 512, 1e5 documents of 100 tokens
         (uniformly random word ids; each document draws from 8 topics).
The document route is timed on the big input (1e5 documents) only.
Medians of --reps calls, the routes alternating, the host clock around calls
that end in a device wait.  Writes one JSON line to
profiles/readout/readout_latency.json.
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


def host_top_words(nw, n):
    """(ids[K, n], counts[K, n]) from the V x K table on the host."""
    V, K = nw.shape
    keys = (nw.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(V, dtype=np.uint64))[:, None]
    keys[nw <= 0] = 0
    m = min(n, V)
    top = np.partition(keys, V - m, axis=0)[V - m:]
    top = np.sort(top, axis=0)[::-1].T                      # [K, m] descending
    ids = np.full((K, n), -1, np.int32)
    cnt = np.zeros((K, n), np.int32)
    ids[:, :m] = np.where(top > 0, (np.uint64(0xFFFFFFFF) - (top & np.uint64(0xFFFFFFFF))).astype(np.int64), -1)
    cnt[:, :m] = (top >> np.uint64(32)).astype(np.int32)
    return ids, cnt


def host_doc_top_topics(z, doc_off, alpha, m, chunk=8192):
    """(topics[D, m], counts[D, m]) from z on the host: the weights of
    documentTopics, weight descending, equal weights by ascending topic."""
    D, K = len(doc_off) - 1, len(alpha)
    A = 0.0
    for a in alpha:
        A += float(a)
    lens = np.diff(doc_off)
    topics = np.zeros((D, m), np.int32)
    counts = np.zeros((D, m), np.int32)
    for d0 in range(0, D, chunk):
        d1 = min(D, d0 + chunk)
        t0, t1 = int(doc_off[d0]), int(doc_off[d1])
        doc = np.repeat(np.arange(d1 - d0), lens[d0:d1])
        nd = np.bincount(doc * K + z[t0:t1], minlength=(d1 - d0) * K).reshape(d1 - d0, K)
        w = (alpha[None, :] + nd) / (lens[d0:d1].astype(np.float64)[:, None] + A)
        # the m-th largest weight per row, then everything at or above it in (weight desc, id asc) order
        kth = np.partition(w, K - m, axis=1)[:, K - m]
        for j in range(d1 - d0):
            cand = np.flatnonzero(w[j] >= kth[j])
            order = cand[np.lexsort((cand, -w[j, cand]))][:m]
            topics[d0 + j] = order
            counts[d0 + j] = nd[j, order]
    return topics, counts


def top_words_part(g, reps):
    out = {"K": g.K, "Kp": g.Kp, "V": g.V, "table_bytes": 4 * g.V * g.Kp, "counts_bytes_to_host_route_a": 4 * g.V * g.K,
           "reps": reps}
    for n in (7, 64):
        route_a = lambda: host_top_words(g.counts()[0], n)
        route_b = lambda: g.top_words(n)
        a, b = route_a(), route_b()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the routes disagree"
        copy_only = lambda: g.counts()[0]
        (ta, ta_min), (tb, tb_min), (tc, tc_min) = _alternate([route_a, route_b, copy_only], reps)
        out[f"n{n}"] = {"a_counts_host_select_s": ta, "a_min_s": ta_min, "b_top_words_s": tb, "b_min_s": tb_min,
                        "a_counts_copy_only_s": tc, "result_bytes_to_host_route_b": 8 * g.K * n,
                        "b_not_slower_than_a": tb <= ta, "a_over_b": ta / tb}
    return out


def doc_topics_part(g, doc_off, reps, m=10):
    route_a = lambda: host_doc_top_topics(g.z(), doc_off, g.alpha, m)
    route_b = lambda: g.doc_top_topics(m)
    a, b = route_a(), route_b()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the routes disagree"
    copy_only = lambda: g.z()
    (ta, ta_min), (tb, tb_min), (tc, tc_min) = _alternate([route_a, route_b, copy_only], reps)
    return {"docs": g.D, "tokens": g.N, "K": g.K, "m": m, "z_bytes_to_host_route_a": 4 * g.N,
            "result_bytes_to_host_route_b": 8 * g.D * m, "reps": reps, "a_z_host_select_s": ta, "a_min_s": ta_min,
            "b_doc_top_topics_s": tb, "b_min_s": tb_min, "a_z_copy_only_s": tc, "b_not_slower_than_a": tb <= ta,
            "a_over_b": ta / tb}


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
        out = {"top_words": top_words_part(g, args.reps)}
    out["train"] = {"docs": train.num_docs, "tokens": train.num_tokens, "sweeps": args.sweeps}
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
        out = {"top_words": top_words_part(g, args.reps), "document_topics": doc_topics_part(g, off, args.reps)}
    out["train"] = {"docs": D, "tokens": D * L}
    return out


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readout", "readout_latency.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("readout_latency.py needs an MI355X")
    rec = {"tool": "readout_latency", "device": torch.cuda.get_device_name(0)}
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
