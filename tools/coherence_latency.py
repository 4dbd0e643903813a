#!/usr/bin/env python3
"""Latency of the co-occurrence counts behind reference-corpus coherence (run
by hand on the GPU; not bench.py).  Two routes to the same integer triangles
for each topic's n = 10 top words over the shard's own corpus, checked equal
before they are timed, in document mode (window 0) and in windows of 10:

  (a) the host: the corpus, numpy and scipy.sparse -- a sparse (unit x listed
      word) presence matrix (a token of a listed word at position p marks the
      window starts [p - W + 1, p] of its document), its Gram matrix, and the
      lists' cells gathered from it;
  (b) GibbsSampler.word_cooccurrences(ids, window): counted on the device,
      8 K n (n + 1) / 2 bytes back.

Inputs:
  small  the training corpus of tests/test_perplexity.py (_corpus_split(100)):
         1980 documents, V = 3000, K = 100, after --sweeps sweeps;
  big    a synthetic shard, V = 1e5, K = 512, 1e5 documents of 200 tokens
         (uniformly random word ids; each document draws from 8 topics).
Medians of --reps calls, the routes alternating, the host clock around calls
that end in a device wait.  Route (a) is first timed on a tenth of the
documents; if ten times that exceeds a minute the record keeps that figure
times ten and marks it extrapolated (its result is then checked against route
(b) on the same tenth, passed from the host).  No ratio is fixed in advance:
the record carries both times and b_not_slower_than_a.  Writes one JSON line to
profiles/coherence/latency.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COOC_LDS = 64 * 1024       # lda_kernels.h: COOC_LDS_BYTES
COOC_WAVES = 4             # lda_kernels.h


def cooc_groups(K, n):
    gt = min(K, COOC_LDS // (8 * COOC_WAVES * (n + 1) + 4 * (n * (n + 1) // 2)))
    return -(-K // gt)


def host_cooc(doc_off, words, ids, window):
    """(cooc[K, n (n + 1) / 2] int64, units) on the host."""
    K, n = ids.shape
    off = np.asarray(doc_off, np.int64) - int(doc_off[0])
    lens = np.diff(off)
    per_doc = np.where(lens > 0, 1 if window == 0 else np.maximum(1, lens - window + 1), 0)
    first = np.zeros(len(lens) + 1, np.int64)          # a document's first unit
    np.cumsum(per_doc, out=first[1:])
    units = int(first[-1])
    listed = np.unique(ids[ids >= 0])
    col = np.full(int(max(words.max(initial=0), listed.max(initial=0))) + 2, -1, np.int64)
    col[listed] = np.arange(len(listed))
    c = col[words]                                     # -1 -> the last cell, which stays -1
    tok = np.flatnonzero(c >= 0)
    doc = np.searchsorted(off, tok, side="right") - 1
    if window == 0:
        rows, cols = first[doc], c[tok]
    else:
        pos = tok - off[doc]
        s = pos[:, None] - np.arange(window)[None, :]  # the starts whose window holds the token
        ok = (s >= 0) & (s < per_doc[doc][:, None])
        rows = (first[doc][:, None] + s)[ok]
        cols = np.broadcast_to(c[tok][:, None], s.shape)[ok]
    P = sp.csr_matrix((np.ones(len(rows), np.int64), (rows, cols)), shape=(units, len(listed)))
    P.data[:] = 1                                      # duplicates were summed: presence
    G = np.asarray((P.T @ P).todense())
    i, j = np.tril_indices(n)
    live = (ids[:, i] >= 0) & (ids[:, j] >= 0)
    a, b = col[np.maximum(ids[:, i], 0)], col[np.maximum(ids[:, j], 0)]
    return np.where(live, G[a, b], 0).astype(np.int64), units


def _median(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(np.min(t))


def measure(g, doc_off, words, reps, n=10):
    ids = g.top_words(n)[0]
    D = len(doc_off) - 1
    tenth = max(1, D // 10)
    off10, words10 = doc_off[:tenth + 1], words[:int(doc_off[tenth])]
    rec = {"K": g.K, "V": g.V, "docs": g.D, "tokens": g.N, "n": n, "reps": reps,
           "topic_groups": cooc_groups(g.K, n), "bytes_to_host_route_b": 8 * g.K * (n * (n + 1) // 2)}
    for window in (0, 10):
        t0 = time.perf_counter()
        a10 = host_cooc(off10, words10, ids, window)
        t10 = time.perf_counter() - t0
        b10 = g.word_cooccurrences(ids, window, off10, words10)
        assert a10[1] == b10[1] and np.array_equal(a10[0], b10[0]), f"the routes disagree on a tenth: window {window}"
        extrapolated = 10 * t10 > 60.0
        b = g.word_cooccurrences(ids, window)             # warm: code object, scratch growth
        if extrapolated:
            ta = ta_min = 10 * t10
        else:
            a = host_cooc(doc_off, words, ids, window)
            assert a[1] == b[1] and np.array_equal(a[0], b[0]), f"the routes disagree: window {window}"
            ta, ta_min = _median(lambda: host_cooc(doc_off, words, ids, window), max(1, min(reps, 3)))
        tb, tb_min = _median(lambda: g.word_cooccurrences(ids, window), reps)
        rec[f"window_{window}"] = {"units": b[1], "a_host_scipy_s": ta, "a_min_s": ta_min,
                                   "a_extrapolated_from_a_tenth": extrapolated, "b_device_s": tb, "b_min_s": tb_min,
                                   "b_not_slower_than_a": tb <= ta, "a_over_b": ta / tb}
    rec["b_not_slower_than_a"] = all(rec[f"window_{w}"]["b_not_slower_than_a"] for w in (0, 10))
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
    return g, train.doc_off, train.words


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
    return g, off, words


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--big", action="store_true", help="the big input only")
    ap.add_argument("--small", action="store_true", help="the small input only")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--big-types", type=int, default=100_000)
    ap.add_argument("--big-topics", type=int, default=512)
    ap.add_argument("--big-len", type=int, default=200)
    ap.add_argument("--big-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coherence", "latency.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("coherence_latency.py needs an MI355X")
    rec = {"tool": "coherence_latency", "device": torch.cuda.get_device_name(0)}
    for name, make in (("small", small_shard), ("big", big_shard)):
        if (name == "small" and args.big) or (name == "big" and args.small):
            continue
        g, off, words = make(args)
        rec[name] = measure(g, off, words, args.reps)
        g.close()
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
