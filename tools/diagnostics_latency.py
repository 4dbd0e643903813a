#!/usr/bin/env python3
"""Latency of the topic-diagnostics statistics (run by hand on the GPU; not
bench.py).  Two routes to the same integer statistics for each topic's n = 20
top words, checked equal before they are timed:

  (a) the only route before lda_topic_codocuments / lda_topic_word_stats:
      z() -- every topic assignment to the host -- and counts() -- the V x K
      table -- then numpy: the top words, the word statistics, per
      (document, topic) a bit mask of the listed words present, the pair counts
      of the masks, and the document statistics from chunked count rows;
  (b) GibbsSampler.top_words(n), .topic_word_stats(ids) and
      .topic_codocuments(ids, Mallet's seven proportions): counted on the
      device, 4 K n (n + 1) / 2 + 72 K + 28 K n bytes back.

Inputs (those of tools/readout_latency.py):
  small  the training corpus of tests/test_perplexity.py (_corpus_split(100)):
         1980 documents, V = 3000, K = 100, after --sweeps sweeps;
  big    a synthetic shard, V = 1e5, K = 512, 1e5 documents of 100 tokens
         (uniformly random word ids; each document draws from 8 topics).
Medians of --reps calls, the routes alternating, the host clock around calls
that end in a device wait.  Also timed on their own: topic_codocuments (the
two document kernels and their copies), one sweep of the same shard, and the
bytes the co-document kernel must read (tokens x 8 B x topic groups).
--trace-run only calls route (b) and two sweeps a few times, for a
`rocprofv3 --kernel-trace --stats` run of its own; --kernel-stats CSV adds
that run's per-kernel averages to the record (k_codoc against its bytes and
against the sampling kernels of one sweep).  Writes one JSON line to
profiles/diagnostics/diagnostics_latency.json.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PROPS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
HBM_PEAK = 8.0e12          # bytes/s, MI355X (HBM3E)
CODOC_LDS = 64 * 1024      # lda_kernels.h: CODOC_LDS_BYTES
CODOC_WAVES = 16           # lda_capi.cpp


def codoc_groups(K, n):
    per = 8 * CODOC_WAVES + 4 * (n * (n + 1) // 2)
    gt = min(K, CODOC_LDS // per)
    return -(-K // gt)


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
    """ids[K, n] from the V x K table on the host (tools/readout_latency.py)."""
    V, K = nw.shape
    keys = (nw.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(V, dtype=np.uint64))[:, None]
    keys[nw <= 0] = 0
    m = min(n, V)
    top = np.partition(keys, V - m, axis=0)[V - m:]
    top = np.sort(top, axis=0)[::-1].T                      # [K, m] descending
    ids = np.full((K, n), -1, np.int32)
    ids[:, :m] = np.where(top > 0, (np.uint64(0xFFFFFFFF) - (top & np.uint64(0xFFFFFFFF))).astype(np.int64), -1)
    return ids


def host_word_stats(nw, nwsum, ids, beta):
    V, K = nw.shape
    live = ids >= 0
    w = np.where(live, ids, 0)
    counts = np.where(live, nw[w, np.arange(K)[:, None]], 0).astype(np.int32)
    totals = np.where(live, nw.sum(1, dtype=np.int64)[w], 0)
    sumsq = np.einsum("wk,wk->k", nw.astype(np.int64), nw.astype(np.int64)).astype(np.uint64)
    # the shares of the listed words only (the full V x K quotient is not needed)
    rows = np.unique(w[live])
    share = ((beta + nw[rows].astype(np.float64)) / (V * beta + nwsum.astype(np.float64))[None, :]).sum(1)
    shares = np.where(live, share[np.searchsorted(rows, w)], 0.0)
    return counts, totals, shares, sumsq


def host_codoc(z, words, doc_off, ids, V):
    """The packed triangles [K, n (n + 1) / 2] from z on the host."""
    K, n = ids.shape
    D = len(doc_off) - 1
    # (word, topic) -> slot through a sorted key table
    kk, ii = np.nonzero(ids >= 0)
    keys = ids[kk, ii].astype(np.int64) * K + kk
    order = np.argsort(keys)
    keys, slots = keys[order], ii[order]
    tok = words.astype(np.int64) * K + z
    pos = np.minimum(np.searchsorted(keys, tok), len(keys) - 1) if len(keys) else np.zeros(len(tok), np.int64)
    hit = keys[pos] == tok if len(keys) else np.zeros(len(tok), bool)
    doc = np.repeat(np.arange(D, dtype=np.int64), np.diff(doc_off))
    # one (document, topic, slot) each, then a mask per (document, topic)
    trip = np.unique((doc[hit] * K + z[hit]) * 64 + slots[pos[hit]])
    out = np.zeros((K, n * (n + 1) // 2), np.int32)
    if len(trip) == 0:
        return out
    dk, slot = trip >> 6, trip & 63
    start = np.flatnonzero(np.r_[True, dk[1:] != dk[:-1]])
    mask = np.add.reduceat(np.uint64(1) << slot.astype(np.uint64), start)
    topic = (dk[start] % K).astype(np.int64)
    one = np.uint64(1)
    for i in range(n):
        has_i = (mask >> np.uint64(i)) & one != 0
        ti, mi = topic[has_i], mask[has_i]
        for j in range(i + 1):
            both = (mi >> np.uint64(j)) & one != 0
            out[:, i * (i + 1) // 2 + j] = np.bincount(ti[both], minlength=K)
    return out


def host_doc_stats(z, doc_off, alpha, props, chunk=8192):
    D, K = len(doc_off) - 1, len(alpha)
    A = 0.0
    for a in alpha:
        A += float(a)
    lens = np.diff(doc_off)
    out = np.zeros((K, 2 + len(props)), np.int64)
    for d0 in range(0, D, chunk):
        d1 = min(D, d0 + chunk)
        t0, t1 = int(doc_off[d0]), int(doc_off[d1])
        doc = np.repeat(np.arange(d1 - d0), lens[d0:d1])
        nd = np.bincount(doc * K + z[t0:t1], minlength=(d1 - d0) * K).reshape(d1 - d0, K)
        has = nd > 0
        out[:, 0] += has.sum(0)
        full = lens[d0:d1] > 0
        out[:, 1] += np.bincount(np.argmax(nd[full], axis=1), minlength=K)
        w = (alpha[None, :] + nd) / (lens[d0:d1].astype(np.float64)[:, None] + A)
        for i, p in enumerate(props):
            out[:, 2 + i] += (has & (w >= p)).sum(0)
    return out


def route_a(g, doc_off, words, n):
    z = g.z()
    nw, nwsum = g.counts()[:2]
    ids = host_top_words(nw, n)
    return (ids,) + host_word_stats(nw, nwsum, ids, g.beta) + (host_codoc(z, words, doc_off, ids, g.V),
                                                                 host_doc_stats(z, doc_off, g.alpha, PROPS))


def route_b(g, n):
    ids = g.top_words(n)[0]
    return (ids,) + g.topic_word_stats(ids) + g.topic_codocuments(ids, PROPS)


def measure(g, doc_off, words, reps, n=20):
    a, b = route_a(g, doc_off, words, n), route_b(g, n)
    names = ("word_ids", "counts", "totals", "share_sums", "sumsq", "codoc", "doc_stats")
    for name, x, y in zip(names, a, b):
        if name == "share_sums":
            assert np.allclose(x, y, rtol=1e-13, atol=0), "the routes disagree: share_sums"
        else:
            assert np.array_equal(x, y), f"the routes disagree: {name}"
    ids = b[0]
    def sweep():
        g.sweep(1)
        g.synchronize()      # lda_sweep returns when the sweep is enqueued

    fns = [lambda: route_a(g, doc_off, words, n), lambda: route_b(g, n), lambda: g.topic_codocuments(ids, PROPS),
           sweep, lambda: (g.z(), g.counts())]
    (ta, ta_min), (tb, tb_min), (tc, tc_min), (ts, ts_min), (tcp, _) = _alternate(fns, reps)
    groups = codoc_groups(g.K, n)
    must_read = 8 * g.N * groups
    return {"K": g.K, "V": g.V, "docs": g.D, "tokens": g.N, "n": n, "reps": reps,
            "bytes_to_host_route_a": 4 * g.N + 4 * g.V * g.K,
            "bytes_to_host_route_b": 4 * g.K * (n * (n + 1) // 2) + 72 * g.K + 28 * g.K * n + 8 * g.K,
            "a_host_numpy_s": ta, "a_min_s": ta_min, "a_copies_only_s": tcp, "b_device_s": tb, "b_min_s": tb_min,
            "b_not_slower_than_a": tb <= ta, "a_over_b": ta / tb,
            "codocuments_call_s": tc, "codocuments_call_min_s": tc_min, "sweep_s": ts, "sweep_min_s": ts_min,
            "codocuments_call_over_sweep": tc / ts,
            "codoc_topic_groups": groups, "codoc_bytes_must_read": must_read,
            # what k_codoc does read: z per group, a word only for a token of the group's topics
            "codoc_bytes_kernel_reads": g.N * (4 * groups + 4),
            "codocuments_call_fraction_of_hbm_peak": must_read / tc / HBM_PEAK}


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


def kernel_stats(path):
    """Average ns per kernel name from a rocprofv3 --kernel-trace --stats CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or row.get("Kernel_Name")
            avg = row.get("AverageNs") or row.get("Average_Ns") or row.get("AverageNs ")
            if name and avg:
                out[name] = {"calls": int(float(row.get("Calls", 0) or 0)), "average_ns": float(avg)}
    return out


def trace_part(stats, big):
    """k_codoc against its bytes and against the sampling kernels of a sweep."""
    def avg(kernel):    # the names are demangled: "lda::k_codoc(lda::CodocArgs)", "void lda::k_sample<8, 3, false>(...)"
        return sum(v["average_ns"] for k, v in stats.items() if "lda::" + kernel in k) * 1e-9
    ours = ("k_codoc", "k_doc_diag", "k_word_stats", "k_sumsq", "k_sample", "k_top_words")
    codoc, diag, sample = avg("k_codoc"), avg("k_doc_diag"), avg("k_sample")
    rec = {"k_codoc_s": codoc, "k_doc_diag_s": diag, "k_sample_s": sample,
           "kernels": {k: v for k, v in stats.items() if any("lda::" + o in k for o in ours)}}
    if codoc > 0 and big:
        rec["k_codoc_fraction_of_hbm_peak"] = big["codoc_bytes_must_read"] / codoc / HBM_PEAK
        rec["k_codoc_bytes_read_fraction_of_hbm_peak"] = big["codoc_bytes_kernel_reads"] / codoc / HBM_PEAK
        if sample > 0:
            rec["k_codoc_over_k_sample"] = codoc / sample
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--big", action="store_true", help="the big input only")
    ap.add_argument("--small", action="store_true", help="the small input only")
    ap.add_argument("--trace-run", action="store_true", help="route (b) and sweeps on the big input, untimed")
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel stats CSV of a --trace-run to add to the record")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--big-types", type=int, default=100_000)
    ap.add_argument("--big-topics", type=int, default=512)
    ap.add_argument("--big-len", type=int, default=100)
    ap.add_argument("--big-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diagnostics", "diagnostics_latency.json"))
    args = ap.parse_args()

    if args.kernel_stats and not os.path.exists(args.out):
        sys.exit(f"--kernel-stats adds to {args.out}, which does not exist")
    if args.kernel_stats:
        rec = json.loads(open(args.out).read())
        rec["kernel_trace_big"] = trace_part(kernel_stats(args.kernel_stats), rec.get("big"))
    else:
        import torch
        if not torch.cuda.is_available():
            sys.exit("diagnostics_latency.py needs an MI355X")
        if args.trace_run:
            g, off, words = big_shard(args)
            for _ in range(5):
                route_b(g, 20)
                g.sweep(2)
            g.close()
            return
        rec = {"tool": "diagnostics_latency", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_s": HBM_PEAK}
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
