#!/usr/bin/env python3
"""Latency of the topic phrases (run by hand on the GPU; not bench.py).  Two
routes to the same arrays, compared equal before anything is timed:

  (a) the route before lda_topic_phrases: z() -- every topic assignment to the
      host -- then a vectorised numpy count: the run boundaries from np.diff
      of z and the document starts, the qualifying runs as rows (topic, words,
      -1 padded to the longest run present), the distinct phrases, their
      counts and first rows from np.unique over the rows (which sorts them in
      the phrase order: a prefix first), then one np.lexsort by (topic, count
      descending, row order) cut at n per topic.  Not the Python loop of
      tests/topic_phrases_numpy.py, which would flatter (b);
  (b) GibbsSampler.topic_phrases(n): counted and selected on the device.

Inputs:
  small  the training corpus of tests/test_perplexity.py (_corpus_split(100)):
         1980 documents, V = 3000, K = 100, after --sweeps sweeps;
  big    the synthetic shard of tools/topic_docs_latency.py, V = 1e5, K = 512,
         1e5 documents of 100 tokens (uniformly random word ids; each document
         starts with 8 topics), after --big-sweeps sweeps.
Both at n = 10, lengths 2 .. 32, min_count 1.  Medians of --reps calls, the
routes alternating, the host clock around calls that end in a device wait; the
copy of z alone is timed beside them.  Writes one JSON line to
profiles/topic_phrases/latency.json.
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

N_TOP, MIN_LEN, MAX_LEN = 10, 2, 32


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


def host_topic_phrases(words, z, doc_off, K, n, lo=MIN_LEN, hi=MAX_LEN, min_count=1):
    """GibbsSampler.topic_phrases' arrays from z on the host, vectorised."""
    N = len(z)
    w = np.full((K, n, hi), -1, np.int32)
    lens = np.zeros((K, n), np.int32)
    cnt = np.zeros((K, n), np.int64)
    first = np.full((K, n), -1, np.int64)
    runs = np.zeros(K, np.int64)
    distinct = np.zeros(K, np.int64)
    if N == 0:
        return w, lens, cnt, first, runs, distinct, 0
    start = np.ones(N, bool)
    start[1:] = np.diff(z) != 0
    ds = doc_off[:-1]
    start[ds[ds < N]] = True
    s = np.flatnonzero(start)
    ln = np.diff(np.append(s, N))
    skipped = int(np.count_nonzero(ln > hi))
    ok = (ln >= lo) & (ln <= hi)
    s, ln = s[ok], ln[ok]
    if len(s) == 0:
        return w, lens, cnt, first, runs, distinct, skipped
    width = int(ln.max())
    rows = np.full((len(s), width + 1), -1, np.int32)
    rows[:, 0] = z[s]
    cols = np.arange(width)
    mask = cols[None, :] < ln[:, None]
    rows[:, 1:][mask] = words[(s[:, None] + cols[None, :])[mask]]
    uniq, idx, c = np.unique(rows, axis=0, return_index=True, return_counts=True)
    topic = uniq[:, 0].astype(np.int64)
    runs += np.bincount(topic, weights=c, minlength=K).astype(np.int64)
    distinct += np.bincount(topic, minlength=K)
    keep = c >= min_count
    uniq, idx, c, topic = uniq[keep], idx[keep], c[keep], topic[keep]
    order = np.lexsort((np.arange(len(c)), -c, topic))
    t_sorted = topic[order]
    begin = np.searchsorted(t_sorted, np.arange(K), side="left")
    rank = np.arange(len(order)) - begin[t_sorted]
    sel = order[rank < n]
    k_sel, r_sel = topic[sel], rank[rank < n]
    plen = ln[idx[sel]]
    w[k_sel, r_sel, :width] = uniq[sel, 1:][:, :min(width, hi)]
    lens[k_sel, r_sel] = plen
    cnt[k_sel, r_sel] = c[sel]
    first[k_sel, r_sel] = s[idx[sel]]
    return w, lens, cnt, first, runs, distinct, skipped


def part(g, words, doc_off, reps):
    out = {"docs": g.D, "tokens": g.N, "K": g.K, "n": N_TOP, "min_len": MIN_LEN, "max_len": MAX_LEN, "reps": reps,
           "z_bytes_to_host_route_a": 4 * g.N}
    route_a = lambda: host_topic_phrases(words, g.z(), doc_off, g.K, N_TOP)
    route_b = lambda: g.topic_phrases(N_TOP, MIN_LEN, MAX_LEN, 1)
    a, b = route_a(), route_b()
    assert all(np.array_equal(x, y) for x, y in zip(a[:6], b[:6])) and a[6] == b[6], "the routes disagree"
    copy_only = lambda: g.z()
    (ta, ta_min), (tb, tb_min), (tc, tc_min) = _alternate([route_a, route_b, copy_only], reps)
    out.update({"qualifying_runs": int(b[4].sum()), "distinct_phrases": int(b[5].sum()), "skipped_long": int(b[6]),
                "a_z_host_count_s": ta, "a_min_s": ta_min, "b_topic_phrases_s": tb, "b_min_s": tb_min,
                "a_z_copy_only_s": tc, "a_copy_share": tc / ta,
                "result_bytes_to_host_route_b": int(sum(x.nbytes for x in b[:6])),
                "b_not_slower_than_a": tb <= ta, "a_over_b": ta / tb})
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
        out = part(g, train.words, train.doc_off, args.reps)
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
        if args.big_sweeps:
            g.sweep(args.big_sweeps)
        out = part(g, words, off, args.reps)
    out["sweeps"] = args.big_sweeps
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--big", action="store_true", help="the big input only")
    ap.add_argument("--small", action="store_true", help="the small input only")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--big-sweeps", type=int, default=50)
    ap.add_argument("--big-types", type=int, default=100_000)
    ap.add_argument("--big-topics", type=int, default=512)
    ap.add_argument("--big-len", type=int, default=100)
    ap.add_argument("--big-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topic_phrases", "latency.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("topic_phrases_latency.py needs an MI355X")
    rec = {"tool": "topic_phrases_latency", "device": torch.cuda.get_device_name(0)}
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
