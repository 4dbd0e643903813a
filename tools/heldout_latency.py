#!/usr/bin/env python3
"""Latency of held-out evaluation by document completion (run by hand on the
GPU; not bench.py).  Two routes to the same number:
  (a) the route before lda_doc_completion: GibbsSampler.infer, then counts()
      (the V x K table to the host), then oracle.doc_completion_loglik (one
      CPU thread);
  (b) GibbsSampler.doc_completion (one native call, scored on the device).
Both include the inference; the scoring halves are also timed alone
(a: counts() + the oracle, b: heldout_loglik with theta given).  Two inputs:
  small  the corpus of tests/test_perplexity.py (_corpus_split(100)): 1980
         training and 220 held-out documents, V = 3000, K = 100;
  big    a synthetic shard, V = 1e5, K = 512, 1e5 held-out documents of 100
         observed and 100 scored tokens (uniformly random word ids, so every
         scored token gathers a random 2 KiB row of a 205 MB table).
Medians of --reps calls, the routes alternating; every call ends in a device
wait.  Writes one JSON line to profiles/heldout/heldout_latency.json.

The kernel's own time comes from a separate run under the profiler,
  rocprofv3 --kernel-trace --stats -d DIR -o heldout -- \\
      python tools/heldout_latency.py --big --only-new
whose kernel statistics (DIR/heldout_results.db, or the kernel-stats csv of
--output-format csv) --kernel-stats turns into
profiles/heldout/heldout_kernel.json (row bytes per second =
scored tokens x Kp x 4 bytes over the kernel's time).
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

INFER = dict(n_iter=100, thin=10, burn_in=10, seed=7)


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


def _routes(g, obs, sc, oracle, reps, only_new):
    """Times both routes on sampler g; obs / sc are (doc_off, words)."""
    def route_a():
        theta = g.infer(obs[0], obs[1], **INFER)
        nw, nwsum, _, _ = g.counts()
        return oracle.doc_completion_loglik(g.K, g.V, nw, nwsum, g.beta, theta, sc[0], sc[1])

    def route_b():
        return g.doc_completion(obs[0], obs[1], sc[0], sc[1], **INFER)[1]

    theta = g.infer(obs[0], obs[1], **INFER)

    def score_a():
        nw, nwsum, _, _ = g.counts()
        return oracle.doc_completion_loglik(g.K, g.V, nw, nwsum, g.beta, theta, sc[0], sc[1])

    def score_b():
        return g.heldout_loglik(theta, sc[0], sc[1])[1]

    n_sc = int(sc[0][-1] - sc[0][0])
    out = {"held_docs": len(sc[0]) - 1, "tokens_observed": int(obs[0][-1] - obs[0][0]), "tokens_scored": n_sc,
           "K": g.K, "Kp": g.Kp, "V": g.V, "table_bytes": 4 * g.V * g.Kp, "row_bytes_gathered": 4 * g.Kp * n_sc,
           "counts_bytes_to_host_route_a": 4 * g.V * g.K, "reps": reps}
    if only_new:
        (b, b_min), (sb, sb_min) = _alternate([route_b, score_b], reps)
        out.update({"b_doc_completion_s": b, "b_min_s": b_min, "b_heldout_loglik_only_s": sb,
                    "b_heldout_loglik_only_min_s": sb_min})
        return out
    ll_a, ll_b = route_a(), route_b()
    (a, a_min), (b, b_min), (sa, sa_min), (sb, sb_min) = _alternate([route_a, route_b, score_a, score_b], reps)
    out.update({
        "a_infer_counts_oracle_s": a, "a_min_s": a_min, "b_doc_completion_s": b, "b_min_s": b_min,
        "b_not_slower_than_a": b <= a, "a_over_b": a / b,
        "a_counts_oracle_only_s": sa, "a_counts_oracle_only_min_s": sa_min,
        "b_heldout_loglik_only_s": sb, "b_heldout_loglik_only_min_s": sb_min, "scoring_only_a_over_b": sa / sb,
        "ll_a": ll_a, "ll_b": ll_b, "rel_diff_a_vs_b": abs(ll_a - ll_b) / abs(ll_a),
        "perplexity_b": float(np.exp(-ll_b / n_sc)),
    })
    return out


def small_part(args, oracle):
    from ldagibbssampling_amd.corpus import document_completion_split, synthetic_lda
    from ldagibbssampling_amd.sampler import GibbsSampler
    K = 100
    c = synthetic_lda(num_docs=2200, num_types=3000, num_topics=K, doc_len=None, mean_len=80, min_len=10,
                      max_len=300, seed=20261015, k_true=min(K, 50))
    perm = np.random.default_rng(0).permutation(c.num_docs)
    n_held = c.num_docs // 10
    train = c.subset(np.sort(perm[n_held:]))
    obs, sc = document_completion_split(c.subset(np.sort(perm[:n_held])))
    with GibbsSampler(K, c.num_types, train.doc_off, train.words, np.full(K, 10.0 / K), 0.01, seed=1) as g:
        g.sweep(args.sweeps)
        out = _routes(g, (obs.doc_off, obs.words), (sc.doc_off, sc.words), oracle, args.reps, args.only_new)
    out["train"] = {"docs": train.num_docs, "tokens": train.num_tokens, "sweeps": args.sweeps}
    return out


def big_part(args, oracle):
    from ldagibbssampling_amd.sampler import GibbsSampler
    V, K, L = args.big_types, args.big_topics, args.big_len
    D, Dh = args.big_train_docs, args.big_held_docs
    rng = np.random.default_rng(5)
    off = np.arange(D + 1, dtype=np.int64) * L
    words = rng.integers(0, V, D * L, dtype=np.int32)
    # topics as after training: each document draws from a few topics
    own = rng.integers(0, K, (D, 8), dtype=np.int32)
    z = np.take_along_axis(own, rng.integers(0, 8, (D, L)), axis=1).reshape(-1).astype(np.int32)
    hoff = np.arange(Dh + 1, dtype=np.int64) * L
    obs = (hoff, rng.integers(0, V, Dh * L, dtype=np.int32))
    sc = (hoff, rng.integers(0, V, Dh * L, dtype=np.int32))
    with GibbsSampler(K, V, off, words, np.full(K, 0.1), 0.01, seed=1, z_init=z) as g:
        g.apply()
        out = _routes(g, obs, sc, oracle, args.reps, args.only_new)
    out["train"] = {"docs": D, "tokens": D * L}
    return out


def kernel_stats(args):
    """The k_doc_completion (and k_heldout_inv) rows of a rocprofv3 run's
    kernel statistics, with the row bytes per second of the big input."""
    rows = []
    want = lambda name: "k_doc_completion" in name or "k_heldout_inv" in name
    if args.kernel_stats.endswith(".db"):       # rocprofv3's default output: an SQLite database (view `kernels`)
        import sqlite3
        db = sqlite3.connect(args.kernel_stats)
        for name, calls, total, mn, mx in db.execute(
                "select name, count(*), sum(duration), min(duration), max(duration) from kernels group by name"):
            if want(name):
                rows.append({"name": name, "calls": calls, "total_ns": total, "average_ns": total / calls,
                             "min_ns": mn, "max_ns": mx})
    else:                                       # --output-format csv: <name>_kernel_stats.csv
        with open(args.kernel_stats, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("Kernel_Name") or ""
                if want(name):
                    rows.append({"name": name, "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                                 "average_ns": float(r["AverageNs"]), "min_ns": int(float(r["MinNs"])),
                                 "max_ns": int(float(r["MaxNs"]))})
    if not any("k_doc_completion" in r["name"] for r in rows):
        sys.exit(f"{args.kernel_stats}: no k_doc_completion row")
    Kp = 64
    while Kp < args.big_topics:
        Kp *= 2
    # a call is cut into chunks of 2^22 / K documents, one launch each
    chunks = -(-args.big_held_docs // max(1, (1 << 22) // args.big_topics))
    row_bytes = 4 * Kp * args.big_held_docs * args.big_len
    for r in rows:
        if "k_doc_completion" in r["name"]:
            r["launches_per_call"] = chunks
            r["row_bytes_per_call"] = row_bytes
            r["row_bytes_per_s"] = row_bytes * (r["calls"] / chunks) / (r["total_ns"] * 1e-9)
    rec = {"tool": "heldout_latency --kernel-stats", "input": "big", "V": args.big_types, "K": args.big_topics,
           "Kp": Kp, "held_docs": args.big_held_docs, "tokens_scored": args.big_held_docs * args.big_len,
           "table_bytes": 4 * args.big_types * Kp, "kernels": rows}
    out = os.path.join(os.path.dirname(args.out), "heldout_kernel.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--big", action="store_true", help="the big input only")
    ap.add_argument("--small", action="store_true", help="the small input only")
    ap.add_argument("--only-new", action="store_true", help="route (b) only (for the profiler run)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--big-types", type=int, default=100_000)
    ap.add_argument("--big-topics", type=int, default=512)
    ap.add_argument("--big-len", type=int, default=100)
    ap.add_argument("--big-train-docs", type=int, default=200_000)
    ap.add_argument("--big-held-docs", type=int, default=100_000)
    ap.add_argument("--kernel-stats", help="a rocprofv3 results .db or kernel-stats csv to summarise (no device needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heldout", "heldout_latency.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args)

    import torch
    if not torch.cuda.is_available():
        sys.exit("heldout_latency.py needs an MI355X")
    oracle = None
    if not args.only_new:
        from oracle import oracle
        oracle.build()
    rec = {"tool": "heldout_latency", "device": torch.cuda.get_device_name(0)}
    if not args.big:
        rec["small"] = small_part(args, oracle)
    if not args.small:
        rec["big"] = big_part(args, oracle)
    line = json.dumps(rec)
    if not args.only_new:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
