#!/usr/bin/env python3
"""Latency of the data behind an LDAvis view (run by hand on the GPU; not
bench.py).  Two routes to the same lists -- each topic's R = 30 most relevant
words under 101 lambdas (0, 0.01, ..., 1), the R most salient words, and the nw
rows of every word in those lists (the token table's input):

  (a) the host: lda_get_counts copies the V x K table to the host, then numpy
      restates the selection: tw, logtp, logprob once, per lambda the key and
      a partition of every topic's column and a sort of the cells at or above its R-th key, the saliency of every
      word, the rows gathered from the host table;
  (b) the device: GibbsSampler.relevant_words(R, lambdas), .salient_words(R)
      and .word_rows(ids): only the lists come back.

Route (a)'s word ids are checked equal to route (b)'s before they are timed
wherever the restatement's own keys are more than 1e-7 apart (the device's log
is not the host's).  Inputs:
  small  V = 3000, K = 100, 160 000 tokens;
  big    V = 100 000, K = 512, 2e7 tokens
(word ~ 1 / (1 + id) over a random permutation of the ids, each document of 200
tokens drawing from 8 topics; two sweeps).  Medians of --reps calls, the
routes alternating, the host clock around calls that end in a device wait.  No
ratio is fixed in advance: the record carries both times, a_over_b and the
bytes each route copies to the host.  Writes one JSON line to
profiles/relevance/latency.json.
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


def host_lists(nw, nwsum, beta, R, lambdas):
    """(ids[L, K, R] int32, salient[R] int32, rows of the listed words) on the
    host, with lda_mi355x.h's expressions."""
    V, K = nw.shape
    tw = nw.sum(axis=1, dtype=np.int64)
    N = float(nwsum.astype(np.int64).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        logprob = np.log((nw.astype(np.float64) + beta) / (nwsum.astype(np.float64)[None, :] + V * beta))
        logtp = np.log(tw.astype(np.float64) / N)
    logtp = np.where(tw > 0, logtp, 0.0)
    logprob[nw <= 0] = -np.inf                       # no candidate
    ids = np.full((len(lambdas), K, R), -1, np.int32)
    for l, lam in enumerate(lambdas):
        key = logprob - ((1.0 - lam) * logtp)[:, None]
        # the R-th largest key of every column, then every cell at or above it (ties included)
        thr = -np.partition(-key, min(R, V) - 1, axis=0)[min(R, V) - 1]
        kk, ww = np.nonzero((key >= thr[None, :]).T & np.isfinite(key.T))
        o = np.lexsort((ww, -key[ww, kk], kk))
        kk, ww = kk[o], ww[o]
        rank = np.arange(kk.size) - np.searchsorted(kk, kk, side="left")
        keep = rank < R
        ids[l, kk[keep], rank[keep]] = ww[keep]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = nw / np.maximum(tw, 1)[:, None].astype(np.float64)
        p = nwsum.astype(np.float64) / N
        term = np.where(nw > 0, q * np.log(q / p[None, :]), 0.0)
    sal = (tw / N) * term.sum(axis=1)
    sal[tw <= 0] = -np.inf
    top = np.flatnonzero((sal >= -np.partition(-sal, min(R, V) - 1)[min(R, V) - 1]) & np.isfinite(sal))
    top = top[np.lexsort((top, -sal[top]))][:R]
    salient = np.full(R, -1, np.int32)
    salient[:top.size] = top
    listed = np.union1d(ids[ids >= 0], salient[salient >= 0])
    return ids, salient, nw[listed], listed


def _median(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(np.min(t))


def measure(g, reps, R=30):
    from ldagibbssampling_amd import capi
    lambdas = np.array([min(1.0, i * 0.01) for i in range(101)])
    beta = 0.01

    def route_b():
        r = g.relevant_words(R, lambdas)
        s = g.salient_words(R)
        listed = np.union1d(r[0][r[0] >= 0], s[0][s[0] >= 0]).astype(np.int32)
        return r, s, g.word_rows(listed), listed

    def route_a(lams=lambdas):
        nw, nwsum = g.counts()[:2]
        return host_lists(nw, nwsum, beta, R, lams)

    b = route_b()                                      # warm: code objects, scratch growth
    t0 = time.perf_counter()
    a1 = route_a(lambdas[:1])
    t1 = time.perf_counter() - t0
    t0 = time.perf_counter()
    a11 = route_a(lambdas[::10])
    t11 = time.perf_counter() - t0
    same = float(np.mean(a11[0] == b[0][0][::10]))
    assert same > 0.999, f"the routes' word ids agree in {same:.6f} of the slots"
    salient_same = float(np.mean(a11[1] == b[1][0]))
    assert salient_same > 0.9, f"the routes' salient words agree in {salient_same:.3f} of the slots"
    estimate = t1 + 10.0 * (t11 - t1)                  # 101 lambdas from the cost of 1 and of 11
    extrapolated = estimate > 60.0
    if extrapolated:
        ta = ta_min = estimate
    else:
        ta, ta_min = _median(route_a, max(1, min(reps, 3)))
    tb, tb_min = _median(route_b, reps)
    tr, _ = _median(lambda: g.relevant_words(R, lambdas), reps)
    ts, _ = _median(lambda: g.salient_words(R), reps)
    tw, _ = _median(lambda: g.word_rows(b[3]), reps)
    t1b, _ = _median(lambda: g.relevant_words(R, 0.6), reps)
    tc, _ = _median(lambda: g.counts(), max(1, min(reps, 3)))
    cells = lambdas.size * g.K * R
    return {"K": g.K, "V": g.V, "tokens": g.N, "R": R, "lambdas": int(lambdas.size), "reps": reps,
            "lambdas_per_pass": capi.relevance_batch(R), "word_ids_equal_fraction": same,
            "salient_ids_equal_fraction": salient_same,
            "listed_words": int(b[3].size),
            "a_host_numpy_s": ta, "a_min_s": ta_min, "a_extrapolated_from_1_and_11_lambdas": extrapolated,
            "a_get_counts_s": tc, "a_one_lambda_s": t1,
            "b_device_s": tb, "b_min_s": tb_min, "b_relevant_words_s": tr, "b_salient_words_s": ts,
            "b_word_rows_s": tw, "b_relevant_words_one_lambda_s": t1b,
            "a_over_b": ta / tb, "b_not_slower_than_a": tb <= ta,
            "bytes_to_host": {"a": 4 * g.V * g.K + 4 * g.K, "b": 32 * cells + 24 * R + int(b[3].size) * (4 * g.K + 8)}}


def shard(V, K, D, L=200, seed=5):
    from ldagibbssampling_amd.sampler import GibbsSampler
    rng = np.random.default_rng(seed)
    p = 1.0 / (1.0 + np.arange(V))
    off = np.arange(D + 1, dtype=np.int64) * L
    words = rng.permutation(V)[rng.choice(V, size=D * L, p=p / p.sum())].astype(np.int32)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relevance", "latency.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("relevance_latency.py needs an MI355X")
    rec = {"tool": "relevance_latency", "device": torch.cuda.get_device_name(0)}
    for name, (V, K, D) in (("small", (3000, 100, 800)), ("big", (100_000, 512, 100_000))):
        if (name == "small" and args.big) or (name == "big" and args.small):
            continue
        g = shard(V, K, D)
        rec[name] = measure(g, args.reps)
        g.close()
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
