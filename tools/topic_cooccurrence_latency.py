#!/usr/bin/env python3
"""Latency of the topic co-occurrence readout (run by hand on the GPU; not
bench.py).  Two routes to the same integers:

  (a) the only route before lda_topic_cooccurrence: doc_counts() of every
      document -- the D x K int32 table to the host -- then numpy: presence
      from the thresholds, codocs = P^T P and product = nd^T nd as float64
      matrix products (exact below 2^53, checked), overlap as K passes of
      np.minimum over the table;
  (b) lda_topic_cooccurrence: counted on the device, 8 K K bytes per
      requested table back.  The call is timed as the issue of this readout
      asks, through ctypes into output arrays allocated once (first-touch
      page faults of fresh 2 MiB numpy arrays were seen to cost 10-30 ms a
      call, a hundred times the call itself; they are the caller's choice,
      not the library's).  Route (a) allocates as numpy does: the public API
      gives it no other way.

Both for codocs alone and for all three tables, with min_tokens = 1,
min_count = 1, min_prop = 0: every nonzero topic of every document is present,
the most pairs the call can have.  Where route (a) runs on all documents the
two routes are compared equal before anything is timed; where it would not fit
comfortably it runs on the first --a-docs documents and its time is scaled by
D / a_docs (recorded as extrapolated, with the factor).

Inputs:
  c1_k20   the C1 changelist corpus (2000 documents), K = 20, after --sweeps sweeps;
  c1_k500  the same corpus at src/cmu_ron's K = 500;
  big      a synthetic shard, K = 512, --big-docs documents of 200 tokens
           (each document draws from 8 topics);
  ab       the block-LDS path against global atomics (the hook
           lda_debug_topic_cooccurrence_global) on a synthetic shard of
           --ab-docs documents of 200 tokens at K = 20 and at
           K = LDA_TOPIC_COOC_LDS_TOPICS, and the global path, the only one
           there, one topic above the boundary.
Medians of --reps calls, the routes alternating, the host clock around calls
that end in a device wait.  Route (b) is also timed alone, back to back
(b_alone_s): right after route (a)'s multi-threaded matrix product the same
call has been seen to take 6-22 ms instead of 0.15 ms at c1_k500 -- supposed,
not shown, to be the BLAS threads still spinning on the CPUs the HIP runtime's
own threads need; a_over_b uses the alternating figure.  Writes one JSON line to
profiles/topic_cooccurrence/latency.json.
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

THRESHOLDS = (1, 1, 0.0)
ALL = ("codocs", "overlap", "product")


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


def host_cooccurrence(g, doc_off, num_docs, stats, min_tokens, min_count, min_prop):
    """Route (a) on the first num_docs documents of the shard."""
    nd = g.doc_counts(doc_begin=0, num_docs=num_docs).astype(np.int64)
    lens = np.diff(doc_off[:num_docs + 1])
    used = lens >= min_tokens
    nd, lens = nd[used], lens[used]
    here = (nd >= min_count) & (nd.astype(np.float64) >= np.float64(min_prop) * lens.astype(np.float64)[:, None])
    out = {"docs_used": int(used.sum()), "tokens": nd.sum(0), "present": here.sum(0).astype(np.int64)}
    if "codocs" in stats:
        p = here.astype(np.float64)
        out["codocs"] = (p.T @ p).astype(np.int64)
    if "overlap" in stats:
        out["overlap"] = np.stack([np.minimum(nd[:, k:k + 1], nd).sum(0) for k in range(nd.shape[1])])
    if "product" in stats:
        assert int(lens.sum()) * int(lens.max(initial=0)) < 2 ** 53
        f = nd.astype(np.float64)
        out["product"] = (f.T @ f).astype(np.int64)
    return out


class Call:
    """lda_topic_cooccurrence into arrays allocated once."""

    def __init__(self, g, stats):
        import ctypes as C
        from ldagibbssampling_amd import capi
        self.g, self.stats, self.used = g, stats, C.c_int64()
        self.out = {"tokens": np.zeros(g.K, np.int64), "present": np.zeros(g.K, np.int64)}
        for s in stats:
            self.out[s] = np.zeros((g.K, g.K), np.int64)
        tabs = [self.out[s].ctypes.data if s in self.out else None for s in capi.TOPIC_COOC_STATS]
        self.args = (g._h, *THRESHOLDS, C.byref(self.used), self.out["tokens"].ctypes.data,
                     self.out["present"].ctypes.data, *tabs)
        self.check = capi.check

    def __call__(self):
        self.check(self.g._L.lda_topic_cooccurrence(*self.args), "lda_topic_cooccurrence")
        return dict(self.out, docs_used=int(self.used.value))


def _equal(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def part(g, doc_off, reps, a_docs):
    a_docs = min(g.D, a_docs)
    out = {"docs": g.D, "tokens": g.N, "K": g.K, "Kp": g.Kp, "reps": reps, "thresholds": list(THRESHOLDS),
           "route_a_docs": a_docs, "route_a_extrapolated": a_docs < g.D, "route_a_scale": g.D / a_docs,
           "nd_bytes_to_host_route_a": 4 * g.D * g.K}
    for name, stats in (("codocs", ("codocs",)), ("all", ALL)):
        route_a = lambda: host_cooccurrence(g, doc_off, a_docs, stats, *THRESHOLDS)
        route_b = Call(g, stats)
        if a_docs == g.D:
            assert _equal(route_a(), route_b()), "the routes disagree"
        (ta, ta_min), (tb, tb_min) = _alternate([route_a, route_b], reps)
        ta, ta_min = ta * g.D / a_docs, ta_min * g.D / a_docs
        (alone, alone_min), = _alternate([route_b], reps)
        out[name] = {"a_doc_counts_numpy_s": ta, "a_min_s": ta_min, "b_topic_cooccurrence_s": tb, "b_min_s": tb_min,
                     "b_alone_s": alone, "b_alone_min_s": alone_min, "result_bytes_to_host_route_b": 8 * (1 + 2 * g.K + len(stats) * g.K * g.K),
                     "b_not_slower_than_a": tb <= ta, "a_over_b": ta / tb}
    return out


def c1_part(args, K, alpha_sum, beta):
    from ldagibbssampling_amd.corpus import synthetic_changelists
    from ldagibbssampling_amd.sampler import GibbsSampler
    c = synthetic_changelists(num_docs=2000, num_types=5000, seed=1)
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, alpha_sum / K), beta, seed=1) as g:
        g.sweep(args.sweeps)
        out = part(g, c.doc_off, args.reps, g.D)
    out["sweeps"] = args.sweeps
    return out


def _shard(K, D, L, seed):
    rng = np.random.default_rng(seed)
    off = np.arange(D + 1, dtype=np.int64) * L
    words = rng.integers(0, 1000, D * L, dtype=np.int32)
    own = rng.integers(0, K, (D, 8), dtype=np.int32)
    z = np.take_along_axis(own, rng.integers(0, 8, (D, L)), axis=1).reshape(-1).astype(np.int32)
    return off, words, z


def big_part(args):
    from ldagibbssampling_amd.sampler import GibbsSampler
    K, L, D = 512, 200, args.big_docs
    off, words, z = _shard(K, D, L, 5)
    with GibbsSampler(K, 1000, off, words, np.full(K, 0.1), 0.01, seed=1, z_init=z) as g:
        g.apply()
        return part(g, off, args.reps, args.a_docs)


def ab_part(args):
    from ldagibbssampling_amd import capi
    from ldagibbssampling_amd.sampler import GibbsSampler
    lib = capi.load()
    edge = capi.TOPIC_COOC_LDS_TOPICS
    out = {"docs": args.ab_docs, "doc_len": 200, "thresholds": list(THRESHOLDS), "reps": args.reps,
           "lds_topics": edge}
    for K in (20, edge, edge + 1):
        off, words, z = _shard(K, args.ab_docs, 200, 6)
        with GibbsSampler(K, 1000, off, words, np.full(K, 0.1), 0.01, seed=1, z_init=z) as g:
            g.apply()
            rec = {}
            for name, stats in (("codocs", ("codocs",)), ("all", ALL)):
                default = Call(g, stats)

                def forced():
                    lib.lda_debug_topic_cooccurrence_global(1)
                    try:
                        return default()
                    finally:
                        lib.lda_debug_topic_cooccurrence_global(0)
                want = g.topic_cooccurrence(stats, *THRESHOLDS)
                assert _equal(default(), want) and _equal(forced(), want), "the paths disagree"
                (td, td_min), (tg, tg_min) = _alternate([default, forced], args.reps)
                rec[name] = {"default_path": "lds" if K <= edge else "global", "default_s": td, "default_min_s": td_min,
                             "global_atomics_s": tg, "global_atomics_min_s": tg_min, "global_over_default": tg / td}
            out[f"K{K}"] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=("c1", "big", "ab"), help="one part only")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--big-docs", type=int, default=200_000)
    ap.add_argument("--a-docs", type=int, default=5_000, help="route (a)'s documents on the big shard")
    ap.add_argument("--ab-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topic_cooccurrence", "latency.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("topic_cooccurrence_latency.py needs an MI355X")
    rec = {"tool": "topic_cooccurrence_latency", "device": torch.cuda.get_device_name(0)}
    if args.only in (None, "c1"):
        rec["c1_k20"] = c1_part(args, 20, 20 * 0.1, 0.01)
        rec["c1_k500"] = c1_part(args, 500, 100.0, 1.0)
    if args.only in (None, "big"):
        rec["big"] = big_part(args)
    if args.only in (None, "ab"):
        rec["ab"] = ab_part(args)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
