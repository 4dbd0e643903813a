#!/usr/bin/env python3
"""Latency of the topics-by-group readout (run by hand on the GPU; not
bench.py).  Two questions, two routes each to the same integers:

  prevalence
  (a) the only route before lda_group_topics: doc_counts() of every document
      -- the D x K int32 table to the host -- then numpy: per group a masked
      sum of the rows (tokens), of the presence bits (present) and of
      (n << 32) // L in uint64 (shares);
  (b) lda_group_topics: counted on the device, 8 (2 G + 3 G K) bytes back.
  a group's words
  (a) get_z, then np.add.at into a V x K table over the masked documents'
      tokens and a per-topic selection of the top n (np.lexsort on -count,
      word);
  (b) lda_subcorpus_count + lda_subcorpus_top_words: 2 K n int32 and K int64
      back.

Route (b) is timed as the C call through ctypes into arrays allocated once
(first-touch page faults of fresh numpy arrays are the caller's choice, not the
library's); route (a) allocates as numpy does: the public API gives it no other
way.  Where route (a) runs on all documents the two routes are compared equal
before anything is timed; where the D x K table would not fit comfortably it
runs on the first --a-docs documents and its time is scaled by D / a_docs
(recorded as extrapolated, with the factor).  jsLDA's thresholds (10, 2, 0.05),
G = 20 groups drawn at random, the mask is group 0.

Inputs:
  c1_k20   the C1 changelist corpus (2000 documents), K = 20, after --sweeps sweeps;
  c1_k500  the same corpus at src/cmu_ron's K = 500;
  big      a synthetic shard, K = 512, --big-docs documents of 200 tokens
           (each document draws from 8 topics);
  ab       the block-LDS path against global atomics (the hook
           lda_debug_group_topics_global) on a synthetic shard of --ab-docs
           documents of 200 tokens at K = 20: G = 20, the last G that
           lda_group_topics_path puts on the LDS side, and the first on the
           global side, where the global path is the only one.
Medians of --reps calls, the routes alternating, the host clock around calls
that end in a device wait; route (b) is also timed alone, back to back
(b_alone_s).  Writes one JSON line to profiles/group_topics/latency.json.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

THRESHOLDS = (10, 2, 0.05)
G = 20
TOP_N = 10


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


def host_group_topics(g, doc_off, groups, num_groups, num_docs, min_tokens, min_count, min_prop):
    """Prevalence, route (a), on the first num_docs documents of the shard."""
    nd = g.doc_counts(doc_begin=0, num_docs=num_docs).astype(np.int64)
    lens = np.diff(doc_off[:num_docs + 1])
    grp = groups[:num_docs]
    used = (grp >= 0) & (lens >= min_tokens)
    nd, lens, grp = nd[used], lens[used], grp[used]
    here = (nd >= min_count) & (nd.astype(np.float64) >= np.float64(min_prop) * lens.astype(np.float64)[:, None])
    shares = (nd.astype(np.uint64) << np.uint64(32)) // lens.astype(np.uint64)[:, None]
    K = nd.shape[1]
    out = {"group_docs": np.bincount(grp, minlength=num_groups).astype(np.int64),
           "group_tokens": np.bincount(grp, weights=lens, minlength=num_groups).astype(np.int64),
           "tokens": np.zeros((num_groups, K), np.int64), "present": np.zeros((num_groups, K), np.int64),
           "shares": np.zeros((num_groups, K), np.uint64)}
    for k in range(num_groups):
        rows = grp == k
        out["tokens"][k] = nd[rows].sum(0)
        out["present"][k] = here[rows].sum(0)
        out["shares"][k] = shares[rows].sum(0, dtype=np.uint64)
    return out


def host_group_words(g, doc_off, words, mask, n):
    """A group's words, route (a)."""
    z = g.z()
    keep = np.repeat(mask != 0, np.diff(doc_off))
    sub = np.zeros((g.V, g.K), np.int64)
    np.add.at(sub, (words[keep], z[keep]), 1)
    ids = np.full((g.K, n), -1, np.int32)
    cnt = np.zeros((g.K, n), np.int32)
    rows = np.arange(g.V)
    for k in range(g.K):
        order = np.lexsort((rows, -sub[:, k]))[:n]
        order = order[sub[order, k] > 0]
        ids[k, :len(order)] = order
        cnt[k, :len(order)] = sub[order, k]
    return ids, cnt, sub.sum(0)


class GroupCall:
    """lda_group_topics into arrays allocated once."""

    def __init__(self, g, groups, num_groups):
        from ldagibbssampling_amd import capi
        self.g, self.groups = g, np.ascontiguousarray(groups, np.int32)
        self.out = {"group_docs": np.zeros(num_groups, np.int64), "group_tokens": np.zeros(num_groups, np.int64),
                    "tokens": np.zeros((num_groups, g.K), np.int64), "present": np.zeros((num_groups, g.K), np.int64),
                    "shares": np.zeros((num_groups, g.K), np.uint64)}
        self.args = (g._h, self.groups.ctypes.data, num_groups, *THRESHOLDS,
                     *(self.out[s].ctypes.data for s in ("group_docs", "group_tokens", "tokens", "present", "shares")))
        self.check = capi.check

    def __call__(self):
        self.check(self.g._L.lda_group_topics(*self.args), "lda_group_topics")
        return self.out


class WordsCall:
    """lda_subcorpus_count + lda_subcorpus_top_words into arrays allocated once."""

    def __init__(self, g, mask, n):
        from ldagibbssampling_amd import capi
        self.g, self.mask, self.n = g, np.ascontiguousarray(mask, np.uint8), n
        self.ids, self.cnt = np.zeros((g.K, n), np.int32), np.zeros((g.K, n), np.int32)
        self.tot = np.zeros(g.K, np.int64)
        self.check = capi.check

    def __call__(self):
        L, h = self.g._L, self.g._h
        self.check(L.lda_subcorpus_count(h, self.mask.ctypes.data, 0), "lda_subcorpus_count")
        self.check(L.lda_subcorpus_top_words(h, self.n, self.ids.ctypes.data, self.cnt.ctypes.data,
                                             self.tot.ctypes.data), "lda_subcorpus_top_words")
        return self.ids, self.cnt, self.tot


def _equal(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _record(ta, tb, alone):
    return {"a_host_s": ta[0], "a_min_s": ta[1], "b_device_s": tb[0], "b_min_s": tb[1], "b_alone_s": alone[0],
            "b_alone_min_s": alone[1], "b_not_slower_than_a": tb[0] <= ta[0], "a_over_b": ta[0] / tb[0]}


def part(g, doc_off, words, reps, a_docs):
    from ldagibbssampling_amd import capi
    a_docs = min(g.D, a_docs)
    groups = np.random.default_rng(3).integers(0, G, g.D).astype(np.int32)
    mask = (groups == 0).astype(np.uint8)
    scale = g.D / a_docs
    out = {"docs": g.D, "tokens": g.N, "K": g.K, "Kp": g.Kp, "V": g.V, "G": G, "reps": reps,
           "thresholds": list(THRESHOLDS), "route_a_docs": a_docs, "route_a_extrapolated": a_docs < g.D,
           "route_a_scale": scale, "nd_bytes_to_host_route_a": 4 * g.D * g.K,
           "result_bytes_to_host_route_b": 8 * (2 * G + 3 * G * g.K),
           "path": "lds" if capi.load().lda_group_topics_path(G, g.K, 3, None) == 1 else "global"}
    route_a = lambda: host_group_topics(g, doc_off, groups, G, a_docs, *THRESHOLDS)
    route_b = GroupCall(g, groups, G)
    if a_docs == g.D:
        assert _equal(route_a(), route_b()), "the prevalence routes disagree"
    ta, tb = _alternate([route_a, route_b], reps)
    alone, = _alternate([route_b], reps)
    out["prevalence"] = _record((ta[0] * scale, ta[1] * scale), tb, alone)
    words_a = lambda: host_group_words(g, doc_off, words, mask, TOP_N)
    words_b = WordsCall(g, mask, TOP_N)
    assert _equal(words_a(), words_b()), "the word routes disagree"
    ta, tb = _alternate([words_a, words_b], reps)
    alone, = _alternate([words_b], reps)
    out["group_words"] = dict(_record(ta, tb, alone), n=TOP_N, masked_docs=int(mask.sum()),
                              z_bytes_to_host_route_a=4 * g.N, result_bytes_to_host_route_b=8 * g.K * (TOP_N + 1))
    g.subcorpus_release()
    return out


def c1_part(args, K, alpha_sum, beta):
    from ldagibbssampling_amd.corpus import synthetic_changelists
    from ldagibbssampling_amd.sampler import GibbsSampler
    c = synthetic_changelists(num_docs=2000, num_types=5000, seed=1)
    with GibbsSampler(K, c.num_types, c.doc_off, c.words, np.full(K, alpha_sum / K), beta, seed=1) as g:
        g.sweep(args.sweeps)
        out = part(g, c.doc_off, c.words, args.reps, g.D)
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
        return part(g, off, words, args.reps, args.a_docs)


def ab_part(args):
    from ldagibbssampling_amd import capi
    from ldagibbssampling_amd.sampler import GibbsSampler
    lib = capi.load()
    K = 20
    edge = 1
    while lib.lda_group_topics_path(edge + 1, K, 3, None) == 1:
        edge += 1
    out = {"docs": args.ab_docs, "doc_len": 200, "K": K, "thresholds": list(THRESHOLDS), "reps": args.reps,
           "last_lds_groups": edge}
    off, words, z = _shard(K, args.ab_docs, 200, 6)
    with GibbsSampler(K, 1000, off, words, np.full(K, 0.1), 0.01, seed=1, z_init=z) as g:
        g.apply()
        for groups_n in (G, edge, edge + 1):
            groups = np.random.default_rng(4).integers(0, groups_n, g.D).astype(np.int32)
            default = GroupCall(g, groups, groups_n)
            lds = C.c_int32()
            path = lib.lda_group_topics_path(groups_n, K, 3, C.byref(lds))

            def forced():
                lib.lda_debug_group_topics_global(1)
                try:
                    return default()
                finally:
                    lib.lda_debug_group_topics_global(0)
            want = {k: v.copy() for k, v in default().items()}
            assert _equal(forced(), want), "the paths disagree"
            (td, td_min), (tg, tg_min) = _alternate([default, forced], args.reps)
            out[f"G{groups_n}"] = {"default_path": "lds" if path == 1 else "global", "default_lds_bytes": lds.value,
                                   "default_s": td, "default_min_s": td_min, "global_atomics_s": tg,
                                   "global_atomics_min_s": tg_min, "global_over_default": tg / td}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=("c1", "big", "ab"), help="one part only")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--big-docs", type=int, default=200_000)
    ap.add_argument("--a-docs", type=int, default=5_000, help="prevalence route (a)'s documents on the big shard")
    ap.add_argument("--ab-docs", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_topics", "latency.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("group_topics_latency.py needs an MI355X")
    rec = {"tool": "group_topics_latency", "device": torch.cuda.get_device_name(0)}
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
