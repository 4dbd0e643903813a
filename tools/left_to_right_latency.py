#!/usr/bin/env python3
"""Wall time of GibbsSampler.left_to_right (lda_left_to_right):
medians of --reps calls after one warm call, with and without resampling,
--particles particles, on
  small: the held-out set of tests/test_perplexity.py (K = 100, 220 whole
         documents) against a model trained --sweeps sweeps on its training set;
  big:   a synthetic shard, V = 1e5, K = 512, 1e4 held-out documents x 100
         tokens (the model's topics as after training, as heldout_latency.py).
Beside the times: the per-token log likelihood of both modes and, reported and
not asserted, that of doc_completion (lda_infer 100, 10, 10, seed 7) on the
same model and documents (its scored halves only).

  python tools/left_to_right_latency.py [--only small|big] [--out FILE]
writes profiles/left_to_right/latency.json.
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

INFER = dict(n_iter=100, thin=10, burn_in=10, seed=7)


def _measure(g, held, obs, sc, args):
    """held: (doc_off, words) of the whole held-out documents; obs / sc their
    document-completion halves."""
    lens = np.diff(held[0])
    out = {"held_docs": len(lens), "tokens": int(lens.sum()), "longest_document": int(lens.max()),
           "K": g.K, "Kp": g.Kp, "V": g.V, "particles": args.particles, "reps": args.reps,
           "draws_per_particle": {"no_resampling": int(lens.sum()),
                                  "resampling": int((lens * (lens + 1) // 2).sum())}}
    for name, resampling in (("no_resampling", False), ("resampling", True)):
        call = lambda: g.left_to_right(held[0], held[1], args.particles, resampling, seed=7)
        _, total, scored = call()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            t.append(time.perf_counter() - t0)
            print(f"  {name}: {t[-1]:.4f} s", flush=True)
        out[name] = {"median_s": float(np.median(t)), "min_s": float(np.min(t)), "log_likelihood": total,
                     "tokens_scored": scored, "ll_per_token": total / scored}
    _, ll_dc = g.doc_completion(obs[0], obs[1], sc[0], sc[1], **INFER)
    n_sc = int(sc[0][-1] - sc[0][0])
    out["doc_completion"] = {"log_likelihood": ll_dc, "tokens_scored": n_sc, "ll_per_token": ll_dc / n_sc,
                             "note": "scores the second half of each document given the first; reported, not asserted"}
    return out


def small_part(args):
    from ldagibbssampling_amd.corpus import document_completion_split, synthetic_lda
    from ldagibbssampling_amd.sampler import GibbsSampler
    K = 100
    c = synthetic_lda(num_docs=2200, num_types=3000, num_topics=K, doc_len=None, mean_len=80, min_len=10,
                      max_len=300, seed=20261015, k_true=min(K, 50))
    perm = np.random.default_rng(0).permutation(c.num_docs)
    n_held = c.num_docs // 10
    train, held = c.subset(np.sort(perm[n_held:])), c.subset(np.sort(perm[:n_held]))
    obs, sc = document_completion_split(held)
    with GibbsSampler(K, c.num_types, train.doc_off, train.words, np.full(K, 10.0 / K), 0.01, seed=1) as g:
        g.sweep(args.sweeps)
        out = _measure(g, (held.doc_off, held.words), (obs.doc_off, obs.words), (sc.doc_off, sc.words), args)
    out["train"] = {"docs": train.num_docs, "tokens": train.num_tokens, "sweeps": args.sweeps}
    return out


def big_part(args):
    from ldagibbssampling_amd.corpus import Corpus, document_completion_split
    from ldagibbssampling_amd.sampler import GibbsSampler
    V, K, L, D, Dh = 100000, 512, 100, args.big_train_docs, args.big_held_docs
    rng = np.random.default_rng(5)
    off = np.arange(D + 1, dtype=np.int64) * L
    words = rng.integers(0, V, D * L, dtype=np.int32)
    # topics as after training: each document draws from a few topics
    own = rng.integers(0, K, (D, 8), dtype=np.int32)
    z = np.take_along_axis(own, rng.integers(0, 8, (D, L)), axis=1).reshape(-1).astype(np.int32)
    held = Corpus(np.arange(Dh + 1, dtype=np.int64) * L, rng.integers(0, V, Dh * L, dtype=np.int32), V)
    obs, sc = document_completion_split(held)
    with GibbsSampler(K, V, off, words, np.full(K, 0.1), 0.01, seed=1, z_init=z) as g:
        g.apply()
        out = _measure(g, (held.doc_off, held.words), (obs.doc_off, obs.words), (sc.doc_off, sc.words), args)
    out["train"] = {"docs": D, "tokens": D * L}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=("small", "big"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--particles", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=100)
    ap.add_argument("--big-train-docs", type=int, default=100000)
    ap.add_argument("--big-held-docs", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "left_to_right", "latency.json"))
    args = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0)}
    if os.path.exists(args.out) and args.only:
        res.update(json.load(open(args.out)))     # the other part stays
    for name, part in (("small", small_part), ("big", big_part)):
        if args.only in (None, name):
            print(name, flush=True)
            res[name] = part(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
