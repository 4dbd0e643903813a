#!/usr/bin/env python3
"""Latency of prediction scoring (run by hand on the GPU; not bench.py).

1. The C1 changelist corpus (2000 documents) at the reference's cmu_ron
   settings (K = 500) is trained for a few sweeps, then Q = 16 changelists are
   scored against every training document two ways:
     (a) the public route before lda_score_docs: getSampledDistributions, then
         getTopicProbabilities(d) for each d, then a numpy cosine;
     (b) TopicInferencer.scoreInstances (one native call).
   Both include the inference; the scoring halves are also timed alone.
2. GibbsSampler.score_docs alone on a synthetic shard (default 1e6 documents x
   200 tokens, K = 512, Q = 16): documents x queries per second and bytes of z
   read per second (4 bytes per token per query tile).  The call includes the
   upload of theta and the copy of the Q x D scores to the host; Q = 1 is
   timed as well, where that copy is 16x smaller.

Writes one JSON line to profiles/score/score_latency.json (and prints it).
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


def _timed(fn, reps):
    """Median and minimum wall time of fn() (every fn ends in a device wait)."""
    fn()                                    # warm: code objects, scratch growth
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), float(np.min(t))


def changelist_part(args):
    from ldagibbssampling_amd import topic_model as tm
    from ldagibbssampling_amd.corpus import synthetic_changelists

    K, Q = args.k_model, args.queries
    c = synthetic_changelists(num_docs=args.model_docs, num_types=5000, seed=1)
    il = tm.InstanceList.fromCorpus(c)
    m = tm.ParallelTopicModel(K, 100.0, 1.0)
    m.setRandomSeed(3)
    m.setTopicDisplay(0, 0)
    m.setOptimizeInterval(0)
    m.setNumIterations(args.sweeps)
    m.addInstances(il)
    m.estimate()
    D = c.num_docs
    held = synthetic_changelists(num_docs=Q, num_types=5000, seed=2)
    held = [tm.Instance(held.doc(d)) for d in range(Q)]
    inf = m.getInferencer()

    def cosine_host(theta):
        p = np.stack([m.getTopicProbabilities(d) for d in range(D)])
        return (theta @ p.T) / (np.linalg.norm(theta, axis=1)[:, None] * np.linalg.norm(p, axis=1)[None, :])

    def route_a():
        return cosine_host(inf.getSampledDistributions(held, 100, 10, 10, seed=7))

    def route_b():
        return inf.scoreInstances(held, 100, 10, 10, seed=7)[0]

    ref, got = route_a(), route_b()
    err = float(np.max(np.abs(got - ref) / np.abs(ref)))
    theta = inf.getSampledDistributions(held, 100, 10, 10, seed=7)
    a_med, a_min = _timed(route_a, args.reps)
    b_med, b_min = _timed(route_b, args.reps)
    a2_med, _ = _timed(lambda: cosine_host(theta), args.reps)
    b2_med, _ = _timed(lambda: m.scoreDistributions(theta), args.reps)
    m.close()
    return {
        "model": {"docs": D, "tokens": c.num_tokens, "K": K, "sweeps": args.sweeps, "queries": Q},
        "a_infer_then_probabilities_numpy_s": a_med, "a_min_s": a_min,
        "b_score_instances_s": b_med, "b_min_s": b_min,
        "b_faster_than_a": b_med < a_med, "a_over_b": a_med / b_med,
        "a_scoring_only_s": a2_med, "b_scoring_only_s": b2_med, "scoring_only_a_over_b": a2_med / b2_med,
        "max_rel_diff_a_vs_b": err,
    }


def shard_part(args):
    from ldagibbssampling_amd.sampler import GibbsSampler

    D, L, K, V = args.shard_docs, args.shard_len, args.k_shard, 2000
    rng = np.random.default_rng(5)
    off = np.arange(D + 1, dtype=np.int64) * L
    words = rng.integers(0, V, D * L, dtype=np.int32)
    # topics as after training: each document draws from a few topics
    own = rng.integers(0, K, (D, 8), dtype=np.int32)
    z = np.take_along_axis(own, rng.integers(0, 8, (D, L)), axis=1).reshape(-1).astype(np.int32)
    out = {"docs": D, "doc_len": L, "K": K, "tokens": D * L}
    with GibbsSampler(K, V, off, words, np.full(K, 0.1), 0.01, seed=1, z_init=z) as g:
        g.apply()
        for Q in (args.queries, 1):
            theta = np.ascontiguousarray(rng.dirichlet(np.full(K, 0.1), Q))
            med, mn = _timed(lambda: g.score_docs(theta), args.reps)
            tiles = -(-Q // 16)
            out[f"q{Q}"] = {
                "call_s": med, "call_min_s": mn,
                "doc_queries_per_s": D * Q / med,
                "z_bytes_per_s": 4.0 * D * L * tiles / med,
                "scores_bytes_to_host": 8 * D * Q,
            }
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model-docs", type=int, default=2000)
    ap.add_argument("--k-model", type=int, default=500)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--shard-docs", type=int, default=1_000_000)
    ap.add_argument("--shard-len", type=int, default=200)
    ap.add_argument("--k-shard", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-shard", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score", "score_latency.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("score_latency.py needs an MI355X")
    rec = {"tool": "score_latency", "device": torch.cuda.get_device_name(0),
           "changelists": changelist_part(args)}
    if not args.skip_shard:
        rec["shard"] = shard_part(args)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
