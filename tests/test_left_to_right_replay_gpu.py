"""GPU checks of every draw of lda_left_to_right (k_left_to_right), at every
instantiation C = Kp / 64 = 1 .. 64, beside test_left_to_right_gpu.py, whose
samplers, documents and helpers these tests share:

  * that module's every-draw check without resampling at the three C it does
    not reach (4, 16, 64), each with K short of Kp, so that some lanes hold
    padding topics only and one lane holds the boundary;
  * with resampling, at every C, the whole chain of every (document,
    particle) replayed in numpy with the device's uniforms
    (ltr_replay_numpy.replay_particle).

Tolerances (derived, not tuned), as in test_left_to_right_gpu.py, whose bound
is stated for K <= 1500: the prefixes and the particle sum add K <= 3000
(R <= 16) positive terms, a relative error of at most (K + 8) 2^-53 < 3.4e-13
in any summation order, so p_r, phat and doc_ll stay held to 1e-11 relative
and a drawn topic's prefix interval is widened by 1e-12 W.  The replayed
chains need no such widening: the replay's own margin, at least 1e-10 W
against a prefix error of at most (Kp + 8) 2^-53 W <= 4.6e-13 W, says that
every draw has one outcome in any summation order.
"""
import numpy as np
import pytest

import ltr_numpy as N
import ltr_replay_numpy as P
import test_left_to_right_gpu as T

pytestmark = pytest.mark.gpu
MORE = {
    # K: (V, sampler, alpha); C = Kp / 64 = 4, 16, 64 with K short of Kp: lanes
    # of padding topics only (from lane 50, 63 and 47 on) and, at K = 1000 and
    # 3000, one lane that holds both kinds
    200: (150, "dense", lambda K: 0.03 + 0.2 * ((7 * np.arange(K)) % 11) / 11),
    1000: (100, "dense", lambda K: 0.02 + 0.3 * np.arange(K)[::-1] / K),
    3000: (60, "sparse", lambda K: 0.01 + 0.05 * (np.arange(K) % 5)),
}
CONFIGS = {**T.CONFIGS, **MORE}
KP_OVER_64 = {3: 1, 20: 1, 100: 2, 512: 8, 1500: 32, 200: 4, 1000: 16, 3000: 64}
_cache = {}


def _shard(K):
    """test_left_to_right_gpu's sampler of K where it has one, else one made
    the same way: after 3 sweeps, with its counts and phi (fetched once,
    shared, never changed)."""
    if K in T.CONFIGS:
        return T._shard(K)
    if K not in _cache:
        from ldagibbssampling_amd.sampler import GibbsSampler
        V, sampler, alpha = MORE[K]
        c = T._train_corpus(V)
        g = GibbsSampler(K, V, c.doc_off, c.words, alpha(K), T.BETA, seed=9, sampler=sampler)
        g.sweep(3)
        nw, nwsum, _, _ = g.counts()
        phi = N.phi_table(nw, nwsum, T.BETA)
        for a in (nw, phi):
            a.setflags(write=False)
        _cache[K] = (g, alpha(K), nw, phi)
    return _cache[K]


def test_configurations_reach_every_instantiation():
    assert set(CONFIGS) == set(KP_OVER_64) and sorted(KP_OVER_64.values()) == [1, 1, 2, 4, 8, 16, 32, 64]
    assert sum(len(set(np.round(a(K), 12))) > 1 for K, (_, _, a) in MORE.items()) >= 2


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("K", list(MORE))
def test_every_draw_without_resampling(K, R, oracle):
    """test_left_to_right_gpu.test_every_draw_without_resampling, on its
    documents, at the K of MORE."""
    g, alpha, nw, phi = _shard(K)
    assert g.Kp // 64 == KP_OVER_64[K]
    off, words = T._held_docs(g.V, 7 + K)
    skip = N.skipped(nw, words)
    seed = 1234 + K
    doc_ll, total, tokens, tp, z = g.left_to_right(off, words, R, False, seed=seed, token_prob=True, z=True)
    assert z.shape == (R, len(words)) and tokens == int((~skip).sum()) and total == T._ordered_sum(doc_ll)
    assert np.all(z[:, skip] == -1) and np.all((z[:, ~skip] >= 0) & (z[:, ~skip] < K))
    # p_r[i] from the topics before i (final once drawn), hence phat and doc_ll
    ref = T._phat_from_z(phi, alpha, off, words, skip, z)
    np.testing.assert_allclose(tp, ref, rtol=1e-11, atol=0.0)
    for d in range(len(off) - 1):
        r = ref[off[d]:off[d + 1]]
        ll = float(np.sum(np.log(r[r > 0])))
        assert abs(doc_ll[d] - ll) <= 1e-11 * abs(ll), d
    # each drawn topic's prefix interval holds u W
    worst = 0.0
    for r in range(R):
        for d in range(len(off) - 1):
            nd = np.zeros(K)
            for i in range(off[d], off[d + 1]):
                if skip[i]:
                    continue
                pre = np.cumsum(N.weights(phi, alpha, nd, words[i]))
                W, k = pre[-1], z[r, i]
                t = N.uniform(seed, int(i), int(i - off[d]), r) * W
                lo = pre[k - 1] if k else 0.0
                assert lo - 1e-12 * W <= t, (r, d, i)
                assert t < pre[k] + 1e-12 * W, (r, d, i)
                worst = max(worst, (lo - t) / W, (t - pre[k]) / W)
                nd[k] += 1
    print(f"K={K} R={R}: the worst excursion of u W out of its interval {worst:.3e} W")


# --------------------------------------------------- the whole chain, replayed
CHAIN_LENGTHS = (0, 1, 2, 5, 63, 64, 65, 129, 130)
CHAIN_R = 3
MARGIN_FLOOR = 1e-10


def _chain_docs(V, seed):
    """Held-out documents of CHAIN_LENGTHS, the smallest that cross both
    64-token chunk edges of the resampling pass (chunks at 0, 64 and 128, the
    last with a single token at limit 129), with empty-row types where the
    pass can trip: inside the 5-token document, last in the 64-token one, at
    63 and 64 (the last lane of a chunk and the first of the next) of the 65-
    and the 130-token ones, first and last in the 129-token one; then a
    document of empty-row types only."""
    rng = np.random.default_rng(seed)
    docs = {n: rng.integers(0, V - 2, n).astype(np.int32) for n in CHAIN_LENGTHS}
    docs[5][2] = V - 1
    docs[64][63] = V - 2
    docs[65][[63, 64]] = V - 1, V - 2
    docs[129][[0, 128]] = V - 2, V - 1
    docs[130][[63, 64]] = V - 2, V - 1
    docs = [docs[n] for n in CHAIN_LENGTHS] + [np.array([V - 1, V - 2, V - 1], np.int32)]
    off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return off, np.concatenate(docs).astype(np.int32)


def _chain_seeds(K):
    """(the documents' seed, the call's seed) of test_every_draw_with_resampling."""
    return 300 + K, 4321 + K


def _chain_replay(K, nw, phi, alpha):
    """The held-out documents of K and the replay of every (document,
    particle) chain with the device's uniforms -- token j of document d is
    call-token off[d] + j, its limit the position in the document: (off,
    words, skip, seed, p[D][R, L], z[R, N], the smallest margin)."""
    V = nw.shape[0]
    doc_seed, seed = _chain_seeds(K)
    off, words = _chain_docs(V, doc_seed)
    skip = N.skipped(nw, words)
    z = np.full((CHAIN_R, len(words)), -1)
    p, margin = [], np.inf
    for d in range(len(off) - 1):
        s = slice(off[d], off[d + 1])
        pd = np.zeros((CHAIN_R, off[d + 1] - off[d]))
        for r in range(CHAIN_R):
            u_of = lambda j, i: N.uniform(seed, int(off[d]) + j, i, r)
            pd[r], z[r, s], m = P.replay_particle(phi, alpha, words[s], skip[s], True, u_of)
            margin = min(margin, m)
        p.append(pd)
    return off, words, skip, seed, p, z, margin


@pytest.mark.parametrize("K", list(CONFIGS))
def test_every_draw_with_resampling(K, oracle):
    """Every draw of every resampling pass: with resampling p_r[i] depends on
    every draw made at limit i, so phat at every position and the final z pin
    the whole chain -- the uniform of each draw, the count taken out before it
    and put back after it, the row it read, the hand-over of the topics between
    the 64-token chunks.  Three jobs share one block with an idle fourth wave."""
    g, alpha, nw, phi = _shard(K)
    assert g.Kp // 64 == KP_OVER_64[K]
    off, words, skip, seed, p_ref, z_ref, margin = _chain_replay(K, nw, phi, alpha)
    lens = np.diff(off)
    assert lens.tolist() == list(CHAIN_LENGTHS) + [3]
    where = lambda n: off[CHAIN_LENGTHS.index(n)]
    assert skip[where(129)] and skip[where(129) + 128] and skip[where(64) + 63]
    assert skip[where(65) + 63] and skip[where(65) + 64] and skip[where(130) + 63] and skip[where(130) + 64]
    assert skip[off[-2]:].all() and skip.sum() == 11
    # a condition on the inputs, from the reference alone: no draw so near an
    # edge of its interval that two summation orders may tell it apart
    print(f"K={K}: the smallest margin of {CHAIN_R} x {len(lens)} replayed chains {margin:.3e} W")
    assert margin >= MARGIN_FLOOR, (
        f"K={K}: a draw of the replay sits {margin:.3e} W from an edge of its interval, under "
        f"{MARGIN_FLOOR:g} W: the inputs do not pin the chain, change the seeds in _chain_seeds")
    doc_ll, total, tokens, tp, z = g.left_to_right(off, words, CHAIN_R, True, seed=seed, token_prob=True, z=True)
    assert z.shape == (CHAIN_R, len(words)) and tokens == int((~skip).sum()) and total == T._ordered_sum(doc_ll)
    assert np.all(z_ref[:, skip] == -1) and np.all(z_ref[:, ~skip] >= 0)
    np.testing.assert_array_equal(z, z_ref)
    worst_tp = worst_ll = 0.0
    for d in range(len(lens)):
        s = slice(off[d], off[d + 1])
        phat, ll = N.estimate(p_ref[d])
        assert np.all((phat == 0.0) == skip[s])
        err = np.abs(tp[s] - phat)[~skip[s]] / phat[~skip[s]]
        worst_tp = max(worst_tp, float(err.max()) if len(err) else 0.0)
        worst_ll = max(worst_ll, abs(doc_ll[d] - ll) / abs(ll) if ll else 0.0)
    print(f"K={K}: the worst relative error of token_prob {worst_tp:.3e}, of doc_ll {worst_ll:.3e}")
    for d in range(len(lens)):
        s = slice(off[d], off[d + 1])
        phat, ll = N.estimate(p_ref[d])
        np.testing.assert_allclose(tp[s], phat, rtol=1e-11, atol=0.0, err_msg=f"document {d}")
        assert abs(doc_ll[d] - ll) <= 1e-11 * abs(ll), d
