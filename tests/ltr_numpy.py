"""A numpy restatement of the left-to-right estimator (lda_left_to_right,
Mallet's MarginalProbEstimator.evaluateLeftToRight): the
checker of test_left_to_right*.py.  Everything is fp64 and written for
clarity, one document at a time.

  phi[w, k] = (nw[w, k] + beta) * (1 / (nwsum[k] + V beta))
  a token whose type has no training tokens (nw[w].sum() == 0) is skipped
  a draw with uniform u over weights x: t = u * sum(x); the smallest k whose
  inclusive prefix exceeds t, else the last k with x[k] > 0
"""
import itertools

import numpy as np

STREAM = 3


def phi_table(nw, nwsum, beta):
    nw = np.asarray(nw, np.float64)
    inv = 1.0 / (np.asarray(nwsum, np.float64) + nw.shape[0] * float(beta))
    return (nw + float(beta)) * inv[None, :]


def skipped(nw, doc):
    tot = np.asarray(nw, np.int64).sum(axis=1)
    return np.array([tot[w] == 0 for w in doc], bool)


def uniform(seed, g, limit, r):
    """The device's uniform of the draw of call-token g at limit `limit` in
    particle r (Philox4x32-10 words 0 and 1, 53 bits)."""
    from oracle import oracle
    seed &= 2**64 - 1
    x = oracle.philox4x32_10([g & 0xFFFFFFFF, g >> 32, limit, STREAM | (r << 8)], [seed & 0xFFFFFFFF, seed >> 32])
    return float((x[0] << 21) | (x[1] >> 11)) * 2.0**-53


def weights(phi, alpha, nd, w):
    return (nd + alpha) * phi[w]


def draw(x, u):
    pre = np.cumsum(x)
    hit = np.nonzero(pre > u * pre[-1])[0]
    return int(hit[0]) if len(hit) else int(np.nonzero(x > 0)[0][-1])


def run_particle(phi, alpha, doc, skip, resampling, u_of):
    """One particle: (p[L], z[L]); u_of(j, i) is the uniform of the draw of
    token j at limit i.  Skipped tokens: p = 0, z = -1."""
    L, K = len(doc), phi.shape[1]
    alpha = np.asarray(alpha, np.float64)
    A = float(np.sum(alpha))
    nd = np.zeros(K)
    z = np.full(L, -1)
    p = np.zeros(L)
    so_far = 0
    for i in range(L):
        if resampling:
            for j in range(i):
                if skip[j]:
                    continue
                nd[z[j]] -= 1
                z[j] = draw(weights(phi, alpha, nd, doc[j]), u_of(j, i))
                nd[z[j]] += 1
        if skip[i]:
            continue
        x = weights(phi, alpha, nd, doc[i])
        p[i] = x.sum() / (A + so_far)
        so_far += 1
        z[i] = draw(x, u_of(i, i))
        nd[z[i]] += 1
    return p, z


def estimate(p):
    """(phat[L], doc_ll) of the particles' p[R, L] (0 columns = skipped)."""
    p = np.asarray(p, np.float64)
    s = np.zeros(p.shape[1])
    for r in range(p.shape[0]):
        s = s + p[r]
    phat = s / p.shape[0]
    return phat, float(np.sum(np.log(phat[phat > 0])))


def p_from_z(phi, alpha, doc, skip, z, upto=None):
    """p[i] recomputed from the topics of the tokens before i (valid for every
    i without resampling, for the last scored i with it)."""
    alpha = np.asarray(alpha, np.float64)
    A, K = float(np.sum(alpha)), phi.shape[1]
    nd = np.zeros(K)
    p = np.zeros(len(doc))
    so_far = 0
    for i in range(len(doc)):
        if skip[i]:
            continue
        if upto is None or i == upto:
            p[i] = weights(phi, alpha, nd, doc[i]).sum() / (A + so_far)
        so_far += 1
        nd[z[i]] += 1
    return p


def exact(phi, alpha, doc, skip, resampling):
    """The algorithm's Markov chain over the assignments, enumerated: per
    position (E[p_r[i]], lo_i, hi_i) -- None for a skipped one -- and, for the
    chain without resampling, the marginal p(w) = E[prod_i p_r[i]]."""
    alpha = np.asarray(alpha, np.float64)
    A, K = float(np.sum(alpha)), phi.shape[1]
    kept = [i for i in range(len(doc)) if not skip[i]]

    def nd_of(state):
        nd = np.zeros(K)
        for k in state:
            nd[k] += 1
        return nd

    dist = {(): 1.0}          # assignment of the kept tokens so far -> probability
    out = [None] * len(doc)
    for n, i in enumerate(kept):
        if resampling:
            for j in range(n):
                new = {}
                for state, pr in dist.items():
                    nd = nd_of(state)
                    nd[state[j]] -= 1
                    x = weights(phi, alpha, nd, doc[kept[j]])
                    x = x / x.sum()
                    for k in range(K):
                        s2 = state[:j] + (k,) + state[j + 1:]
                        new[s2] = new.get(s2, 0.0) + pr * x[k]
                dist = new
        vals, new = [], {}
        mean = 0.0
        for state, pr in dist.items():
            x = weights(phi, alpha, nd_of(state), doc[i])
            W = x.sum()
            pi = W / (A + n)
            vals.append(pi)
            mean += pr * pi
            for k in range(K):
                new[state + (k,)] = new.get(state + (k,), 0.0) + pr * x[k] / W
        dist = new
        out[i] = (mean, min(vals), max(vals))
    marginal = 0.0
    for state in itertools.product(range(K), repeat=len(kept)):
        nd = np.zeros(K)
        t = 1.0
        for n, (i, k) in enumerate(zip(kept, state)):
            t *= (nd[k] + alpha[k]) * phi[doc[i], k] / (A + n)
            nd[k] += 1
        marginal += t
    return out, marginal
