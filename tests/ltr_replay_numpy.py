"""The replay of ltr_numpy.run_particle that reports its own margin: the
checker of test_left_to_right_replay*.py.  Plain fp64 numpy, like ltr_numpy,
whose weights and draw rule it restates draw for draw.

  margin of a draw = min(t - prefix[k - 1], prefix[k] - t) / W, prefix[-1] = 0:
  how far t = u W sat from the nearer edge of the drawn topic's interval
"""
import numpy as np

from ltr_numpy import weights


def draw_margin(x, u):
    """(k, margin) of a draw: k as ltr_numpy.draw(x, u), margin = how far
    t = u W sat from the nearer edge of k's prefix interval, min(t - prefix[k -
    1], prefix[k] - t) / W with prefix[-1] = 0 (negative for the fall-back to
    the last positive weight, whose prefix does not exceed t)."""
    pre = np.cumsum(x)
    W = pre[-1]
    t = u * W
    hit = np.nonzero(pre > t)[0]
    k = int(hit[0]) if len(hit) else int(np.nonzero(x > 0)[0][-1])
    lo = pre[k - 1] if k else 0.0
    return k, float(min(t - lo, pre[k] - t) / W)


def replay_particle(phi, alpha, doc, skip, resampling, u_of):
    """run_particle that reports its own margin: (p[L], z[L], margin), p and
    z exactly ltr_numpy.run_particle's for the same uniforms, margin the
    smallest draw_margin over every draw of the run (inf without a draw).  Two
    summation orders of the same positive weights agree on every prefix to
    (K + 8) 2^-53 W, so a run whose margin exceeds that has one outcome in
    any order."""
    L, K = len(doc), phi.shape[1]
    alpha = np.asarray(alpha, np.float64)
    A = float(np.sum(alpha))
    nd = np.zeros(K)
    z = np.full(L, -1)
    p = np.zeros(L)
    so_far = 0
    margin = np.inf
    for i in range(L):
        if resampling:
            for j in range(i):
                if skip[j]:
                    continue
                nd[z[j]] -= 1
                z[j], m = draw_margin(weights(phi, alpha, nd, doc[j]), u_of(j, i))
                margin = min(margin, m)
                nd[z[j]] += 1
        if skip[i]:
            continue
        x = weights(phi, alpha, nd, doc[i])
        p[i] = x.sum() / (A + so_far)
        so_far += 1
        z[i], m = draw_margin(x, u_of(i, i))
        margin = min(margin, m)
        nd[z[i]] += 1
    return p, z, float(margin)
