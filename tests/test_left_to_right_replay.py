"""The replaying restatement (tests/ltr_replay_numpy.py, the checker of
test_left_to_right_replay_gpu.py) against the restatement itself, without a
device: on test_left_to_right.py's tiny model it is ltr_numpy.run_particle
bit for bit, and its margin is right on weights made by hand."""
import numpy as np
import pytest

import ltr_numpy as N
import ltr_replay_numpy as P
from test_left_to_right import ALPHA, BETA, DOC, NW


@pytest.mark.parametrize("resampling", [False, True])
def test_replay_is_the_restated_sampler(resampling):
    """replay_particle: run_particle's p and z bit for bit for the same
    uniforms, and a margin that is the smallest of its draws' own."""
    phi = N.phi_table(NW, NW.sum(0), BETA)
    skip = N.skipped(NW, DOC)
    L = len(DOC)
    for s in range(20):
        u = np.random.default_rng(100 + s).random((L, L))
        u_of = lambda j, i: u[j, i]
        p0, z0 = N.run_particle(phi, ALPHA, DOC, skip, resampling, u_of)
        asked = []

        def seen(j, i):
            asked.append((j, i))
            return u[j, i]

        p, z, margin = P.replay_particle(phi, ALPHA, DOC, skip, resampling, seen)
        assert p.tobytes() == p0.tobytes() and z.tolist() == z0.tolist()
        # one uniform per draw: token j at its own limit, and with resampling at every later scored limit
        want = []
        for i in range(L):
            if resampling:
                want += [(j, i) for j in range(i) if not skip[j]]
            if not skip[i]:
                want.append((i, i))
        assert asked == want
        assert 0.0 < margin <= 0.5
    # no draw at all: nothing bounds the margin
    p, z, margin = P.replay_particle(phi, ALPHA, [4, 4], [True, True], resampling, u_of)
    assert p.tolist() == [0.0, 0.0] and z.tolist() == [-1, -1] and margin == np.inf


def test_replay_margin_on_known_weights():
    """Prefixes 0, 2, 2, 3, 3 of W = 3 (the example of
    test_restatement_draw_and_skip): t = 1.5 is 0.5 from topic 1's upper edge
    and 1.5 from its lower one; t = 2.25 is 0.25 above topic 3's lower edge."""
    x = np.array([0.0, 2.0, 0.0, 1.0, 0.0])
    assert P.draw_margin(x, 0.5) == (1, 0.5 / 3.0)
    assert P.draw_margin(x, 0.75) == (3, 0.25 / 3.0)
    assert P.draw_margin(x, 0.125) == (1, 0.375 / 3.0)
    k, m = P.draw_margin(x, 2.0 / 3.0 - 2.0 ** -40)
    assert k == 1 and abs(m - 2.0 ** -40) <= 2.0 ** -52
    for u in (0.0, 0.5, 0.66, 0.67, 0.999, 1.0):
        assert P.draw_margin(x, u)[0] == N.draw(x, u)
    assert P.draw_margin(x, 0.0)[1] == 0.0          # on the lower edge of the first positive weight
    # one topic, one token: the replay's margin is that draw's
    phi = np.array([[0.25, 0.5, 0.25]])
    alpha = np.array([1.0, 2.0, 1.0])               # weights 0.25, 1, 0.25: prefixes 0.25, 1.25, 1.5
    p, z, margin = P.replay_particle(phi, alpha, [0], [False], True, lambda j, i: 0.25)
    assert z.tolist() == [1] and p[0] == 1.5 / 4.0 and margin == (0.375 - 0.25) / 1.5
