"""Every sampler kernel family's draws against LDA's conditional in float64,
through GibbsSampler alone: no oracle on this side.  The corpora, references
and bars are draw_conditional_numpy's; test_draw_conditional.py runs the same
cases (K <= 1500) through cpu_exact and shows that a reference with one term
broken fails these bars.  Each test prints the lines its CPU twin prints:
kernels and cpu_exact are bit-exact, so the figures must be equal.

Sizes (MI355X): the module takes 12 s, its slowest case 1.8 s; design B's
round trip is timed and printed by the test itself (test_replay)."""
import time

import numpy as np
import pytest

import draw_conditional_numpy as DC

pytestmark = pytest.mark.gpu


def _sampler(case, monkeypatch):
    from ldagibbssampling_amd.sampler import GibbsSampler
    if case.family in ("half", "full"):
        monkeypatch.setenv("LDA_DENSE_HALF", str(case.half))
    else:
        monkeypatch.delenv("LDA_DENSE_HALF", raising=False)      # the library's own choice
    return GibbsSampler(case.K, case.V, case.doc_off, case.words, case.alpha, case.beta, seed=case.seed,
                        z_init=case.z0, tokens_per_range=case.tokens_per_range, sampler=case.kind)


def _assert_ok(title, reports):
    for name, r in reports.items():
        print(f"{title} [{name}] {r.figures()}")
    bad = {name: r.failures for name, r in reports.items() if not r.ok}
    assert not bad, (title, bad)


@pytest.mark.parametrize("c", DC.replica_cases(saturated=True), ids=DC.case_id)
def test_replicas(monkeypatch, c):
    """Design A: the first tokens of n identical documents after one sweep."""
    case = DC.replica_case(c[1], c[0], symmetric=c[2], tokens_per_range=c[3], saturated=c[4])
    with _sampler(case, monkeypatch) as g:
        g.sweep(1)
        z1 = g.z()
    title = f"A {DC.case_id(c)}"
    print(f"{title}: {len(case.words)} tokens, V = {case.V}")
    _assert_ok(title, DC.replica_reports(case, z1))


@pytest.mark.parametrize("f,K,update", DC.REPLAY_CASES, ids=lambda v: str(v))
def test_replay(monkeypatch, f, K, update):
    """Design B: one sweep of the six-token corpus replayed DC.REPLAYS times in
    one context (set_z re-seeds the counts; sweep(1) applies them, samples and
    applies), against the exact joint law of each document.  Any failing call
    raises and ends the loop.  Measured on an MI355X: 72-78 us per replay in
    the dense families (recount 76-97), 91-102 sparse, 111 / 129 at K = 1500 /
    4096, so n = 4000 (the starting size; 2000 is the floor) costs 0.3-0.5 s."""
    case = DC.replay_case(K, f)
    zs = np.empty((DC.REPLAYS, len(case.z0)), np.int32)
    with _sampler(case, monkeypatch) as g:
        g.set_count_update(update)
        t0 = time.perf_counter()
        for i in range(DC.REPLAYS):
            g.set_z(case.z0)
            g.sweep_index = i
            g.sweep(1)
            zs[i] = g.z()
        dt = time.perf_counter() - t0
        assert g.recount == (update == "recount")
    print(f"B {f}-K{K} {update}: {1e6 * dt / DC.REPLAYS:.0f} us per replay, {dt:.2f} s")
    _assert_ok(f"B {f}-K{K}", DC.replay_reports(case, zs))


@pytest.mark.parametrize("f,K", DC.FROZEN_CASES, ids=lambda v: str(v))
def test_frozen(monkeypatch, f, K):
    """Design C: the frozen kernels through infer, on one-token documents of
    the most frequent word and of a word with one training token."""
    case = DC.frozen_case(K, f)
    with _sampler(case, monkeypatch) as g:
        g.sweep(3)
        z = g.z()
        nw, nwsum, _, _ = g.counts()
        ref = np.zeros((case.V, case.K), np.int64)
        np.add.at(ref, (case.words, z), 1)
        np.testing.assert_array_equal(nw, ref)
        np.testing.assert_array_equal(nwsum, ref.sum(0))
        reports = {}
        n = DC.FROZEN_DOCS
        for i, w in enumerate(DC.frozen_words(case, z)):
            theta = g.infer(np.arange(n + 1, dtype=np.int64), np.full(n, w, np.int32), n_iter=1, burn_in=0,
                            thin=1, seed=11 + i)
            p, groups = DC.frozen_reference(case, ref, ref.sum(0), w)
            reports[f"word {w}"] = DC.check_draws(DC.theta_topics(theta, case.alpha), p, groups)
    _assert_ok(f"C {f}-K{K}", reports)
