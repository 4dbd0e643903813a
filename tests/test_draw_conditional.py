"""CPU half of the draw-conditional tests: the helper tested against numpy's
own sampler, every case with K <= 1500 through cpu_exact (the same corpora,
seeds and bars as test_draw_conditional_gpu.py, whose kernels are bit-exact
with it), and the proof that the bars discriminate: a reference with one term
of the conditional broken fails them on the template built for that term.

Each test prints its figures; for K <= 1500 the GPU module prints the same
lines from the kernels' draws (run both with -s to compare)."""
import numpy as np
import pytest

import draw_conditional_numpy as DC

CPU_MAX_K = 1500
A_CASES = [c for c in DC.replica_cases(saturated=False) if c[1] <= CPU_MAX_K]


def _sampler(oracle, case, z0=None):
    return oracle.ExactSampler(case.K, case.V, case.doc_off, case.words, case.alpha, case.beta, case.seed,
                               z_init=case.z0 if z0 is None else z0, kind=case.kind,
                               half=0 if case.half is None else case.half)


def _sweep_once(oracle, case):
    o = _sampler(oracle, case)
    o.sweep(1)
    return o.z()


def _replay(oracle, case, n):
    zs = np.empty((n, len(case.z0)), np.int32)
    for i in range(n):
        o = _sampler(oracle, case)
        o.apply()
        o.sweep_index = i
        o.sample()
        zs[i] = o.z()
    return zs


def _infer_word(oracle, o, case, w, n, seed):
    theta = o.infer(np.arange(n + 1, dtype=np.int64), np.full(n, w, np.int32), n_iter=1, burn_in=0, thin=1,
                    seed=seed)
    return DC.theta_topics(theta, case.alpha)


_memo = {}


def _replica_run(oracle, c):
    """(case, z after one sweep), computed once per case and left unchanged."""
    if c not in _memo:
        case = DC.replica_case(c[1], c[0], symmetric=c[2], tokens_per_range=c[3], saturated=c[4])
        _memo[c] = (case, _sweep_once(oracle, case))
    return _memo[c]


def _show(title, reports):
    for name, r in reports.items():
        print(f"{title} [{name}] {r.figures()}")


def _assert_ok(title, reports):
    _show(title, reports)
    bad = {name: r.failures for name, r in reports.items() if not r.ok}
    assert not bad, (title, bad)


# ------------------------------------------------------------------ helper
@pytest.mark.parametrize("c", A_CASES, ids=DC.case_id)
def test_statistic_accepts_true_draws(c):
    """numpy's own draws from the reference pass the bars on every template."""
    case = DC.replica_case(c[1], c[0], symmetric=c[2], tokens_per_range=c[3])
    # (seed [K, 1]: with seed K, K = 1500 symmetric drew chi2 = 16.6 at dof 3 on template 2, which
    # the chi2_3 tail allows once in 1100 draws and this module makes some 300)
    rng = np.random.default_rng([c[1], 1])
    for tpl in case.templates:
        p, groups = DC.replica_reference(case, tpl)
        r = DC.check_draws(rng.choice(case.K, len(tpl.tok0), p=p), p, groups)
        assert r.ok, (tpl.name, r.failures, r.figures())


def test_statistic_accepts_true_draws_replay_and_frozen():
    rng = np.random.default_rng(8)
    for f, K, _ in DC.REPLAY_CASES:
        if K > CPU_MAX_K:
            continue
        case = DC.replay_case(K, f)
        for d in range(2):
            p, groups = DC.replay_reference(case, d)
            r = DC.check_counts(rng.multinomial(DC.REPLAYS, p), p, groups)
            assert r.ok, (f, K, d, r.failures)


def test_statistic_rejects_and_pools():
    """A shifted law fails both bars; draws in cells that expect nothing fail
    the pooled-cell rule; a drawn topic >= K is refused."""
    rng = np.random.default_rng(1)
    p = np.array([0.5, 0.3, 0.2 - 1e-4, 1e-4])
    q = np.array([0.45, 0.35, 0.2 - 1e-4, 1e-4])
    r = DC.check_draws(rng.choice(4, 8192, p=q), p, {"first": [0]})
    assert len(r.failures) == 2
    obs = np.array([4000, 2400, 1570, 30])
    assert any("together expect" in f for f in DC.check_counts(obs, p).failures)
    with pytest.raises(AssertionError):
        DC.check_draws(np.array([0, 4]), p)


def test_replay_reference_is_a_distribution_of_sequential_gibbs():
    """The enumeration against a straightforward simulation of sequential
    Gibbs on the same snapshot (numpy's generator, 40000 runs)."""
    case = DC.replay_case(5, "quarter")
    rng = np.random.default_rng(3)
    nw = np.zeros((case.V, case.K), np.int64)
    np.add.at(nw, (case.words, case.z0), 1)
    nwsum = nw.sum(0)
    n = 40000
    zs = np.empty((n, 6), np.int64)
    for r in range(n):
        z = case.z0.copy()
        for d in range(2):
            lo, hi = case.doc_off[d], case.doc_off[d + 1]
            for i in range(lo, hi):
                nd = np.bincount(z[lo:hi], minlength=case.K)
                z[i] = rng.choice(case.K, p=DC.conditional(nd, nw[case.words[i]], nwsum, case.alpha, case.beta,
                                                           case.V, int(z[i])))
        zs[r] = z
    reports = DC.replay_reports(case, zs)
    assert all(r.ok for r in reports.values()), {k: r.failures for k, r in reports.items()}


# ------------------------------------------------------ the cases on cpu_exact
@pytest.mark.parametrize("c", A_CASES, ids=DC.case_id)
def test_replicas_cpu_exact(oracle, c):
    case, z1 = _replica_run(oracle, c)
    _assert_ok(f"A {DC.case_id(c)}", DC.replica_reports(case, z1))


@pytest.mark.parametrize("f,K,update", [c for c in DC.REPLAY_CASES if c[1] <= CPU_MAX_K and c[2] == "delta"],
                         ids=lambda v: str(v))
def test_replay_cpu_exact(oracle, f, K, update):
    """cpu_exact has one count update (the two GPU modes are bit-identical)."""
    case = DC.replay_case(K, f)
    _assert_ok(f"B {f}-K{K}", DC.replay_reports(case, _replay(oracle, case, DC.REPLAYS)))


def _frozen_run(oracle, f, K):
    case = DC.frozen_case(K, f)
    o = _sampler(oracle, case)
    o.sweep(3)
    z = o.z()
    nw, nwsum, _, _ = o.counts()
    ref = np.zeros((case.V, case.K), np.int64)
    np.add.at(ref, (case.words, z), 1)
    np.testing.assert_array_equal(nw, ref)
    np.testing.assert_array_equal(nwsum, ref.sum(0))
    draws = {w: _infer_word(oracle, o, case, w, DC.FROZEN_DOCS, seed=11 + i)
             for i, w in enumerate(DC.frozen_words(case, z))}
    return case, ref, z, draws


@pytest.mark.parametrize("f,K", [c for c in DC.FROZEN_CASES if c[1] <= CPU_MAX_K], ids=lambda v: str(v))
def test_frozen_cpu_exact(oracle, f, K):
    case, nw, _, draws = _frozen_run(oracle, f, K)
    reports = {}
    for w, zs in draws.items():
        p, groups = DC.frozen_reference(case, nw, nw.sum(0), w)
        reports[f"word {w}"] = DC.check_draws(zs, p, groups)
    _assert_ok(f"C {f}-K{K}", reports)


# ------------------------------------------------------- the bars discriminate
VISIBLE = [("quarter", 20), ("full", 100), ("dense", 300), ("sparse", 300), ("big", 1500)]


@pytest.mark.parametrize("f,K", VISIBLE, ids=lambda v: str(v))
def test_each_term_is_visible(oracle, f, K):
    """Against cpu_exact's draws, a reference with one term broken misses the
    bars on the template meant for it (and the true one passes, above)."""
    c = next(c for c in A_CASES if c[0] == f and c[1] == K and not c[2])
    case, z1 = _replica_run(oracle, c)
    tpl = {t.name[0]: t.name for t in case.templates}

    def fails(what, names, **ref):
        reports = DC.replica_reports(case, z1, **ref)
        for nm in names:
            print(f"{f}-K{K} {what} [{tpl[nm]}] {reports[tpl[nm]].figures()} -> {reports[tpl[nm]].failures}")
            assert not reports[tpl[nm]].ok, (what, tpl[nm], reports[tpl[nm]].figures())

    fails("no nw-1", "12", corr=("nd", "nwsum"))
    fails("no nd-1", "2", corr=("nw", "nwsum"))
    fails("beta x 1.5", "7", beta=1.5 * case.beta)
    a = case.alpha.copy()
    a[K - 1] = 0.0
    fails("alpha[K-1] = 0", "6", alpha=a)
    fails("frozen formula on a training token", "2", corr=DC.FROZEN)


@pytest.mark.parametrize("f,K", [("quarter", 3), ("sparse", 5), ("dense", 300), ("big", 1500)], ids=lambda v: str(v))
def test_nwsum_term_is_visible(oracle, f, K):
    """Design B sees nwsum - 1, which design A cannot."""
    case = DC.replay_case(K, f)
    zs = _replay(oracle, case, DC.REPLAYS)
    reports = DC.replay_reports(case, zs, corr=("nd", "nw"))
    _show(f"B {f}-K{K} no nwsum-1", reports)
    assert not any(r.ok for r in reports.values())


@pytest.mark.parametrize("f,K", [("quarter", 20), ("sparse", 300), ("big", 1500)], ids=lambda v: str(v))
def test_training_formula_on_frozen_is_visible(oracle, f, K):
    """The word with one training token: taking that token out (the training
    corrections, at its topic) moves its cell from 1 + b to b."""
    case, nw, z, draws = _frozen_run(oracle, f, K)
    w = DC.frozen_words(case, z)[1]
    zo = int(z[np.flatnonzero(case.words == w)[0]])
    p, groups = DC.frozen_reference(case, nw, nw.sum(0), w, corr=("nw", "nwsum"), zo=zo)
    r = DC.check_draws(draws[w], p, groups)
    print(f"C {f}-K{K} training formula: {r.figures()} -> {r.failures}")
    assert not r.ok
