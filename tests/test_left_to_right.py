"""CPU-side checks of the left-to-right estimator (no device needed): the new
symbols are declared and bound, NULL handles and bad arguments fail with a
status and a message, the Python faces refuse wrong shapes before any native
call, the result object's perplexity, and the numpy restatement
(tests/ltr_numpy.py, the checker of test_left_to_right_gpu.py) against itself:
its enumerated expectations against its own sampler."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import ltr_numpy as N
from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")


@pytest.fixture(scope="module")
def libs():
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(tm.TM_LIB_PATH)):
        from ldagibbssampling_amd.build import build_library
        build_library()
    return capi.load(), tm.load_tm()


@pytest.fixture()
def handle(libs):
    _, T = libs
    h = C.c_void_p()
    assert T.ldatm_create(C.byref(h), 4, 1.0, 0.01) == 0
    yield h
    T.ldatm_destroy(h)


def test_new_symbols_in_headers_bindings_and_libraries(libs):
    L, T = libs
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"\blda_status\s+lda_left_to_right\s*\(", text)
    assert re.search(r"\bvoid\s+lda_debug_ltr_chunk_cells\s*\(", text)
    for name in ("lda_left_to_right", "lda_debug_ltr_chunk_cells"):
        assert name in capi.SIGNATURES and getattr(L, name) is not None
    text_tm = open(TM_HEADER).read()
    assert re.search(r"\blda_status\s+ldatm_left_to_right\s*\(", text_tm)
    assert "ldatm_left_to_right" in tm.TM_SIGNATURES and T.ldatm_left_to_right is not None
    # the limits are in the header, with the Python constants equal to them
    assert re.search(r"#define LDA_LTR_MAX_PARTICLES %d\b" % capi.LTR_MAX_PARTICLES, text)
    assert re.search(r"#define LDA_LTR_MAX_DOC_TOKENS %d\b" % capi.LTR_MAX_DOC_TOKENS, text)
    # only symbols were added: the ABI version stays, and the history names the addition
    assert "#define LDA_ABI_VERSION 8" in text and L.lda_abi_version() == 8
    assert re.search(r"lda_heldout_loglik and lda_doc_completion[^/]*lda_left_to_right[^/]*version stays 8", text)
    import ldagibbssampling_amd as pkg
    assert pkg.MarginalProbEstimator is tm.MarginalProbEstimator
    # stream 3 is the estimator's own
    kh = open(os.path.join(os.path.dirname(capi.LIB_PATH), "..", "csrc", "lda_kernels.h")).read()
    assert re.search(r"STREAM_LTR = %du;" % N.STREAM, kh)


def test_null_and_bad_arguments_without_a_device(libs, handle):
    L, T = libs
    off = np.array([0, 1], np.int64)
    w = np.array([0], np.int32)
    out = np.zeros(1)
    p = lambda a: a.ctypes.data
    assert L.lda_left_to_right(None, 1, p(off), p(w), 4, 1, 0, p(out), None, None, None, None) == -1
    assert b"null" in L.lda_last_error()
    assert T.ldatm_left_to_right(None, 1, p(off), p(w), 4, 1, 0, p(out), None, None) == -1
    assert b"null" in T.ldatm_last_error()
    assert T.ldatm_left_to_right(handle, 1, p(off), p(w), 4, 1, 0, None, None, None) == -1
    assert b"null doc_ll" in T.ldatm_last_error()
    # a model without instances has no state to evaluate against: a status, not a crash
    assert T.ldatm_left_to_right(handle, 1, p(off), p(w), 4, 1, 0, p(out), None, None) != 0
    assert T.ldatm_last_error()
    L.lda_debug_ltr_chunk_cells(0)


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the shape check")


def test_python_faces_reject_wrong_shapes(libs):
    off, words = np.array([0, 2, 3], np.int64), np.array([0, 1, 2], np.int32)
    from ldagibbssampling_amd.sampler import GibbsSampler
    g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
    g.K, g.D, g._h, g._L = 4, 3, None, _NoNative()
    with pytest.raises(ValueError, match="spans 3 tokens but words holds 1"):
        g.left_to_right(off, [0])
    with pytest.raises(ValueError, match="at least one offset"):
        g.left_to_right([], [])
    for bad in (0, -3):
        with pytest.raises(ValueError, match="particles must be at least 1"):
            g.left_to_right(off, words, particles=bad)
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    real = m._L
    try:
        m._L = _NoNative()
        est = m.getProbEstimator()
        assert isinstance(est, tm.MarginalProbEstimator)
        with pytest.raises(ValueError, match="numParticles must be at least 1"):
            est.leftToRight([tm.Instance([0, 1])], 0)
        with pytest.raises(ValueError, match="numParticles must be at least 1"):
            est.evaluateLeftToRight([tm.Instance([0, 1])], -1, True, io.StringIO())
    finally:
        m._L = real
        m.close()


def test_result_perplexity():
    r = tm.LeftToRightResult(-690.5, 100, np.array([-300.0, -390.5]))
    assert r.perplexity == float(np.exp(690.5 / 100))
    assert (r.logLikelihood, r.tokens) == (-690.5, 100) and r.perDocument.shape == (2,)
    assert np.isnan(tm.LeftToRightResult(0.0, 0, np.zeros(0)).perplexity)
    assert "perplexity" in repr(r)


# ------------------------------------------------ the restatement, by itself
NW = np.array([[30, 1, 0], [0, 25, 2], [1, 0, 40], [12, 10, 9], [0, 0, 0]], np.int32)   # type 4: an empty row
ALPHA = np.array([0.3, 0.2, 0.4])
BETA = 0.01
DOC = [3, 0, 4, 0, 3]


def test_restatement_draw_and_skip():
    assert N.skipped(NW, DOC).tolist() == [False, False, True, False, False]
    x = np.array([0.0, 2.0, 0.0, 1.0, 0.0])
    assert [N.draw(x, u) for u in (0.0, 0.5, 0.66, 0.67, 0.999)] == [1, 1, 1, 3, 3]
    assert N.draw(x, 1.0) == 3                       # no prefix exceeds t: the last positive weight
    phi = N.phi_table(NW, NW.sum(0), BETA)
    np.testing.assert_allclose(phi.sum(0), 1.0, rtol=1e-14)
    p = np.array([[0.5, 0.0, 0.25], [0.25, 0.0, 0.25]])
    phat, ll = N.estimate(p)
    assert phat.tolist() == [0.375, 0.0, 0.25] and ll == float(np.log(0.375) + np.log(0.25))


@pytest.mark.parametrize("resampling", [False, True])
def test_restatement_expectation_against_its_own_sampler(resampling):
    """n single-particle runs of the restated sampler against the enumerated
    chain: the mean of p[i] within 6 (hi - lo) / 2 / sqrt(n) of E[p[i]] (a
    bound on the standard error from the range), and without resampling the
    mean weight within 6 of its standard errors of the marginal."""
    phi = N.phi_table(NW, NW.sum(0), BETA)
    skip = N.skipped(NW, DOC)
    ex, marginal = N.exact(phi, ALPHA, DOC, skip, resampling)
    n = 3000
    rng = np.random.default_rng(11 + resampling)
    ps = np.array([N.run_particle(phi, ALPHA, DOC, skip, resampling, lambda j, i: rng.random())[0]
                   for _ in range(n)])
    assert ex[2] is None and np.all(ps[:, 2] == 0.0)
    for i in (0, 1, 3, 4):
        mean, lo, hi = ex[i]
        assert lo <= mean <= hi
        assert abs(ps[:, i].mean() - mean) <= 6 * (hi - lo) / 2 / np.sqrt(n) + 1e-12, i
    assert ex[0][1] == ex[0][2]                      # position 0 is deterministic
    if not resampling:
        w = ps[:, ~skip].prod(axis=1)
        assert abs(w.mean() - marginal) <= 6 * w.std(ddof=1) / np.sqrt(n)


def test_restatement_modes_differ():
    """The two modes have different expectations at position 3 of this
    document (by far more than the GPU test's bar at M R = 32000), and the same
    ones where no token has been resampled yet."""
    phi = N.phi_table(NW, NW.sum(0), BETA)
    skip = N.skipped(NW, DOC)
    a, ma = N.exact(phi, ALPHA, DOC, skip, False)
    b, mb = N.exact(phi, ALPHA, DOC, skip, True)
    assert ma == mb
    for i in (0, 1):
        assert abs(a[i][0] - b[i][0]) <= 1e-14
    bar = 6 * (a[3][2] - a[3][1]) / 2 / np.sqrt(32000)
    assert abs(a[3][0] - b[3][0]) > 3 * bar


def test_no_instantiation_uses_scratch(libs):
    """One k_left_to_right per C = 1 .. 64 in the built library's gfx950 code
    object, none with scratch memory; nd lives in LDS from C = 32 on (a wave's
    64 C int32, four waves a block) and nowhere below."""
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import left_to_right_isa
    finally:
        sys.path.remove(tools)
    rows = left_to_right_isa.rows(capi.LIB_PATH)
    assert [c for k, c, _, _ in rows if k == "k_left_to_right"] == [1, 2, 4, 8, 16, 32, 64]
    assert [k for k, _, _, _ in rows].count("k_ltr_reduce") == 1
    for kernel, c, _, d in rows:
        assert d["scratch_bytes"] == 0 and not d["scratch_enabled"], (kernel, c)
        assert d["lds_bytes"] == (4 * 64 * c * 4 if c is not None and c >= 32 else 0), (kernel, c)
        assert d["vgprs_total"] <= 512
