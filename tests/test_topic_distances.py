"""CPU-side checks of the topic distances (no device needed):
lda_topic_distances / lda_topic_nearest and their ldatm_ mirrors are declared,
bound and exported; bad arguments fail with a status and a message of their own
before any device work; the Python faces check their arguments before any
native call and fail loudly without a GPU; and the numpy restatement that
checks the device (tests/topic_distance_numpy.py) is itself checked on a
hand-made table.  The GPU behaviour is in test_topic_distances_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import topic_distance_numpy as TD
from ldagibbssampling_amd import capi
from ldagibbssampling_amd import topic_model as tm

SAMPLER_CALLS = ["lda_topic_distances", "lda_topic_nearest", "lda_topic_distance_slabs"]
MODEL_CALLS = ["ldatm_topic_distances", "ldatm_nearest_topics"]
TM_HEADER = os.path.join(os.path.dirname(capi.HEADER_PATH), "lda_topic_model.h")
INVALID = -1


@pytest.fixture(scope="module")
def libs():
    if not (os.path.exists(capi.LIB_PATH) and os.path.exists(tm.TM_LIB_PATH)):
        from ldagibbssampling_amd.build import build_library
        build_library()
    return capi.load(), tm.load_tm()


def _handle(T, K=4):
    h = C.c_void_p()
    assert T.ldatm_create(C.byref(h), K, 1.0, 0.01) == 0
    return h


def _declared(path, prefix):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, text))


def _exported(path, prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r"\bT (%s\w+)" % prefix, out))


def test_symbols_in_header_binding_and_exports(libs):
    assert set(SAMPLER_CALLS) <= _declared(capi.HEADER_PATH, "lda_")
    assert set(SAMPLER_CALLS) <= set(capi.SIGNATURES)
    assert set(SAMPLER_CALLS) <= _exported(capi.LIB_PATH, "lda_")
    assert set(MODEL_CALLS) <= _declared(TM_HEADER, "ldatm_")
    assert set(MODEL_CALLS) <= set(tm.TM_SIGNATURES)
    assert set(MODEL_CALLS) <= _exported(tm.TM_LIB_PATH, "ldatm_")


def test_defines_match_the_header_and_the_abi_stays_8(libs):
    L, _ = libs
    text = open(capi.HEADER_PATH).read()
    assert "#define LDA_TOPIC_NEAREST_MAX %d\n" % capi.TOPIC_NEAREST_MAX in text
    assert capi.TOPIC_NEAREST_MAX == 64
    for define, name in (("COSINE", "cosine"), ("HELLINGER", "hellinger"), ("JS", "jensen_shannon"),
                         ("KL", "kullback_leibler")):
        assert "#define LDA_TOPIC_%s %d\n" % (define, capi.TOPIC_METRICS[name]) in text
    assert [capi.TOPIC_METRICS[n] for n in ("cosine", "hellinger", "jensen_shannon", "kullback_leibler")] == [0, 1, 2, 3]
    assert capi.TOPIC_METRICS == TD.METRICS
    assert L.lda_abi_version() == 8


def test_sampler_calls_reject_a_null_context(libs):
    L, _ = libs
    out = np.zeros(8, np.float64)
    ids = np.zeros(8, np.int32)
    assert L.lda_topic_distances(None, None, 0, out.ctypes.data) == INVALID
    assert b"null ctx" in L.lda_last_error()
    assert L.lda_topic_nearest(None, None, 0, 1, ids.ctypes.data, out.ctypes.data) == INVALID
    assert b"null ctx" in L.lda_last_error()


def test_the_slab_rule_is_a_function_of_the_shape_alone(libs):
    """lda_topic_distance_slabs (host only) against the rule the header
    states: at least 256 rows a slab, at most 64 slabs, the slabs' pair sums
    within 256 MiB (one plane if that is more)."""
    L, _ = libs
    s, r = C.c_int32(), C.c_int32()

    def rule(V, K, K2):
        n = max(1, min(-(-V // 256), (256 << 20) // (8 * K * K2), 64))
        rows = -(-V // n)
        return -(-V // rows), rows

    for V, K, K2 in [(1, 20, 20), (7, 64, 64), (300, 100, 100), (300, 2048, 2048), (3001, 512, 512), (3001, 20, 20),
                     (100000, 512, 512), (100000, 4096, 4096), (100000, 100, 512), (20000, 3000, 3000)]:
        assert L.lda_topic_distance_slabs(V, K, K2, C.byref(s), C.byref(r)) == 0
        assert (s.value, r.value) == rule(V, K, K2), (V, K, K2)
        assert (s.value - 1) * r.value < V <= s.value * r.value
        assert s.value * 8 * K * K2 <= max(256 << 20, 8 * K * K2)
    assert rule(3001, 512, 512) == (12, 251)            # eleven slabs of 251 rows and one of 240
    assert rule(100000, 4096, 4096) == (2, 50000)
    assert rule(20000, 3000, 3000)[0] == 3
    assert L.lda_topic_distance_slabs(0, 4, 4, C.byref(s), C.byref(r)) == INVALID and L.lda_last_error()


def test_model_calls_reject_bad_arguments_before_any_device_work(libs):
    """Models without documents and without a GPU: the argument checks come
    first, so each call names its own argument, not the missing device."""
    _, T = libs
    h, same, other = _handle(T), _handle(T), _handle(T)
    try:
        out = np.zeros(64 * 64, np.float64)
        ids = np.zeros(64 * 64, np.int32)
        po, pi = out.ctypes.data, ids.ctypes.data
        assert T.ldatm_topic_distances(None, None, 0, po) == INVALID and b"null" in T.ldatm_last_error()
        assert T.ldatm_nearest_topics(None, None, 0, 1, pi, po) == INVALID and b"null" in T.ldatm_last_error()
        for metric in (-1, 4, 99):
            assert T.ldatm_topic_distances(h, None, metric, po) == INVALID and b"metric" in T.ldatm_last_error()
            assert T.ldatm_nearest_topics(h, None, metric, 1, pi, po) == INVALID
            assert b"metric" in T.ldatm_last_error()
        for n in (0, -1, capi.TOPIC_NEAREST_MAX + 1):
            assert T.ldatm_nearest_topics(h, None, 2, n, pi, po) == INVALID
            assert b"LDA_TOPIC_NEAREST_MAX" in T.ldatm_last_error()
        assert T.ldatm_topic_distances(h, None, 2, None) == INVALID and b"null output" in T.ldatm_last_error()
        assert T.ldatm_nearest_topics(h, None, 2, 1, None, po) == INVALID and b"null output" in T.ldatm_last_error()
        assert T.ldatm_nearest_topics(h, None, 2, 1, pi, None) == INVALID and b"null output" in T.ldatm_last_error()
        # alphabets of 3 and 5 words: num_types differs
        for handle, V in ((h, 3), (same, 3), (other, 5)):
            words = (C.c_char_p * V)(*[b"w%d" % i for i in range(V)])
            assert T.ldatm_set_alphabet(handle, V, words) == 0
        assert T.ldatm_topic_distances(h, other, 2, po) == INVALID and b"num_types" in T.ldatm_last_error()
        assert T.ldatm_nearest_topics(h, other, 2, 1, pi, po) == INVALID and b"num_types" in T.ldatm_last_error()
        # the bad metric is named before the mismatch, and the mismatch before the device
        assert T.ldatm_topic_distances(h, other, 7, po) == INVALID and b"metric" in T.ldatm_last_error()
    finally:
        for x in (h, same, other):
            T.ldatm_destroy(x)


class _NoNative:
    """Stands where the loaded library would: any native call is a failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the argument check")


def test_python_faces_check_their_arguments_first(libs):
    from ldagibbssampling_amd.sampler import GibbsSampler
    for name in ("topic_distances", "nearest_topics"):
        assert callable(getattr(GibbsSampler, name))
    for name in ("topicDistances", "nearestTopics"):
        assert callable(getattr(tm.ParallelTopicModel, name))

    def sampler(V):
        g = GibbsSampler.__new__(GibbsSampler)      # no device: only the argument checks run
        g.K, g.V, g.D, g._h, g._L = 4, V, 3, None, _NoNative()
        return g

    g, g5 = sampler(3), sampler(5)
    for bad in ("euclid", "js", "", 4, -1, 2.0, True):
        with pytest.raises(ValueError, match="metric must be"):
            g.topic_distances(bad)
        with pytest.raises(ValueError, match="metric must be"):
            g.nearest_topics(3, bad)
    for bad in (0, -1, capi.TOPIC_NEAREST_MAX + 1):
        with pytest.raises(ValueError, match="n must be in"):
            g.nearest_topics(bad)
    for bad in ("a sampler", 3, np.zeros((4, 4))):
        with pytest.raises(ValueError, match="other must be a GibbsSampler"):
            g.topic_distances("cosine", bad)
        with pytest.raises(ValueError, match="other must be a GibbsSampler"):
            g.nearest_topics(2, "cosine", bad)
    with pytest.raises(ValueError, match="word types"):
        g.topic_distances("hellinger", g5)
    with pytest.raises(ValueError, match="word types"):
        g.nearest_topics(1, other=g5)

    def model(words):
        m = tm.ParallelTopicModel(4, 1.0, 0.01)
        il = tm.InstanceList(tm.Alphabet(words))
        il.add(tm.Instance([0, 1]))
        m.addInstances(il)
        return m

    m, same, swapped = model(["a", "b", "c"]), model(["a", "b", "c"]), model(["a", "c", "b"])
    real = m._L
    try:
        m._L = _NoNative()
        with pytest.raises(ValueError, match="metric must be"):
            m.topicDistances(metric="manhattan")
        with pytest.raises(ValueError, match="metric must be"):
            m.nearestTopics(2, metric=9)
        for bad in (0, capi.TOPIC_NEAREST_MAX + 1):
            with pytest.raises(ValueError, match="n must be in"):
                m.nearestTopics(bad)
        with pytest.raises(ValueError, match="other must be a ParallelTopicModel"):
            m.topicDistances(other=g)
        with pytest.raises(ValueError, match="other must be a ParallelTopicModel"):
            m.nearestTopics(2, other="model")
        # the same number of words in another order: the ids mean other words
        with pytest.raises(ValueError, match="alphabets differ"):
            m.topicDistances(other=swapped)
        with pytest.raises(ValueError, match="alphabets differ"):
            m.nearestTopics(2, other=swapped, metric="cosine")
        # an equal alphabet passes the checks and reaches the native call
        with pytest.raises(AssertionError, match="native call ldatm_topic_distances"):
            m.topicDistances(other=same)
    finally:
        m._L = real
        for x in (m, same, swapped):
            x.close()


def test_python_faces_fail_loudly_without_a_gpu(libs):
    """A valid call fails with LdaError when there is no GPU (no host
    fall-back); with one, it answers."""
    import torch
    m = tm.ParallelTopicModel(4, 1.0, 0.01)
    try:
        il = tm.InstanceList(tm.Alphabet(range(3)))
        il.add(tm.Instance([0, 1]))
        il.add(tm.Instance([2]))
        m.addInstances(il)
        calls = (lambda: m.topicDistances(), lambda: m.nearestTopics(2, metric="cosine"),
                 lambda: m.topicDistances(other=m, metric=3))
        if not torch.cuda.is_available():
            for call in calls:
                with pytest.raises(capi.LdaError):
                    call()
        else:
            assert m.topicDistances().shape == (4, 4) and m.nearestTopics(2)[0].shape == (4, 2)
    finally:
        m.close()


# ------------------------------------------------------- the restatement itself
def test_restatement_on_a_hand_made_table():
    """3 words, 3 topics.  Topics 0 and 1 hold the same column (2, 1, 1);
    topic 2 holds (0, 0, 4).  With beta = 0.5: phi_0 = phi_1 = (2.5, 1.5, 1.5) /
    5.5 and phi_2 = (0.5, 0.5, 4.5) / 5.5."""
    nw = np.array([[2, 2, 0], [1, 1, 0], [1, 1, 4]], np.int32)
    nwsum = nw.sum(axis=0).astype(np.int32)
    beta = 0.5
    p = np.array([2.5, 1.5, 1.5]) / 5.5
    q = np.array([0.5, 0.5, 4.5]) / 5.5
    np.testing.assert_allclose(TD.phi(nw, nwsum, beta), np.stack([p, p, q], axis=1), rtol=0, atol=1e-16)
    m = 0.5 * (p + q)
    want = {
        "cosine": float(p @ q / math.sqrt(p @ p) / math.sqrt(q @ q)),
        "hellinger": math.sqrt(1.0 - float(np.sqrt(p * q).sum())),
        "jensen_shannon": 0.5 * float((p * np.log(p / m)).sum()) + 0.5 * float((q * np.log(q / m)).sum()),
        "kullback_leibler": float((p * np.log(p / q)).sum()),
    }
    # worked by hand from the fractions: cos = (1.25 + 0.75 + 6.75) / sqrt(10.75 * 20.75)
    assert abs(want["cosine"] - 8.75 / math.sqrt(10.75 * 20.75)) < 1e-15
    for name, value in want.items():
        d = TD.topic_distances(nw, nwsum, beta, metric=name)
        assert d.shape == (3, 3)
        same = 1.0 if name == "cosine" else 0.0
        # identical columns: 0, 0, 0 and cosine 1 (Hellinger by its square: the
        # root of the direct form's 1 - sum turns a rounding of 1e-16 into 1e-8)
        z = TD.topic_distances(nw, nwsum, beta, metric=name, squared_hellinger=True)
        assert abs(z[0, 1] - same) < 1e-15 and abs(z[1, 0] - same) < 1e-15
        assert all(abs(z[k, k] - same) < 1e-15 for k in range(3))
        assert abs(d[0, 2] - value) < 1e-15 and abs(d[1, 2] - value) < 1e-15
        # rows restricts the result, names and integers are the same metric
        np.testing.assert_array_equal(TD.topic_distances(nw, nwsum, beta, metric=TD.METRICS[name], rows=[2, 0]),
                                      d[[2, 0]])
    kl = TD.topic_distances(nw, nwsum, beta, metric="kullback_leibler")
    kl_qp = float((q * np.log(q / p)).sum())
    # asymmetric: KL(p || q) = 0.7316, KL(q || p) = 0.6527
    assert abs(kl[2, 0] - kl_qp) < 1e-15 and abs(kl[0, 2] - 0.7316) < 1e-4 and abs(kl[2, 0] - 0.6527) < 1e-4
    for name in ("cosine", "hellinger", "jensen_shannon"):
        d = TD.topic_distances(nw, nwsum, beta, metric=name)
        np.testing.assert_allclose(d, d.T, rtol=0, atol=1e-15)
    h2 = TD.topic_distances(nw, nwsum, beta, metric="hellinger", squared_hellinger=True)
    np.testing.assert_allclose(h2, TD.topic_distances(nw, nwsum, beta, metric="hellinger") ** 2, rtol=0, atol=1e-15)
    # cross mode with another beta on side B: the column's phi changes, the row's does not
    x = TD.topic_distances(nw, nwsum, beta, nw, nwsum, 0.1, metric="kullback_leibler")
    q01 = np.array([0.1, 0.1, 4.1]) / 4.3
    assert abs(x[0, 2] - float((p * np.log(p / q01)).sum())) < 1e-15 and x[0, 0] > 1e-3


def test_restatement_limits_for_disjoint_support():
    """As beta -> 0 two topics on disjoint words are as far apart as two
    distributions get: Jensen-Shannon ln 2, Hellinger 1, cosine 0.  The
    Hellinger distance approaches 1 like sqrt(beta / N) (the overlap of a word
    with mass ~1 on one side and ~beta / N on the other), so within 1e-9 at
    beta = 1e-12 needs topics of N >= 1e6 tokens: the table holds 2e9 and
    1.5e9."""
    nw = np.array([[2_000_000_000, 0, 0], [0, 1_500_000_000, 0], [0, 0, 0]], np.int32)
    nwsum = nw.sum(axis=0).astype(np.int32)
    beta = 1e-12
    js = TD.topic_distances(nw, nwsum, beta, metric="jensen_shannon")
    he = TD.topic_distances(nw, nwsum, beta, metric="hellinger")
    co = TD.topic_distances(nw, nwsum, beta, metric="cosine")
    assert abs(js[0, 1] - math.log(2.0)) < 1e-9
    assert abs(he[0, 1] - 1.0) < 1e-9
    assert abs(co[0, 1]) < 1e-9
    # the empty topic 2 is uniform whatever beta is
    np.testing.assert_allclose(TD.phi(nw, nwsum, beta)[:, 2], 1.0 / 3.0, rtol=0, atol=1e-16)


def test_expected_nearest_orders_ties_and_tails():
    mat = np.array([[0.0, 0.5, 0.5, 0.25],
                    [0.5, 0.0, -0.0, 0.5],
                    [0.5, 0.0, 0.0, 0.5],
                    [0.25, 0.5, 0.5, 0.0]])
    t, v = TD.expected_nearest(mat, 4, "hellinger", True)
    assert t.tolist() == [[3, 1, 2, -1], [2, 0, 3, -1], [1, 0, 3, -1], [0, 1, 2, -1]]
    assert np.isnan(v[:, 3]).all() and v[0, :3].tolist() == [0.25, 0.5, 0.5]
    t, v = TD.expected_nearest(mat, 2, "cosine", True)
    assert t.tolist() == [[1, 2], [0, 3], [0, 3], [1, 2]]
    # cross mode: the row's own index is a candidate, and -0.0 ties with 0.0 by id
    t, _ = TD.expected_nearest(mat, 2, "jensen_shannon", False)
    assert t.tolist() == [[0, 3], [1, 2], [1, 2], [3, 0]]
