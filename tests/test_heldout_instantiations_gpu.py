"""The k_doc_completion instantiations that test_heldout_gpu.py's
configurations do not reach (C = Kp / 64 = 2, 4 and 16; it runs 1, 8, 32 and
64), under that module's own check against numpy -- its reference, its
documents (T - 1, T, T + 1 from capi.doc_completion_batch) and its derived
bars, unchanged."""
import numpy as np
import pytest

import test_heldout_gpu as T
from ldagibbssampling_amd import capi

pytestmark = pytest.mark.gpu
MORE = {
    # C = 2 (the other instantiation with 16-token batches), 4 and 16, each
    # with K short of Kp
    "k100_dense": dict(K=100, V=200, sampler="dense", alpha=lambda K: 0.05 + 0.4 * np.arange(K) / K),
    "k200_dense": dict(K=200, V=150, sampler="dense", alpha=lambda K: np.full(K, 0.2)),
    "k1000_dense": dict(K=1000, V=100, sampler="dense", alpha=lambda K: 0.02 + 0.3 * np.arange(K)[::-1] / K),
}
KP_OVER_64 = {"k100_dense": 2, "k200_dense": 4, "k1000_dense": 16}


@pytest.mark.parametrize("name", list(MORE))
def test_heldout_loglik_against_numpy(name, oracle, monkeypatch):
    assert not set(MORE) & set(T.CONFIGS)
    assert capi.padded_topics(MORE[name]["K"]) // 64 == KP_OVER_64[name]
    # the configuration is looked up by name when the shard is made
    monkeypatch.setitem(T.CONFIGS, name, MORE[name])
    T.test_heldout_loglik_against_numpy(name, oracle)
    assert T._shard(name)[0].Kp // 64 == KP_OVER_64[name]
