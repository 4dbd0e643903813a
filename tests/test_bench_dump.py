"""bench.py --dump-outputs: what it writes, from a stand-in sampler (no GPU).

The dump must hold the same cells for the same shapes whatever build wrote
it (seeded draws of rows / token positions), stay float32 / float64 and
under 64 MB, and keep whole arrays whole when they fit."""
import importlib.util
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def bench():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _State:
    """The three members dump_outputs reads of a GibbsSampler."""

    def __init__(self, V, K, N, seed):
        rng = np.random.default_rng(seed)
        self.V, self.K, self.N = V, K, N
        self._z = rng.integers(0, K, size=N, dtype=np.int32)
        self._nw = rng.integers(0, 1 << 20, size=(V, K), dtype=np.int32)

    def counts(self):
        return self._nw, self._nw.sum(axis=0, dtype=np.int64).astype(np.int32), None, None

    def z(self):
        return self._z


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_state_is_dumped_whole(bench, tmp_path):
    s = _State(V=37, K=5, N=1001, seed=3)
    bench.dump_outputs(str(tmp_path), s)
    out = _load(tmp_path)
    assert sorted(out) == ["nw", "nw_rows", "nwsum", "z"]
    assert out["nw"].dtype == np.float64 and out["nwsum"].dtype == np.float64
    assert out["z"].dtype == np.float32
    assert np.array_equal(out["nw"], s._nw) and np.array_equal(out["nw_rows"], np.arange(37))
    assert np.array_equal(out["nwsum"], s._nw.sum(axis=0)) and np.array_equal(out["z"], s._z)


def test_large_state_is_sampled_the_same_way_every_time(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_NW_BYTES", 8 * 16 * 11)      # 11 rows of K = 16
    monkeypatch.setattr(bench, "DUMP_Z_TOKENS", 257)
    s = _State(V=300, K=16, N=5003, seed=4)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), s)
    bench.dump_outputs(str(b), s)
    xa, xb = _load(a), _load(b)
    for k in xa:
        assert np.array_equal(xa[k], xb[k]), k
    rows = xa["nw_rows"].astype(np.int64)
    assert rows.shape == (11,) and len(set(rows.tolist())) == 11 and np.all(np.diff(rows) > 0)
    assert np.array_equal(xa["nw"], s._nw[rows])
    assert xa["z"].shape == (257,)
    # another state of the same shapes is sampled at the same cells
    t = _State(V=300, K=16, N=5003, seed=5)
    c = tmp_path / "c"
    bench.dump_outputs(str(c), t)
    xc = _load(c)
    assert np.array_equal(xc["nw_rows"], xa["nw_rows"]) and np.array_equal(xc["nw"], t._nw[rows])


def test_dump_budget_at_the_largest_config(bench):
    """The kept cells of every configuration stay under 64 MB."""
    for cfg in bench.CONFIGS.values():
        rows = min(cfg["V"], max(1, bench.DUMP_NW_BYTES // (8 * cfg["K"])))
        total = 8 * rows * cfg["K"] + 8 * rows + 8 * cfg["K"] + 4 * bench.DUMP_Z_TOKENS
        assert total <= 64 * 10**6, (cfg["desc"], total)
