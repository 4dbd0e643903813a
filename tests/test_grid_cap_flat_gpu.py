"""The flat and per-row kernels past their launchers' block caps (DESIGN.md
§6, "Capped launchers"): one wide and long corpus, bit for bit against
cpu_exact.

V = 140,003, K = 20 (Kp = 64) and about 4.3M tokens in 33,000 documents of 0
to 260 tokens: V Kp = 8,960,192 cells.  A launcher that caps its grid at B
blocks covers P = 256 B tokens or int4 cells (4 B rows for the wave-per-row
kernels) in one pass; every cap below is asserted to be exceeded at least
twice over (n >= 2 P + 37) before the kernels run:

  k_init_z 2,097,152 tokens, k_count 1,048,576, k_word_hist / k_word_scatter
  2,097,152, k_zw_build 4,194,304 (its second trip; the corpus is not a
  third), k_recount 32 x CUs items, k_apply_packed / k_build_sparse 65,536
  rows, k_row_caps 32,768 rows, k_apply_build / k_row_stats 8,192 rows,
  k_fold_delta / k_exch_pack[4] / k_exch_unpack[4] 8,388,608 cells (their
  second trip), k_counts_checksum 2,097,152 cells, k_philox_draws 1,048,576.

Three runs launch them: "recount" (dense: k_init_z, k_count, k_word_hist,
k_word_scatter, k_zw_build, k_recount, k_apply_packed), "delta" (dense:
k_init_z, k_count, k_apply_packed on a delta) and "sparse" (k_init_z,
k_count, k_apply_cols, k_row_caps, k_build_sparse, then k_apply_build).
The oracle runs once per sampler kind and its snapshots are shared.
"""
import numpy as np
import pytest

from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu

V, K, KP, D = 140003, 20, 64, 33000
BETA, SEED = 0.01, 2025
HOT = 7
RUNS = {"recount": "dense", "delta": "dense", "sparse": "sparse"}
_corpus = None
_oracles = {}
_ctx = {}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def corpus():
    global _corpus
    if _corpus is None:
        rng = np.random.default_rng(12)
        lens = rng.integers(0, 261, D)
        lens[::97] = 0
        off = np.zeros(D + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        words = rng.integers(0, V, int(off[-1])).astype(np.int32)
        words[words % 1000 == 999] -= 1                  # every thousandth word type has no token: an empty row
        words[rng.random(len(words)) < 0.03] = HOT       # a word of ~130 recount items, rows of large counts
        _corpus = Corpus(off, words, V)
    return _corpus


def alpha():
    return 0.05 + 0.4 * np.arange(K) / K


def check_caps():
    """Every cap named in the module's docstring is exceeded by this shape."""
    c = corpus()
    N, cells = c.num_tokens, V * KP
    assert KP == 64 and cells == 8960192
    assert N >= 2 * 2097152 + 37            # k_init_z, k_word_hist, k_word_scatter; k_count twice over
    assert N > 4194304                      # k_zw_build: a second trip
    assert cells > 8388608                  # k_fold_delta, k_exch_*: a second trip
    assert cells >= 2 * 2097152 + 37        # k_counts_checksum
    assert V >= 2 * 65536 + 37              # k_apply_packed, k_build_sparse, and every smaller row cap
    assert len(np.unique(c.words)) >= 2 * 32 * _cus() + 37      # k_recount: a used word is at least one item
    return c


def oracle_at(oracle, kind, sweeps):
    """(z, nw, nwsum) of cpu_exact after sweep(0) and `sweeps` sweeps."""
    c = corpus()
    if kind not in _oracles:
        o = oracle.ExactSampler(K, V, c.doc_off, c.words, alpha(), BETA, SEED, kind=kind)
        o.apply()
        _oracles[kind] = (o, {})
    o, snaps = _oracles[kind]
    while sweeps not in snaps:
        if o.sweep_index not in snaps:
            nw, nwsum, _, _ = o.counts()
            snaps[o.sweep_index] = (o.z(), nw, nwsum)
        if o.sweep_index < sweeps:
            o.sweep(1)
    return snaps[sweeps]


def same(g, snap):
    z, nw, nwsum = snap
    np.testing.assert_array_equal(g.z(), z)
    gnw, gns, _, _ = g.counts()
    np.testing.assert_array_equal(gnw, nw)
    np.testing.assert_array_equal(gns, nwsum)


def context(oracle, run):
    """The run's context after sweep(0) and 2 sweeps, each state held against
    the oracle on the way (made once per run and kept for the later tests)."""
    if run not in _ctx:
        from ldagibbssampling_amd.sampler import GibbsSampler
        c = check_caps()
        g = GibbsSampler(K, V, c.doc_off, c.words, alpha(), BETA, seed=SEED, sampler=RUNS[run])
        assert g.Kp == KP
        if RUNS[run] == "dense":
            g.set_count_update(run)
            assert g.count_update()[0] == run
        g.sweep(0)
        same(g, oracle_at(oracle, RUNS[run], 0))
        g.sweep(2)
        same(g, oracle_at(oracle, RUNS[run], 2))
        if run == "recount":
            assert np.all(g.recount_times(2) > 0)
        if run == "delta":
            assert np.all(g.recount_times(2) == 0)
        _ctx[run] = g
    return _ctx[run]


@pytest.mark.parametrize("run", list(RUNS))
def test_sweeps_bit_exact_past_the_caps(oracle, run):
    g = context(oracle, run)
    assert g.sweep_index >= 2


@pytest.mark.parametrize("run", list(RUNS))
def test_readouts_past_the_caps(oracle, run):
    """k_row_stats, k_counts_checksum, and k_row_caps through lda_infer's
    empty-row test, on the state the parity test left."""
    g = context(oracle, run)
    c = corpus()
    z, nw, nwsum = oracle_at(oracle, RUNS[run], g.sweep_index)
    nwf = nw.astype(np.float64)
    tot, nnz = nwf.sum(1), (nwf > 0).sum(1)
    assert abs(g.row_stats() - (tot * nnz).sum() / tot.sum()) < 1e-9
    assert g.counts_checksum() == oracle.counts_checksum(nw, nwsum)
    # held-out documents of words from every pass of k_row_caps (32,768 rows),
    # words without training tokens among them: those tokens are dropped
    rng = np.random.default_rng(3)
    empty_rows = np.flatnonzero(tot == 0)
    assert len(empty_rows) >= 140 and empty_rows.max() > 2 * 32768
    held = np.concatenate([rng.integers(0, V, 400), empty_rows[-40:], rng.integers(2 * 32768, V, 200)]).astype(np.int32)
    rng.shuffle(held)
    off = np.arange(0, len(held) + 1, 20, dtype=np.int64)
    o = oracle.ExactSampler(K, V, c.doc_off, c.words, alpha(), BETA, SEED, z_init=z, kind=RUNS[run])
    o.apply()
    args = dict(n_iter=6, burn_in=2, thin=2, seed=4)
    np.testing.assert_allclose(g.infer(off, held, **args), o.infer(off, held, **args), rtol=0, atol=1e-12)


@pytest.mark.parametrize("run", list(RUNS))
def test_split_sweep_and_fold_past_the_caps(oracle, run):
    """Two exchange parts for one sweep (k_fold_delta in the apply), then back
    to one part and another sweep."""
    g = context(oracle, run)
    n = g.sweep_index
    g.set_exchange_parts(2)
    g.sample()
    g.apply()
    same(g, oracle_at(oracle, RUNS[run], n + 1))
    g.set_exchange_parts(1)
    g.sweep(1)
    same(g, oracle_at(oracle, RUNS[run], n + 2))


@pytest.mark.parametrize("cells", [2, 4])
def test_compact_exchange_past_the_caps(oracle, cells):
    """test_exchange_gpu.test_compact_exchange_bit_exact on two shards of this
    corpus: the packed words and escapes against oracle.exchange_pack, the
    unpacked sum against the int32 sum."""
    import torch
    from ldagibbssampling_amd.distributed import shard_corpus
    from ldagibbssampling_amd.sampler import GibbsSampler
    c = check_caps()
    world = 2
    shards = [shard_corpus(c.doc_off, c.words, world, r) for r in range(world)]
    gs = [GibbsSampler(K, V, sh.doc_off, sh.words, alpha(), BETA, seed=SEED, token_base=sh.token_base)
          for sh in shards]
    try:
        for g in gs:
            g.set_exchange_cells(cells)
        N = max(g.N for g in gs)
        before = [g.delta_tensor().clone() for g in gs]
        want = torch.stack([b.to(torch.int64) for b in before]).sum(0).to(torch.int32)
        packs = [g.exchange_pack(0, world, N) for g in gs]
        torch.cuda.synchronize()
        if cells == 4:
            assert min(int(e[0]) for _, e in packs) >= 1      # the hot word's cells pass 2^7 / world
        for (pk, es), b in zip(packs, before):
            opk, oes = oracle.exchange_pack(b.cpu().numpy(), world, KP, N, cells=cells)
            np.testing.assert_array_equal(pk.cpu().numpy(), opk)
            n = int(oes[0])
            assert int(es[0]) == n
            got = es[1:1 + 3 * n].cpu().numpy().reshape(-1, 3)
            ref = oes[1:1 + 3 * n].reshape(-1, 3)
            np.testing.assert_array_equal(got[np.lexsort(got.T[::-1])], ref[np.lexsort(ref.T[::-1])])
        total = torch.stack([pk.to(torch.int64) for pk, _ in packs]).sum(0)
        assert int(total.max()) < 2 ** 31 and pk.numel() == V * KP // cells + KP
        esc_all = torch.cat([es for _, es in packs])
        for g, (pk, _) in zip(gs, packs):
            pk.copy_(total.to(torch.int32))
            g.exchange_unpack(0, world, N, esc_all)
        torch.cuda.synchronize()
        for g in gs:
            assert torch.equal(g.delta_tensor(), want)
    finally:
        for g in gs:
            g.close()


def test_philox_draws_past_the_cap(oracle):
    from ldagibbssampling_amd import capi
    L = capi.load()
    P = 4096 * 256
    n = 2 * P + 37
    rng = np.random.default_rng(8)
    gtok = rng.integers(0, 1 << 40, n).astype(np.int64)
    out = np.zeros(n, np.uint32)
    seed, c2, c3 = 2**63 + 5, 13, 1
    assert L.lda_philox_draws(seed, c2, c3, gtok.ctypes.data, n, out.ctypes.data) == 0
    at = np.concatenate([[0, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, n - 1], rng.integers(0, n, 2000)])
    ref = np.array([oracle.draw(seed, int(gtok[i]), c2, c3) for i in at], np.uint32)
    np.testing.assert_array_equal(out[at], ref)
