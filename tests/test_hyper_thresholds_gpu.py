"""The LDS / global thresholds of the hyperparameter statistics, exact against
test_hyper_gpu's numpy expressions.

k_doc_hist keeps document lengths below DOC_HIST_LEN = 1024 and per-topic
counts up to DOC_HIST_SMALL = 4 in LDS and sends the rest to device atomics;
its flush is guarded by i <= L and c <= L for corpora whose longest document
is shorter than either table.  k_count_hist bins counts below COUNT_HIST_LDS =
4096 in LDS and flushes bins i <= max_count.  The states are placed with
z_init and read after sweep(0), which applies the initial counts and samples
nothing, so every count below is exactly the one written here.
"""
import numpy as np
import pytest

import test_hyper_gpu as T
from ldagibbssampling_amd import capi
from ldagibbssampling_amd.corpus import Corpus

pytestmark = pytest.mark.gpu

DOC_HIST_LEN, DOC_HIST_SMALL, COUNT_HIST_LDS = 1024, 4, 4096
CONFIGS = [(20, "dense"), (2048, "sparse")]


def _sampler(K, kind, off, words, V, z0):
    from ldagibbssampling_amd.sampler import GibbsSampler
    g = GibbsSampler(K, V, off, words, 0.1, 0.01, seed=2, sampler=kind, z_init=z0)
    g.sweep(0)
    np.testing.assert_array_equal(g.z(), z0)
    return g


def _expected(z, off, K, max_len, times):
    lens = np.diff(off)
    nd = T._nd(z, off, K)
    dl = times * np.bincount(lens, minlength=max_len + 1)
    td = np.zeros((K, max_len + 1), np.int64)
    for k in range(K):
        v = nd[:, k]
        td[k] = times * np.bincount(v[v > 0], minlength=max_len + 1)
    return nd, dl, td


def _check_doc_hist(g, z, off, K):
    L = g.max_doc_length()
    assert L == np.diff(off).max()
    nd = None
    for max_len in (L, L + 7):                        # the row stride is max_len + 1
        dl, td = g.doc_topic_histograms(max_len=max_len)
        assert dl.shape == (max_len + 1,) and td.shape == (K, max_len + 1)
        nd, edl, etd = _expected(z, off, K, max_len, 1)
        np.testing.assert_array_equal(dl, edl)
        np.testing.assert_array_equal(td, etd)
        g.doc_topic_histograms(dl, td)                # accumulates
        np.testing.assert_array_equal(dl, 2 * edl)
        np.testing.assert_array_equal(td, 2 * etd)
    if L > 0:
        with pytest.raises(capi.LdaError):
            g.doc_topic_histograms(max_len=L - 1)
    return nd


@pytest.mark.parametrize("K,kind", CONFIGS)
def test_doc_hist_at_the_lds_edges(K, kind):
    rng = np.random.default_rng(K)
    V = 200
    lens = np.concatenate([[1023, 1024, 1025, 3000, 0, 1, 9, 9, 0, 1024, 1023],
                           rng.integers(0, 30, 84)]).astype(np.int64)
    rng.shuffle(lens)
    D = len(lens)
    assert D >= 2 * 40 and (D + 31) // 32 >= 3        # three blocks, eight documents to a wave
    off = np.zeros(D + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    z0 = rng.integers(0, K, int(off[-1])).astype(np.int32)
    # counts of exactly 4 and 5 (and 1015: far past the LDS table) in chosen documents
    for d in np.flatnonzero(lens == 9):
        z0[off[d]:off[d] + 4] = 3
        z0[off[d] + 4:off[d + 1]] = 4
    d = int(np.flatnonzero(lens == 1024)[0])
    z0[off[d]:off[d] + 4] = 0
    z0[off[d] + 4:off[d] + 9] = 1
    z0[off[d] + 9:off[d + 1]] = 2
    g = _sampler(K, kind, off, words, V, z0)
    nd = _check_doc_hist(g, z0, off, K)
    assert {DOC_HIST_LEN - 1, DOC_HIST_LEN, DOC_HIST_LEN + 1, 3000, 0} <= set(lens.tolist())
    assert {1, 2, 3, DOC_HIST_SMALL, DOC_HIST_SMALL + 1, 1015} <= set(np.unique(nd).tolist())
    g.close()


@pytest.mark.parametrize("K,kind", CONFIGS)
@pytest.mark.parametrize("L", [1, 3, 4])
def test_doc_hist_when_the_longest_document_is_shorter_than_the_tables(L, K, kind):
    rng = np.random.default_rng(10 * K + L)
    V = 50
    lens = rng.integers(0, L + 1, 70)
    lens[:2] = (L, 0)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    words = rng.integers(0, V, int(off[-1])).astype(np.int32)
    z0 = rng.integers(0, K, int(off[-1])).astype(np.int32)
    z0[off[0]:off[1]] = 5                              # a count of exactly L, the last column
    g = _sampler(K, kind, off, words, V, z0)
    nd = _check_doc_hist(g, z0, off, K)
    assert nd.max() == L == g.max_doc_length() and L <= DOC_HIST_SMALL
    g.close()


def _cells_corpus(cells, rest, seed):
    """Word 0 holds cells[k] tokens of topic k (exactly: z_init); `rest` more
    tokens of other words at random topics; 20 documents."""
    rng = np.random.default_rng(seed)
    V, K = 40, 20
    w0 = np.zeros(sum(cells), np.int32)
    z0 = np.repeat(np.arange(len(cells)), cells).astype(np.int32)
    words = np.concatenate([w0, rng.integers(1, V, rest).astype(np.int32)])
    z = np.concatenate([z0, rng.integers(0, K, rest).astype(np.int32)])
    order = rng.permutation(len(words))
    words, z = words[order], z[order]
    off = np.linspace(0, len(words), 21).astype(np.int64)
    return Corpus(off, words, V), z, K


def test_count_hist_cells_at_the_lds_size():
    c, z0, K = _cells_corpus([COUNT_HIST_LDS - 1, COUNT_HIST_LDS, COUNT_HIST_LDS + 1], 6000, 1)
    g = _sampler(K, "dense", c.doc_off, c.words, c.num_types, z0)
    nw = g.counts()[0]
    assert nw[0, :3].tolist() == [4095, 4096, 4097] and nw[1:].max() < COUNT_HIST_LDS - 1
    top = COUNT_HIST_LDS + 1
    h = g.count_histogram(top)
    np.testing.assert_array_equal(h, np.bincount(nw[nw > 0], minlength=top + 1))
    assert h[4095] == h[4096] == h[4097] == 1
    g.count_histogram(top, h)                          # accumulates
    np.testing.assert_array_equal(h, 2 * np.bincount(nw[nw > 0], minlength=top + 1))
    with pytest.raises(capi.LdaError):
        g.count_histogram(COUNT_HIST_LDS)              # the cell of 4097 exceeds it
    g.close()


@pytest.mark.parametrize("max_count", [COUNT_HIST_LDS - 1, COUNT_HIST_LDS])
def test_count_hist_flush_on_both_sides_of_the_lds_size(max_count):
    c, z0, K = _cells_corpus([COUNT_HIST_LDS - 1, 3000, 17], 6000, 2)
    g = _sampler(K, "dense", c.doc_off, c.words, c.num_types, z0)
    nw = g.counts()[0]
    assert nw.max() == COUNT_HIST_LDS - 1              # the largest cell sits in the LDS table's last bin
    h = g.count_histogram(max_count)
    assert h.shape == (max_count + 1,) and h[COUNT_HIST_LDS - 1] == 1
    np.testing.assert_array_equal(h, np.bincount(nw[nw > 0], minlength=max_count + 1))
    g.close()
