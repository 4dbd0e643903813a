"""The arguments of lifecycle_readout_probes select what they are meant to
select: checked without a device, on cpu_exact's chain after the first sweeps
of test_lifecycle_readouts_gpu.py's script (sweep(0) with the other shard's
counts, sweep(1): its second checkpoint) and with the numpy restatements alone.

One property cannot hold everywhere.  A phrase counted twice needs two equal
same-topic runs under one topic; with 512 or 2048 topics over about 6000 tokens
the chain holds none after these sweeps (136 and 40 distinct phrases, each seen
once), so a count of 2 is asserted at K = 20 and K = 300, and at K = 512 and
K = 2048 only that phrases are listed and that min_count = 2 lists none.
"""
import numpy as np
import pytest

import lifecycle_probes as P
import lifecycle_readout_probes as R
import doc_neighbors_numpy as DN
import group_topics_numpy as GN
import topic_docs_numpy as TDOC
import topic_phrases_numpy as TPN
from test_lifecycle_gpu import CASES, _foreign


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-K{c[1]}")
def state(request, oracle):
    """(K, alpha, z, nd) after sweep(0), sweep(1) of the long-lived context's mirror."""
    kind, K = request.param
    c = P.train_corpus()
    alpha = np.full(K, 0.1)
    o = oracle.ExactSampler(K, P.V, c.doc_off, c.words, alpha, P.BETA0, P.SEED, kind=kind)
    cells, vals = _foreign(K, o.Kp)
    np.add.at(o.delta(), cells, vals)
    o.sweep(0)
    o.sweep(1)
    z = o.z()
    return K, alpha, z, TDOC.doc_topic_counts(z, c.doc_off, K)


def test_orders_hold_every_probe_and_every_chain():
    for order in (R.ORDER_A, R.ORDER_B):
        assert set(order) == set(R.SIZED + R.UNSIZED)
    assert set(R.OLD) <= set(R.SIZED + R.UNSIZED) and not set(R.NEW_SIZED) & set(P.SIZED + P.UNSIZED)
    # the rotation of the GPU test (by 3 (cp // 2)) over the sparse cases' 12
    # checkpoints, the fewest: every chain is adjacent at some checkpoint
    seen = set()
    for cp in range(12):
        base = R.ORDER_A if cp % 2 == 0 else R.ORDER_B
        shift = (3 * (cp // 2)) % len(base)
        order = base[shift:] + base[:shift]
        seen |= set(zip(order, order[1:]))
    assert set(R.CHAINS) <= seen, sorted(set(R.CHAINS) - seen)


def test_document_thresholds_and_masks_split_the_corpus():
    lens = np.diff(P.train_corpus().doc_off)
    D = len(lens)
    thresholds = set(R.TOP_DOCS_MIN_TOKENS + R.NEAREST_MIN_TOKENS + R.NEIGHBOR_MIN_TOKENS)
    thresholds |= {t[0] for t in R.COOC_THRESHOLDS + R.GROUP_THRESHOLDS}
    assert {1, 60} <= thresholds
    for t in thresholds:
        assert (lens < t).any() and (lens >= t).any(), t
    # doc_neighbors at n = 64: fewer candidates than slots
    assert 2 <= (lens >= R.NEIGHBOR_MIN_TOKENS[1]).sum() < R.DOC_N[1]
    selected = sorted(int(np.count_nonzero(R.masks(i)[0])) for i in range(3))
    assert selected[0] == 0 and selected[2] == D and 0 < selected[1] < D
    assert [R.masks(i)[1] is not None for i in range(3)] == [True, False, True]       # alternate sizes accumulate
    assert 0 < np.count_nonzero(R.masks(0)[1]) < D and not np.any(R.masks(2)[0] & R.masks(2)[1])
    assert R.TOP_DOCS_N[1] > D                                                          # empty slots by size alone
    assert len(R.word_ids(1)) == P.V and P.unseen_word() in R.word_ids(2) and len(set(R.word_ids(2))) < 5
    assert len(R.LAMBDAS[1]) == 11 and R.LAMBDAS[0][0] in R.LAMBDAS[1] and set(R.LAMBDAS[2]) <= set(R.LAMBDAS[1])


def test_groups_leave_one_empty(state):
    K, _, z, _ = state
    off = P.train_corpus().doc_off
    shapes = []
    for i in range(3):
        groups, G = R.doc_groups(i)
        e = GN.expected_group_topics(z, off, K, groups, G, *R.GROUP_THRESHOLDS[i], R.GROUP_STATS[i])
        shapes.append(G)
        if i:
            assert (e["group_docs"] == 0).any() and (e["group_docs"] > 0).any(), i
            assert all(np.count_nonzero(groups == g) for g in range(G))      # empty by the threshold, not unassigned
        else:
            assert e["group_docs"][0] == np.count_nonzero(np.diff(off))
    assert shapes == [1, len(off) - 1, 3] and (R.doc_groups(2)[0] == -1).any()


def test_top_documents_have_empty_and_tied_slots(state):
    K, _, z, _ = state
    off = P.train_corpus().doc_off
    tied = []
    for i in range(3):
        docs, cnt, lens = TDOC.expected_topic_docs(z, off, K, R.TOP_DOCS_N[i], R.TOP_DOCS_SMOOTHING[i],
                                                   R.TOP_DOCS_MIN_TOKENS[i])
        assert (docs >= 0).any(), i
        tied.append(TDOC.has_tie(K, R.TOP_DOCS_SMOOTHING[i], docs, cnt, lens) if docs.shape[1] > 1 else False)
        if i == 1:
            assert (docs == -1).any()
    assert any(tied), tied


def test_phrases_qualify_at_the_chosen_counts(state):
    K, _, z, _ = state
    c = P.train_corpus()
    assert {a[1] for a in R.PHRASE_ARGS} >= {R.capi.PHRASE_LEN_MAX} and max(a[2] for a in R.PHRASE_ARGS) > 1
    for i in range(3):
        min_len, max_len, min_count = R.PHRASE_ARGS[i]
        res = TPN.expected_topic_phrases(c.words, z, c.doc_off, K, R.PHRASES_N[i], min_len, max_len, min_count)
        if K <= 300:
            assert (res[2] >= max(2, min_count)).any(), (i, int(res[2].max()))
        else:
            assert (res[2] >= 1).any() == (min_count == 1), i
        # the lookups: the listed phrases are found, the made-up ones mostly not
        topics, phrases = R.phrase_queries(K, res, max_len)
        table, _ = TPN.phrase_table(c.words, z, c.doc_off, min_len, max_len)
        counts, first = R.expected_phrase_counts(table, topics, phrases)
        listed = int(np.count_nonzero(res[1]))
        assert np.array_equal(counts[:listed], res[2][res[1] > 0])
        assert np.array_equal(first[:listed], res[3][res[1] > 0])
        assert len(counts) > listed and (counts[listed:] == 0).any() and (first[counts == 0] == -1).all(), i


def test_neighbour_lists_are_exhausted(state):
    K, alpha, _, nd = state
    lens = np.diff(P.train_corpus().doc_off)
    rows = DN.rows_from_counts(nd, alpha)
    ids = R.neighbor_docs(1, len(lens))[1]
    for metric in R.DOC_METRICS:
        d = DN.distances(rows[ids], rows, metric)
        near, vals = DN.nearest(d, R.DOC_N[1], metric, lengths=lens, min_tokens=R.NEIGHBOR_MIN_TOKENS[1], skip=ids)
        assert (near[:, 0] >= 0).all() and (near[:, -1] == -1).all() and np.isnan(vals[:, -1]).all()
    assert len(R.DOC_METRICS) == 3 and R.DOC_Q[1] > 64
