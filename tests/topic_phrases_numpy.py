"""The topic phrases restated by brute force, straight from the definition
(DESIGN.md 9j), without a device: a Python loop over documents and tokens and
a dictionary keyed by (topic, tuple(words)).

A run is a maximal range of consecutive tokens [s, e) of one document with one
topic; its phrase is (topic, words[s:e]).  It qualifies with min_len <= e - s
<= max_len; a longer run counts toward skipped_long alone, a shorter one toward
nothing.  Per topic the phrases are ordered by count descending, then by the
word id sequence ascending, a proper prefix before its extension (Python's
tuple order)."""
import numpy as np


def runs(z, doc_off):
    """Every run as (topic, start, end), in token order."""
    out = []
    for d in range(len(doc_off) - 1):
        s, e = int(doc_off[d]), int(doc_off[d + 1])
        while s < e:
            t = s + 1
            while t < e and z[t] == z[s]:
                t += 1
            out.append((int(z[s]), s, t))
            s = t
    return out


def phrase_table(words, z, doc_off, min_len=2, max_len=32):
    """({(topic, words tuple): [count, smallest start]}, skipped_long)."""
    table, skipped = {}, 0
    for k, s, e in runs(z, doc_off):
        if e - s > max_len:
            skipped += 1
        elif e - s >= min_len:
            key = (k, tuple(int(w) for w in words[s:e]))
            if key in table:
                table[key][0] += 1
            else:
                table[key] = [1, s]
    return table, skipped


def ranked(table, K, min_count=1):
    """Per topic [(words tuple, count, first), ...] in the total order."""
    per = [[] for _ in range(K)]
    for (k, ph), (c, f) in table.items():
        if c >= min_count:
            per[k].append((ph, c, f))
    for lst in per:
        lst.sort(key=lambda e: (-e[1], e[0]))
    return per


def expected_topic_phrases(words, z, doc_off, K, n, min_len=2, max_len=32, min_count=1):
    """What lda_topic_phrases returns: (words[K, n, max_len] int32, lengths[K, n]
    int32, counts[K, n] int64, first[K, n] int64, runs[K] int64, distinct[K]
    int64, skipped_long)."""
    table, skipped = phrase_table(words, z, doc_off, min_len, max_len)
    w = np.full((K, n, max_len), -1, np.int32)
    lens = np.zeros((K, n), np.int32)
    cnt = np.zeros((K, n), np.int64)
    first = np.full((K, n), -1, np.int64)
    nruns = np.zeros(K, np.int64)
    distinct = np.zeros(K, np.int64)
    for (k, _), (c, _) in table.items():
        nruns[k] += c
        distinct[k] += 1
    for k, lst in enumerate(ranked(table, K, min_count)):
        for i, (ph, c, f) in enumerate(lst[:n]):
            w[k, i, :len(ph)] = ph
            lens[k, i], cnt[k, i], first[k, i] = len(ph), c, f
    return w, lens, cnt, first, nruns, distinct, skipped


def content_tie(lens, cnt):
    """True if two neighbours of one topic's list share a count: their order
    was decided by content."""
    return bool(np.any((cnt[:, 1:] == cnt[:, :-1]) & (lens[:, 1:] > 0)))


def bound_and_proven(shard_counts, totals):
    """The multi-shard bound: B_k = sum over shards of the shard's last listed
    count (0 where the list is not full); proven[k] = the leading totals
    strictly above B_k, n where B_k = 0."""
    sc = np.asarray(shard_counts, np.int64)
    tot = np.asarray(totals, np.int64)
    B = sc[:, :, -1].sum(axis=0)
    n = tot.shape[1]
    proven = np.zeros(len(B), np.int32)
    for k in range(len(B)):
        lead = 0
        while lead < n and tot[k, lead] > B[k]:
            lead += 1
        proven[k] = n if B[k] == 0 else lead
    return B, proven
