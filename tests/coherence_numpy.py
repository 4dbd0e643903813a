"""The brute-force restatement of reference-corpus coherence (no GPU, no
native code): it enumerates the units of a corpus, tests set membership, and
applies the three formulas of ldatm_coherence_finish in the stated order.

Units.  window == 0: every document with at least one token.  window == W >=
1: a document of L >= 1 tokens gives max(1, L - W + 1) units, the token ranges
[s, s + W) clipped to the document.  A token id of -1 is in no list."""
import math

import numpy as np

MEASURES = ("u_mass", "c_uci", "c_npmi")
DEFAULT_EPS = {"u_mass": 1.0, "c_uci": 1e-12, "c_npmi": 1e-12}


def units_of(doc_off, words, window):
    """The units as sets of word ids, in corpus order."""
    out = []
    for d in range(len(doc_off) - 1):
        doc = [int(w) for w in words[int(doc_off[d]) - int(doc_off[0]):int(doc_off[d + 1]) - int(doc_off[0])]]
        if not doc:
            continue
        if window == 0:
            out.append(set(doc))
        else:
            for s in range(max(1, len(doc) - window + 1)):
                out.append(set(doc[s:s + window]))
    return out


def presence(doc_off, words, window):
    """(where, units): for every word id >= 0 of the corpus the set of the
    units (numbered in corpus order) that hold it, and the number of units.
    It depends on the corpus and the window alone, so tests share it among
    word lists."""
    units = units_of(doc_off, words, window)
    where = {}
    for u, unit in enumerate(units):
        for w in unit:
            if w >= 0:
                where.setdefault(w, set()).add(u)
    return where, len(units)


def cooccurrences(word_ids, doc_off, words, window, pres=None):
    """(cooc[K, n (n + 1) / 2] int64, units): cell (i, j), j <= i, of topic k
    at i (i + 1) / 2 + j = units holding word_ids[k, i] and word_ids[k, j].
    pres: presence(doc_off, words, window), when the caller has it."""
    ids = np.asarray(word_ids)
    K, n = ids.shape
    where, units = presence(doc_off, words, window) if pres is None else pres
    both = {}       # units holding two words, counted once per pair of words
    cooc = np.zeros((K, n * (n + 1) // 2), np.int64)
    for k in range(K):
        for i in range(n):
            wi = int(ids[k, i])
            if wi < 0:
                continue
            for j in range(i + 1):
                wj = int(ids[k, j])
                if wj < 0:
                    continue
                key = (wi, wj) if wi <= wj else (wj, wi)
                if key not in both:
                    both[key] = len(where.get(wi, set()) & where.get(wj, set()))
                cooc[k, i * (i + 1) // 2 + j] = both[key]
    return cooc, units


def terms(measure, tri, n, units, epsilon=None):
    """The kept pairs' terms of one topic's triangle, i ascending then j
    ascending."""
    eps = DEFAULT_EPS[measure] if epsilon is None else epsilon
    N = float(units)
    out = []
    if units == 0:
        return out
    for i in range(1, n):
        Di = int(tri[i * (i + 1) // 2 + i])
        for j in range(i):
            Dj, Dij = int(tri[j * (j + 1) // 2 + j]), int(tri[i * (i + 1) // 2 + j])
            if Di == 0 or Dj == 0:
                continue
            if measure == "u_mass":
                out.append(math.log((Dij + eps) / Dj))
                continue
            if Dij == units:
                continue
            p = Dij / N + eps
            uci = math.log(p / ((Di / N) * (Dj / N)))
            out.append(uci if measure == "c_uci" else uci / -math.log(p))
    return out


def finish(measure, cooc, units, epsilon=None):
    """(sums[K], pairs[K], abs[K]): the sums added in order from 0.0, the
    number of kept pairs and the sum of the terms' magnitudes."""
    cooc = np.asarray(cooc)
    K, T = cooc.shape
    n = int(round((math.sqrt(8 * T + 1) - 1) / 2))
    sums, pairs, mags = np.zeros(K), np.zeros(K, np.int64), np.zeros(K)
    for k in range(K):
        t = terms(measure, cooc[k], n, units, epsilon)
        s = 0.0
        for x in t:
            s += x
        sums[k], pairs[k], mags[k] = s, len(t), sum(abs(x) for x in t)
    return sums, pairs, mags
