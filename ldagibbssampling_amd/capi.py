"""ctypes binding of the C ABI in include/lda_mi355x.h (liblda_mi355x.so).

The library is built in-tree (ldagibbssampling_amd/lib/) by build.py /
__graft_entry__.build().  There is no CPU fallback: if the library is missing
or cannot be loaded, importing the sampler raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblda_mi355x.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lda_mi355x.h")

LDA_OK = 0
STATUS_NAMES = {
    -1: "LDA_ERR_INVALID_ARG",
    -2: "LDA_ERR_DEVICE",
    -3: "LDA_ERR_OUT_OF_MEMORY",
    -4: "LDA_ERR_STATE",
    -5: "LDA_ERR_UNSUPPORTED",
    -6: "LDA_ERR_INTERNAL",
}
MAX_TOPICS = 4096
MAX_TOPICS_DENSE = 1024
MAX_DOC_TOKENS_BIGK = 65535
MAX_EXCHANGE_PARTS = 4
SAMPLERS = {"dense": 0, "sparse": 1}
COUNT_UPDATE = {"auto": 0, "recount": 1, "delta": 2}
SCORE_METRICS = {"cosine": 0, "mse": 1}
# LDA_TOP_WORDS_MAX / LDA_TOP_TOPICS_MAX of lda_mi355x.h
TOP_WORDS_MAX = 64
TOP_TOPICS_MAX = 64
# LDA_TOPIC_DOCS_MAX of lda_mi355x.h
TOPIC_DOCS_MAX = 128
# LDA_TOPIC_COOC_LDS_TOPICS of lda_mi355x.h: lda_topic_cooccurrence accumulates in
# LDS up to this K, with global atomics above
TOPIC_COOC_LDS_TOPICS = 64
# lda_topic_cooccurrence's optional K x K tables, in the order of its arguments
TOPIC_COOC_STATS = ("codocs", "overlap", "product")


def topic_cooc_stats(stats) -> tuple:
    """The requested tables of lda_topic_cooccurrence as a tuple of names, in
    the call's order; a single name is accepted."""
    if isinstance(stats, str):
        stats = (stats,)
    stats = tuple(stats)
    for s in stats:
        if s not in TOPIC_COOC_STATS:
            raise ValueError(f"unknown statistic {s!r}: one of {TOPIC_COOC_STATS}")
    return tuple(s for s in TOPIC_COOC_STATS if s in stats)


def topic_cooc_thresholds(min_tokens, min_count, min_prop) -> tuple:
    """lda_topic_cooccurrence's thresholds, checked as the library checks them."""
    min_tokens, min_count, min_prop = int(min_tokens), int(min_count), float(min_prop)
    if min_tokens < 1:
        raise ValueError("min_tokens must be at least 1")
    if min_count < 1:
        raise ValueError("min_count must be at least 1")
    if not 0.0 <= min_prop <= 1.0:
        raise ValueError("min_prop must be in [0, 1]")
    return min_tokens, min_count, min_prop
# LDA_GROUP_TOPICS_MAX_CELLS of lda_mi355x.h: lda_group_topics takes G * K up to this
GROUP_TOPICS_MAX_CELLS = 1 << 28
# lda_group_topics' optional G x K tables, in the order of its arguments
GROUP_TOPICS_STATS = ("present", "shares")


def group_topics_stats(stats) -> tuple:
    """The requested optional tables of lda_group_topics as a tuple of names,
    in the call's order; a single name is accepted."""
    if isinstance(stats, str):
        stats = (stats,)
    stats = tuple(stats)
    for s in stats:
        if s not in GROUP_TOPICS_STATS:
            raise ValueError(f"unknown statistic {s!r}: one of {GROUP_TOPICS_STATS}")
    return tuple(s for s in GROUP_TOPICS_STATS if s in stats)


def group_ids(doc_group, D: int, G=None) -> tuple:
    """(ids int32 [D], G) of lda_group_topics' doc_group, checked as the library
    checks it: one id in [-1, G) per document; G = None takes the largest id
    plus one (at least 1)."""
    ids = np.ascontiguousarray(doc_group, dtype=np.int64)
    if ids.shape != (int(D),):
        raise ValueError(f"doc_group must hold one group id per document ({int(D)})")
    G = max(1, int(ids.max()) + 1 if ids.size else 1) if G is None else int(G)
    if G < 1:
        raise ValueError("G must be at least 1")
    bad = np.nonzero((ids < -1) | (ids >= G))[0]
    if bad.size:
        raise ValueError(f"doc_group[{int(bad[0])}] = {int(ids[bad[0]])} is outside [-1, G)")
    return ids.astype(np.int32), G


def doc_mask(mask, D: int) -> np.ndarray:
    """lda_subcorpus_count's doc_mask: uint8 [D], nonzero = the document counts."""
    m = np.asarray(mask)
    if m.shape != (int(D),):
        raise ValueError(f"mask must hold one entry per document ({int(D)})")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


# LDA_RELEVANCE_LAMBDAS_MAX / LDA_SALIENT_WORDS_MAX of lda_mi355x.h
RELEVANCE_LAMBDAS_MAX = 128
SALIENT_WORDS_MAX = 256
# LDA_PHRASE_LEN_MAX / LDA_PHRASES_MAX of lda_mi355x.h
PHRASE_LEN_MAX = 32
PHRASES_MAX = 128
# LDA_DIAG_WORDS_MAX / LDA_DIAG_PROPS_MAX of lda_mi355x.h
DIAG_WORDS_MAX = 64
DIAG_PROPS_MAX = 8
# LDA_COOC_WINDOW_MAX of lda_mi355x.h
COOC_WINDOW_MAX = 256
# LDA_LTR_MAX_PARTICLES / LDA_LTR_MAX_DOC_TOKENS of lda_mi355x.h
LTR_MAX_PARTICLES = 1024
LTR_MAX_DOC_TOKENS = 4096
# LDA_TOPIC_* metrics and LDA_TOPIC_NEAREST_MAX of lda_mi355x.h
TOPIC_METRICS = {"cosine": 0, "hellinger": 1, "jensen_shannon": 2, "kullback_leibler": 3}
TOPIC_NEAREST_MAX = 64
# the metrics of lda_doc_distances / lda_doc_nearest / lda_doc_neighbors (the
# LDA_TOPIC_* numbers 0..2) and LDA_DOC_NEAREST_MAX of lda_mi355x.h
DOC_METRICS = {"cosine": 0, "hellinger": 1, "jensen_shannon": 2}
DOC_NEAREST_MAX = 64


def relevance_batch(n: int) -> int:
    """The lambdas one pass of lda_relevant_words handles at list length n
    (lda_mi355x.h): the largest of 8, 4, 2, 1 whose lists, 12 bytes x 64
    topics x n each, fit 64 KiB of LDS.  Passes start at multiples of it."""
    b = 8
    while b > 1 and b * n * 64 * 12 > 64 * 1024:
        b >>= 1
    return b


def check_lambdas(lambdas):
    """lda_relevant_words' lambdas as a contiguous float64 array [L], refused
    before any native call: 1 <= L <= RELEVANCE_LAMBDAS_MAX, each finite and
    in [0, 1].  A scalar is one lambda."""
    import numpy as np
    lam = np.ascontiguousarray(np.atleast_1d(np.asarray(lambdas, dtype=np.float64)))
    if lam.ndim != 1 or not 1 <= lam.size <= RELEVANCE_LAMBDAS_MAX:
        raise ValueError(f"lambdas must be a scalar or a sequence of 1 to {RELEVANCE_LAMBDAS_MAX} values")
    if not np.all(np.isfinite(lam)) or np.any(lam < 0.0) or np.any(lam > 1.0):
        raise ValueError("every lambda must be finite and in [0, 1]")
    return lam


def topic_metric(metric) -> int:
    """LDA_TOPIC_* of a metric name or integer; an unknown one is refused
    before any native call."""
    if isinstance(metric, str):
        if metric not in TOPIC_METRICS:
            raise ValueError(f"metric must be one of {sorted(TOPIC_METRICS)}, not {metric!r}")
        return TOPIC_METRICS[metric]
    if isinstance(metric, (bool, float)) or int(metric) not in TOPIC_METRICS.values():
        raise ValueError(f"metric must be one of {sorted(TOPIC_METRICS)} or 0..3, not {metric!r}")
    return int(metric)


def topic_nearest_n(n) -> int:
    n = int(n)
    if not 1 <= n <= TOPIC_NEAREST_MAX:
        raise ValueError(f"n must be in [1, {TOPIC_NEAREST_MAX}]")
    return n


def doc_metric(metric) -> int:
    """The metric of the document calls (doc_distances, nearest_docs,
    doc_neighbors): a name of DOC_METRICS or its integer; an unknown one is
    refused before any native call."""
    if isinstance(metric, str):
        if metric not in DOC_METRICS:
            raise ValueError(f"metric must be one of {sorted(DOC_METRICS)}, not {metric!r}")
        return DOC_METRICS[metric]
    if isinstance(metric, (bool, float)) or int(metric) not in DOC_METRICS.values():
        raise ValueError(f"metric must be one of {sorted(DOC_METRICS)} or 0..2, not {metric!r}")
    return int(metric)


def doc_nearest_n(n) -> int:
    n = int(n)
    if not 1 <= n <= DOC_NEAREST_MAX:
        raise ValueError(f"n must be in [1, {DOC_NEAREST_MAX}]")
    return n


def doc_queries(theta, counts, K: int):
    """(theta fp64 [Q, K] or None, counts int32 [Q, K] or None) of the query
    rows of the document calls: exactly one must be given, and a wrong shape
    is refused before any native call."""
    if (theta is None) == (counts is None):
        raise ValueError("exactly one of theta and counts must be given")
    if theta is not None:
        return as_theta(theta, K), None
    c = np.asarray(counts)
    if c.ndim == 1:
        c = c[None, :]
    if c.ndim != 2 or c.shape[1] != K:
        raise ValueError(f"counts must have shape [Q, {K}], not {list(np.shape(counts))}")
    if not np.issubdtype(c.dtype, np.integer):
        raise ValueError("counts must be integers")
    if c.size and (c.min() < 0 or c.max() > np.iinfo(np.int32).max):
        raise ValueError("counts must be non-negative int32 values")
    return None, np.ascontiguousarray(c, dtype=np.int32)


def score_metric(metric) -> int:
    """LDA_SCORE_* of a metric name; an integer passes through, so that an
    unknown one reaches the library's own check."""
    if isinstance(metric, str):
        if metric not in SCORE_METRICS:
            raise ValueError(f"metric must be one of {sorted(SCORE_METRICS)}, not {metric!r}")
        return SCORE_METRICS[metric]
    return int(metric)


def as_theta(theta, K: int) -> np.ndarray:
    """theta as a C-contiguous fp64 [Q, K] array (a single row becomes Q = 1);
    a wrong shape is refused before any native call."""
    t = np.asarray(theta, dtype=np.float64)
    if t.ndim == 1:
        t = t[None, :]
    if t.ndim != 2 or t.shape[1] != K:
        raise ValueError(f"theta must have shape [Q, {K}], not {list(np.shape(theta))}")
    return np.ascontiguousarray(t)


def doc_completion_batch(C: int) -> int:
    """Tokens per batch of k_doc_completion for Kp = 64 C (lda_kernels.h
    doc_completion_batch): the document lengths around it are edge cases."""
    return 64 if C <= 8 else 16


def as_docs(doc_off, words, num_docs: int | None = None, what: str = "doc_off"):
    """(int64 doc_off[Dh + 1], int32 words) of a batch of documents as
    C-contiguous arrays; offsets that do not fit the words (or the expected
    number of documents) are refused before any native call."""
    off = np.ascontiguousarray(doc_off, dtype=np.int64).reshape(-1)
    w = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
    if len(off) < 1:
        raise ValueError(f"{what} must hold at least one offset")
    if num_docs is not None and len(off) != num_docs + 1:
        raise ValueError(f"{what} must have {num_docs + 1} entries, not {len(off)}")
    if int(off[-1]) - int(off[0]) != len(w):
        raise ValueError(f"{what} spans {int(off[-1]) - int(off[0])} tokens but words holds {len(w)}")
    return off, w


class LdaError(RuntimeError):
    def __init__(self, status: int, where: str, message: str):
        self.status = status
        super().__init__(f"{where}: {STATUS_NAMES.get(status, status)}: {message}")


class lda_config(C.Structure):
    _fields_ = [
        ("num_topics", C.c_int32),
        ("num_types", C.c_int32),
        ("num_docs", C.c_int64),
        ("alpha", C.POINTER(C.c_double)),
        ("beta", C.c_double),
        ("seed", C.c_uint64),
        ("device", C.c_int32),
        ("sampler", C.c_int32),
        ("token_base", C.c_int64),
        ("tokens_per_range", C.c_int64),
    ]


_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_vp = C.c_void_p

# name -> (restype, argtypes); every symbol include/lda_mi355x.h declares.
SIGNATURES = {
    "lda_create": (C.c_int32, [C.POINTER(_vp), C.POINTER(lda_config), _i64p, _vp, _vp]),
    "lda_destroy": (None, [_vp]),
    "lda_sweep": (C.c_int32, [_vp, C.c_int32]),
    "lda_sample": (C.c_int32, [_vp]),
    "lda_delta_buffer": (C.c_int32, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "lda_apply": (C.c_int32, [_vp]),
    "lda_set_exchange_parts": (C.c_int32, [_vp, C.c_int32, C.c_int32]),
    "lda_get_exchange_parts": (C.c_int32, [_vp, C.POINTER(C.c_int32)]),
    "lda_sample_part": (C.c_int32, [_vp, C.c_int32]),
    "lda_delta_buffer_part": (C.c_int32, [_vp, C.c_int32, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "lda_set_stream": (C.c_int32, [_vp, _vp]),
    "lda_get_stream": (C.c_int32, [_vp, C.POINTER(_vp)]),
    "lda_synchronize": (C.c_int32, [_vp]),
    "lda_get_sweep": (C.c_int32, [_vp, C.POINTER(C.c_uint32)]),
    "lda_set_sweep": (C.c_int32, [_vp, C.c_uint32]),
    "lda_padded_topics": (C.c_int32, [C.c_int32]),
    "lda_get_shape": (C.c_int32, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "lda_get_z": (C.c_int32, [_vp, _i32p]),
    "lda_set_z": (C.c_int32, [_vp, _i32p]),
    "lda_get_counts": (C.c_int32, [_vp, _vp, _vp, _vp, _vp]),
    "lda_set_alpha_beta": (C.c_int32, [_vp, _f64p, C.c_double]),
    "lda_log_likelihood_parts": (C.c_int32, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "lda_log_likelihood": (C.c_int32, [_vp, C.POINTER(C.c_double)]),
    "lda_log_likelihood_enqueue": (C.c_int32, [_vp, C.POINTER(C.c_int64)]),
    "lda_log_likelihood_collect": (C.c_int32, [_vp, C.c_int64, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double)]),
    "lda_infer": (C.c_int32, [_vp, C.c_int64, _i64p, _i32p, C.c_int32, C.c_int32, C.c_int32,
                              C.c_uint64, _f64p]),
    "lda_score_docs": (C.c_int32, [_vp, C.c_int32, C.c_int64, _vp, C.c_int64, C.c_int64, _vp, _vp]),
    "lda_heldout_loglik": (C.c_int32, [_vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "lda_doc_completion": (C.c_int32, [_vp, C.c_int64, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_uint64, _vp, _vp, _vp]),
    "lda_left_to_right": (C.c_int32, [_vp, C.c_int64, _vp, _vp, C.c_int32, C.c_int32, C.c_uint64, _vp, _vp, _vp,
                                      _vp, _vp]),
    "lda_debug_ltr_chunk_cells": (None, [C.c_int64]),
    "lda_top_words": (C.c_int32, [_vp, C.c_int32, _vp, _vp]),
    "lda_doc_top_topics": (C.c_int32, [_vp, C.c_int32, C.c_int64, C.c_int64, _vp, _vp, _vp]),
    "lda_doc_counts": (C.c_int32, [_vp, C.c_int64, C.c_int64, _vp, _vp]),
    "lda_topic_codocuments": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp]),
    "lda_topic_word_stats": (C.c_int32, [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "lda_word_cooccurrences": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp]),
    "lda_debug_cooc_chunk_tokens": (None, [C.c_int64]),
    "lda_topic_top_docs": (C.c_int32, [_vp, C.c_int32, C.c_double, C.c_int32, _vp, _vp, _vp]),
    "lda_debug_topic_docs_chunk_docs": (None, [C.c_int64]),
    "lda_topic_cooccurrence": (C.c_int32, [_vp, C.c_int64, C.c_int32, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lda_debug_topic_cooccurrence_global": (None, [C.c_int32]),
    "lda_group_topics": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int64, C.c_int32, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "lda_group_topics_path": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "lda_debug_group_topics_global": (None, [C.c_int32]),
    "lda_subcorpus_count": (C.c_int32, [_vp, _vp, C.c_int32]),
    "lda_subcorpus_merge": (C.c_int32, [_vp, _vp]),
    "lda_subcorpus_top_words": (C.c_int32, [_vp, C.c_int32, _vp, _vp, _vp]),
    "lda_subcorpus_release": (C.c_int32, [_vp]),
    "lda_relevant_words": (C.c_int32, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lda_salient_words": (C.c_int32, [_vp, C.c_int32, _vp, _vp, _vp, _vp]),
    "lda_word_rows": (C.c_int32, [_vp, C.c_int64, _vp, _vp, _vp]),
    "lda_debug_relevance_slab_rows": (None, [C.c_int64]),
    "lda_topic_phrases": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp]),
    "lda_phrase_counts": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp]),
    "lda_phrase_lookup": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "lda_debug_phrase_table_slots": (None, [C.c_int64]),
    "lda_topic_distances": (C.c_int32, [_vp, _vp, C.c_int32, _vp]),
    "lda_topic_nearest": (C.c_int32, [_vp, _vp, C.c_int32, C.c_int32, _vp, _vp]),
    "lda_topic_distance_slabs": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32)]),
    "lda_doc_distances": (C.c_int32, [_vp, C.c_int32, C.c_int64, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp]),
    "lda_doc_nearest": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "lda_doc_neighbors": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int64, C.c_int64, _vp, C.c_int32, _vp, _vp]),
    "lda_debug_doc_nearest_chunk": (None, [C.c_int64, C.c_int64]),
    "lda_to_mallet_packed": (C.c_int32, [_vp, _vp, _i64p, C.POINTER(C.c_int32)]),
    "lda_max_doc_length": (C.c_int32, [_vp, C.POINTER(C.c_int32)]),
    "lda_doc_topic_histograms": (C.c_int32, [_vp, C.c_int32, _i32p, _i32p]),
    "lda_doc_topic_histograms_accumulate": (C.c_int32, [_vp, C.c_int32]),
    "lda_doc_topic_histograms_take": (C.c_int32, [_vp, C.c_int32, _i32p, _i32p]),
    "lda_doc_topic_histograms_clear": (C.c_int32, [_vp]),
    "lda_count_histogram": (C.c_int32, [_vp, C.c_int64, _i32p]),
    "lda_hyper_statistics": (C.c_int32, [_vp, C.c_int32, _vp, _vp, C.c_int64, _vp, _vp]),
    "lda_learn_parameters": (C.c_int32, [_f64p, C.c_int32, _i32p, _i32p, C.c_int32, C.c_double,
                                         C.c_double, C.c_int32, C.POINTER(C.c_double)]),
    "lda_learn_symmetric_concentration": (C.c_int32, [_i32p, C.c_int64, _i64p, _i32p, C.c_int64,
                                                      C.c_int32, C.c_double,
                                                      C.POINTER(C.c_double)]),
    "lda_digamma": (C.c_double, [C.c_double]),
    "lda_last_sample_ms": (C.c_int32, [_vp, C.POINTER(C.c_float)]),
    "lda_row_stats": (C.c_int32, [_vp, C.POINTER(C.c_double)]),
    "lda_sample_times": (C.c_int32, [_vp, C.c_int32, _vp, C.POINTER(C.c_int32)]),
    "lda_philox_draws": (C.c_int32, [C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_int64, _vp]),
    "lda_recount_times": (C.c_int32, [_vp, C.c_int32, _vp, C.POINTER(C.c_int32)]),
    "lda_count_update_mode": (C.c_int32, [_vp, C.POINTER(C.c_int32)]),
    "lda_set_count_update": (C.c_int32, [_vp, C.c_int32, C.c_int32]),
    "lda_set_warm_start": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int64, C.c_int64]),
    "lda_get_warm_start": (C.c_int32, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lda_exchange_sizes": (C.c_int32, [_vp, C.c_int32, C.c_int64, C.POINTER(C.c_size_t),
                                       C.POINTER(C.c_size_t)]),
    "lda_exchange_pack": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int64, C.POINTER(_vp),
                                      C.POINTER(_vp)]),
    "lda_exchange_unpack": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int64, _vp]),
    "lda_exchange_unpack_lists": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_int64, _vp, C.c_int32]),
    "lda_set_exchange_cells": (C.c_int32, [_vp, C.c_int32]),
    "lda_get_exchange_cells": (C.c_int32, [_vp, C.POINTER(C.c_int32)]),
    "lda_counts_checksum": (C.c_int32, [_vp, C.POINTER(C.c_uint64)]),
    "lda_set_sequential_sweeps": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, C.c_int64]),
    "lda_get_sequential_sweeps": (C.c_int32, [_vp, C.POINTER(C.c_int32), _vp]),
    "lda_staleness_schedule": (C.c_int32, [C.c_int32, C.POINTER(C.c_int32), _vp]),
    "lda_warm_part_tokens": (C.c_int32, [_vp, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _vp]),
    "lda_sweep_parts": (C.c_int32, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lda_get_count_update": (C.c_int32, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lda_abi_version": (C.c_int32, []),
    "lda_debug_fail_host_alloc": (None, [C.c_int32]),
    "lda_last_error": (C.c_char_p, []),
    "lda_version": (C.c_char_p, []),
}

_lib = None


def load(path: str | None = None):
    """Load liblda_mi355x.so; raises if it is missing (no CPU fallback).
    LDA_MI355X_LIB overrides the in-tree path (A/B runs of kernel variants)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("LDA_MI355X_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()')")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64
    # (soname libamdhip64.so.7, loaded by path through its $ORIGIN rpath).
    # Importing torch first makes our NEEDED libamdhip64.so.7 resolve to that
    # already-loaded copy; loading /opt/rocm's copy first would leave torch's
    # runtime without devices ("No HIP GPUs are available").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(status: int, where: str):
    if status != LDA_OK:
        msg = load().lda_last_error()
        raise LdaError(status, where, msg.decode() if msg else "")


def padded_topics(K: int) -> int:
    return int(load().lda_padded_topics(K))
