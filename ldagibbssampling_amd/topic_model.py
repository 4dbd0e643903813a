"""ParallelTopicModel / TopicInferencer / InstanceList: Python face of the
native host mirror (liblda_topic_model.so, include/lda_topic_model.h).

Method names and meaning follow Mallet 2.0.7 as the reference calls it
(src/cmu_ron/TrainAndPredict.java:108-177, 230-234;
src/cmu/TrainAndPredict.java:93-114, 258-274, 436), so the reference's
driver reads the same:

    model = ParallelTopicModel(500, 100, 1)
    model.addInstances(training)
    model.setOptimizeInterval(20)
    model.setNumThreads(4)          # GPU shards (min with the visible GPUs)
    model.setNumIterations(10000)
    model.estimate()
    inferencer = model.getInferencer()
    theta = inferencer.getSampledDistribution(instance, 100, 10, 10)

Everything runs in the C++ library; there is no Python sampling path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi
from .corpus import Corpus, parse_inverse_docs, read_inverse_docs

TM_LIB_PATH = os.path.join(os.path.dirname(capi.LIB_PATH), "liblda_topic_model.so")

_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_vp = C.c_void_p
_i32 = C.c_int32

# every symbol include/lda_topic_model.h declares
TM_SIGNATURES = {
    "ldatm_create": (_i32, [C.POINTER(_vp), _i32, C.c_double, C.c_double]),
    "ldatm_destroy": (None, [_vp]),
    "ldatm_set_alphabet": (_i32, [_vp, _i32, C.POINTER(C.c_char_p)]),
    "ldatm_add_instances": (_i32, [_vp, C.c_int64, _i64p, _vp, C.POINTER(C.c_char_p)]),
    "ldatm_set_num_iterations": (_i32, [_vp, _i32]),
    "ldatm_set_optimize_interval": (_i32, [_vp, _i32]),
    "ldatm_set_burnin_period": (_i32, [_vp, _i32]),
    "ldatm_set_save_sample_interval": (_i32, [_vp, _i32]),
    "ldatm_set_symmetric_alpha": (_i32, [_vp, _i32]),
    "ldatm_set_topic_display": (_i32, [_vp, _i32, _i32]),
    "ldatm_set_random_seed": (_i32, [_vp, C.c_int64]),
    "ldatm_set_num_threads": (_i32, [_vp, _i32]),
    "ldatm_set_sampler": (_i32, [_vp, _i32]),
    "ldatm_set_exchange_parts": (_i32, [_vp, _i32]),
    "ldatm_set_devices": (_i32, [_vp, _i32, _vp]),
    "ldatm_set_warm_start": (_i32, [_vp, _i32, _i32]),
    "ldatm_set_staleness_threads": (_i32, [_vp, _i32]),
    "ldatm_num_shards": (_i32, [_vp, C.POINTER(_i32)]),
    "ldatm_exchange_info": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(C.c_int64)]),
    "ldatm_plan_shards": (_i32, [_i32, _i32, C.c_int64, _i32, _i32, C.c_int64]),
    "ldatm_set_topics": (_i32, [_vp, C.c_int64, _vp]),
    "ldatm_set_hyper": (_i32, [_vp, _vp, C.c_double, C.c_double]),
    "ldatm_get_sweep": (_i32, [_vp, C.POINTER(C.c_uint32)]),
    "ldatm_set_sweep": (_i32, [_vp, C.c_uint32]),
    "ldatm_set_verbosity": (_i32, [_vp, _i32]),
    "ldatm_set_print_log_likelihood": (_i32, [_vp, _i32]),
    "ldatm_estimate": (_i32, [_vp]),
    "ldatm_get_ll_trace": (_i32, [_vp, _vp, _vp, _i32, C.POINTER(_i32)]),
    "ldatm_model_log_likelihood": (_i32, [_vp, C.POINTER(C.c_double)]),
    "ldatm_get_shape": (_i32, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(C.c_int64),
                              C.POINTER(C.c_int64)]),
    "ldatm_get_hyper": (_i32, [_vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ldatm_get_z": (_i32, [_vp, _i32p]),
    "ldatm_get_counts": (_i32, [_vp, _vp, _vp]),
    "ldatm_get_topic_probabilities": (_i32, [_vp, C.c_int64, _f64p]),
    "ldatm_top_words": (_i32, [_vp, _i32, _vp, _vp]),
    "ldatm_doc_top_topics": (_i32, [_vp, _i32, C.c_int64, _vp, _vp, _vp]),
    "ldatm_doc_counts": (_i32, [_vp, C.c_int64, _vp, _vp]),
    "ldatm_topic_distances": (_i32, [_vp, _vp, _i32, _vp]),
    "ldatm_nearest_topics": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "ldatm_topic_codocuments": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "ldatm_topic_statistics": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldatm_diagnostics_finish": (_i32, [_i32, _i32, _i32, C.c_double, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp]),
    "ldatm_topic_diagnostics": (_i32, [_vp, _i32, _vp, _vp]),
    "ldatm_word_cooccurrences": (_i32, [_vp, _i32, _vp, _i32, C.c_int64, _vp, _vp, _vp, _vp]),
    "ldatm_coherence_finish": (_i32, [_i32, _i32, _i32, C.c_double, _vp, C.c_int64, _vp, _vp]),
    "ldatm_topic_coherence": (_i32, [_vp, _i32, _i32, _i32, C.c_double, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp]),
    "ldatm_print_document_topics": (_i32, [_vp, C.c_char_p, C.c_double, _i32]),
    "ldatm_document_topics_text": (_i32, [_vp, C.c_double, _i32, _vp, C.c_size_t,
                                          C.POINTER(C.c_size_t)]),
    "ldatm_print_top_words": (_i32, [_vp, C.c_char_p, _i32, _i32]),
    "ldatm_top_words_text": (_i32, [_vp, _i32, _i32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ldatm_document_distances": (_i32, [_vp, _i32, C.c_int64, _vp, _vp, C.c_int64, _vp, _vp]),
    "ldatm_nearest_documents": (_i32, [_vp, _i32, _i32, C.c_int64, _vp, _vp, _vp, _i32, _vp, _vp]),
    "ldatm_document_neighbors": (_i32, [_vp, _i32, _i32, C.c_int64, _vp, _i32, _vp, _vp]),
    "ldatm_document_neighbors_text": (_i32, [_vp, _i32, _i32, _i32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ldatm_print_document_neighbors": (_i32, [_vp, C.c_char_p, _i32, _i32, _i32]),
    "ldatm_document_neighbors_format": (_i32, [C.c_int64, _i32, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_size_t,
                                               C.POINTER(C.c_size_t)]),
    "ldatm_topic_top_docs": (_i32, [_vp, _i32, C.c_double, _i32, _vp, _vp, _vp]),
    "ldatm_relevant_words": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldatm_salient_words": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "ldatm_word_rows": (_i32, [_vp, C.c_int64, _vp, _vp, _vp]),
    "ldatm_print_relevant_words": (_i32, [_vp, C.c_char_p, _i32, C.c_double]),
    "ldatm_relevant_words_text": (_i32, [_vp, _i32, C.c_double, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ldatm_relevant_words_format": (_i32, [_i32, _i32, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, _vp,
                                           C.c_size_t, C.POINTER(C.c_size_t)]),
    "ldatm_print_topic_documents": (_i32, [_vp, C.c_char_p, _i32, C.c_double, _i32]),
    "ldatm_topic_documents_text": (_i32, [_vp, _i32, C.c_double, _i32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ldatm_topic_documents_format": (_i32, [_i32, _i32, C.c_double, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "ldatm_topic_phrases": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldatm_topic_phrases_text": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ldatm_print_topic_phrases": (_i32, [_vp, C.c_char_p, _i32, _i32, _i32, _i32]),
    "ldatm_topic_phrases_format": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, C.c_int64, _vp, C.c_size_t,
                                          C.POINTER(C.c_size_t)]),
    "ldatm_topic_phrases_bound": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ldatm_topic_cooccurrence": (_i32, [_vp, C.c_int64, _i32, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldatm_topic_correlation_finish": (_i32, [_i32, _i32, C.c_int64, _vp, _vp, _i32, _vp, _vp]),
    "ldatm_topic_correlations": (_i32, [_vp, _i32, C.c_int64, _i32, C.c_double, _vp]),
    "ldatm_topic_partners": (_i32, [_vp, _i32, C.c_int64, _i32, C.c_double, _i32, _vp, _vp]),
    "ldatm_topic_partners_select": (_i32, [_i32, _i32, _vp, _vp, _vp]),
    "ldatm_topic_correlations_text": (_i32, [_vp, _i32, _i32, C.c_int64, _i32, C.c_double, _vp, C.c_size_t,
                                             C.POINTER(C.c_size_t)]),
    "ldatm_print_topic_correlations": (_i32, [_vp, C.c_char_p, _i32, _i32, C.c_int64, _i32, C.c_double]),
    "ldatm_topic_correlations_format": (_i32, [_i32, _i32, _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ldatm_group_topics": (_i32, [_vp, _vp, _i32, C.c_int64, _i32, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "ldatm_group_prevalence_finish": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldatm_group_prevalence": (_i32, [_vp, _vp, _i32, _i32, C.c_int64, _i32, C.c_double, _vp]),
    "ldatm_group_top_topics_select": (_i32, [_i32, _i32, _i32, _vp, _vp, _vp]),
    "ldatm_group_topics_text": (_i32, [_vp, _vp, _i32, _i32, _i32, C.c_int64, _i32, C.c_double, _vp, C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "ldatm_print_group_topics": (_i32, [_vp, C.c_char_p, _vp, _i32, _i32, _i32, C.c_int64, _i32, C.c_double]),
    "ldatm_group_topics_format": (_i32, [_i32, _i32, _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ldatm_subcorpus_top_words": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "ldatm_save": (_i32, [_vp, C.c_char_p]),
    "ldatm_load": (_i32, [C.POINTER(_vp), C.c_char_p]),
    "ldatm_infer": (_i32, [_vp, C.c_int64, _i64p, _vp, _i32, _i32, _i32, C.c_uint64, _f64p]),
    "ldatm_score_theta": (_i32, [_vp, _i32, C.c_int64, _vp, C.c_int64, _vp, _vp]),
    "ldatm_score": (_i32, [_vp, _i32, C.c_int64, _vp, _vp, _i32, _i32, _i32, C.c_uint64, C.c_int64, _vp,
                           _vp, _vp]),
    "ldatm_score_top": (_i32, [_vp, _i32, C.c_int64, _vp, _i32, _vp, _vp]),
    "ldatm_heldout_loglik": (_i32, [_vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "ldatm_evaluate": (_i32, [_vp, C.c_int64, _vp, _vp, _i32, _i32, _i32, C.c_uint64, _vp, _vp, _vp, _vp]),
    "ldatm_left_to_right": (_i32, [_vp, C.c_int64, _vp, _vp, _i32, _i32, C.c_uint64, _vp, _vp, _vp]),
    "ldatm_completion_split": (_i32, [_i32, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldatm_set_held_out": (_i32, [_vp, C.c_int64, _vp, _vp, _i32, _i32, _i32, _i32, C.c_uint64]),
    "ldatm_get_held_out_trace": (_i32, [_vp, _vp, _vp, _i32, C.POINTER(_i32)]),
    "ldatm_format_double": (_i32, [C.c_double, _i32, C.c_char_p, C.c_size_t]),
    "ldatm_last_error": (C.c_char_p, []),
}

_tm = None


def load_tm(path: str = TM_LIB_PATH):
    """Load liblda_topic_model.so (after the sampler library and torch)."""
    global _tm
    if _tm is not None:
        return _tm
    capi.load()                     # torch first, then liblda_mi355x.so (one HIP runtime)
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build the native libraries first "
                          "(python -c 'import __graft_entry__ as g; g.build()')")
    L = C.CDLL(path)
    for name, (res, args) in TM_SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _tm = L
    return L


def _check(status: int, where: str):
    if status != capi.LDA_OK:
        msg = load_tm().ldatm_last_error()
        raise capi.LdaError(status, where, msg.decode() if msg else "")


def format_double(x: float, style: int = 0) -> str:
    """Java Double.toString (style 0) / Mallet's 5-digit NumberFormat (style 1)."""
    buf = C.create_string_buffer(128)
    _check(load_tm().ldatm_format_double(float(x), int(style), buf, 128), "ldatm_format_double")
    return buf.value.decode()


def topic_document_weights(K: int, smoothing: float, docs, counts, lengths) -> np.ndarray:
    """lda_topic_top_docs' weight (n_dk + smoothing) / (L_d + K smoothing) of
    every slot, float64, with K smoothing formed first; NaN where the id is -1."""
    docs = np.asarray(docs)
    ks = float(K) * float(smoothing)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (np.asarray(counts, np.float64) + float(smoothing)) / (np.asarray(lengths, np.float64) + ks)
    return np.where(docs >= 0, w, np.nan)


def format_topic_documents(docs, counts, lengths, smoothing: float = 10.0, names=None) -> str:
    """ldatm_topic_documents_format (host only, no device): printTopicDocuments'
    text from [K, n] arrays as topicDocuments returns them; names[d] is
    document d's name column (None, or no entry: "null-source")."""
    ids = np.ascontiguousarray(docs, np.int64)
    cnt = np.ascontiguousarray(counts, np.int32)
    lens = np.ascontiguousarray(lengths, np.int32)
    if ids.ndim != 2 or cnt.shape != ids.shape or lens.shape != ids.shape:
        raise ValueError("docs, counts and lengths must be [K, n] arrays of one shape")
    K, n = ids.shape
    names = list(names or [])
    arr = (C.c_char_p * max(len(names), 1))(*[None if s is None else str(s).encode() for s in names])
    L = load_tm()
    size = C.c_size_t()
    args = (K, n, float(smoothing), ids.ctypes.data, cnt.ctypes.data, lens.ctypes.data,
            C.cast(arr, C.c_void_p), len(names))
    _check(L.ldatm_topic_documents_format(*args, None, 0, C.byref(size)), "ldatm_topic_documents_format")
    buf = C.create_string_buffer(size.value + 1)
    _check(L.ldatm_topic_documents_format(*args, buf, size.value + 1, C.byref(size)), "ldatm_topic_documents_format")
    return buf.value.decode()


def format_document_neighbors(neighbors, values, docs=None, names=None) -> str:
    """ldatm_document_neighbors_format (host only, no device):
    printDocumentNeighbors' text from [M, n] arrays as documentNeighbors returns
    them; docs[M] are the query documents (None: 0 .. M-1), names[d] document
    d's name column (None, or no entry: "null-source")."""
    ids = np.ascontiguousarray(neighbors, np.int64)
    vals = np.ascontiguousarray(values, np.float64)
    if ids.ndim != 2 or vals.shape != ids.shape or ids.shape[1] < 1:
        raise ValueError("neighbors and values must be [M, n] arrays of one shape, n >= 1")
    M, n = ids.shape
    q = None
    if docs is not None:
        q = np.ascontiguousarray(docs, np.int64).reshape(-1)
        if len(q) != M:
            raise ValueError(f"docs must hold one id per row ({M})")
    names = list(names or [])
    arr = (C.c_char_p * max(len(names), 1))(*[None if s is None else str(s).encode() for s in names])
    L = load_tm()
    size = C.c_size_t()
    args = (M, n, q.ctypes.data if q is not None and M else None, ids.ctypes.data if M else None,
            vals.ctypes.data if M else None, C.cast(arr, C.c_void_p), len(names))
    _check(L.ldatm_document_neighbors_format(*args, None, 0, C.byref(size)), "ldatm_document_neighbors_format")
    buf = C.create_string_buffer(size.value + 1)
    _check(L.ldatm_document_neighbors_format(*args, buf, size.value + 1, C.byref(size)),
           "ldatm_document_neighbors_format")
    return buf.value.decode()


def format_topic_phrases(words, lengths, counts, names=None) -> str:
    """ldatm_topic_phrases_format (host only, no device): printTopicPhrases'
    text from words[K, n, max_len], lengths[K, n] and counts[K, n] as
    topicPhrases returns them; names[w] is word w's text (None, or no entry:
    the id)."""
    w = np.ascontiguousarray(words, np.int32)
    lens = np.ascontiguousarray(lengths, np.int32)
    cnt = np.ascontiguousarray(counts, np.int64)
    if w.ndim != 3 or lens.shape != w.shape[:2] or cnt.shape != w.shape[:2]:
        raise ValueError("words must be [K, n, max_len], lengths and counts [K, n]")
    K, n, max_len = w.shape
    names = list(names or [])
    arr = (C.c_char_p * max(len(names), 1))(*[None if s is None else str(s).encode() for s in names])
    L = load_tm()
    size = C.c_size_t()
    args = (K, n, max_len, w.ctypes.data, lens.ctypes.data, cnt.ctypes.data, C.cast(arr, C.c_void_p), len(names))
    _check(L.ldatm_topic_phrases_format(*args, None, 0, C.byref(size)), "ldatm_topic_phrases_format")
    buf = C.create_string_buffer(size.value + 1)
    _check(L.ldatm_topic_phrases_format(*args, buf, size.value + 1, C.byref(size)), "ldatm_topic_phrases_format")
    return buf.value.decode()


def topic_phrases_bound(shard_counts, totals):
    """ldatm_topic_phrases_bound (host only): from the shards' listed counts
    shard_counts[G, K, PHRASES_MAX] and the merged totals[K, n], (B[K] int64,
    proven[K] int32): B_k sums the shards' 128th counts (0 for a list that is
    not full) and bounds every phrase outside the united lists; proven[k] is
    the number of leading totals strictly above B_k, n where B_k = 0."""
    sc = np.ascontiguousarray(shard_counts, np.int64)
    tot = np.ascontiguousarray(totals, np.int64)
    if sc.ndim != 3 or sc.shape[2] != capi.PHRASES_MAX or tot.ndim != 2 or tot.shape[0] != sc.shape[1]:
        raise ValueError("shard_counts must be [G, K, PHRASES_MAX] and totals [K, n]")
    G, K, _ = sc.shape
    bound = np.zeros(K, np.int64)
    proven = np.zeros(K, np.int32)
    _check(load_tm().ldatm_topic_phrases_bound(K, tot.shape[1], G, sc.ctypes.data, tot.ctypes.data,
                                               bound.ctypes.data, proven.ctypes.data), "ldatm_topic_phrases_bound")
    return bound, proven


def format_relevant_words(word_ids, counts, totals, logprob, loglift, lambda_: float = 0.6, names=None) -> str:
    """ldatm_relevant_words_format (host only, no device): printRelevantWords'
    text from one lambda's [K, n] arrays as relevantWords returns them;
    names[w] is word w's text (None, or no entry: the id)."""
    ids = np.ascontiguousarray(word_ids, np.int32)
    cnt = np.ascontiguousarray(counts, np.int32)
    tot = np.ascontiguousarray(totals, np.int64)
    lp = np.ascontiguousarray(logprob, np.float64)
    ll = np.ascontiguousarray(loglift, np.float64)
    if ids.ndim != 2 or any(a.shape != ids.shape for a in (cnt, tot, lp, ll)):
        raise ValueError("word_ids, counts, totals, logprob and loglift must be [K, n] arrays of one shape")
    K, n = ids.shape
    names = list(names or [])
    arr = (C.c_char_p * max(len(names), 1))(*[None if s is None else str(s).encode() for s in names])
    L = load_tm()
    size = C.c_size_t()
    args = (K, n, float(lambda_), ids.ctypes.data, cnt.ctypes.data, tot.ctypes.data, lp.ctypes.data, ll.ctypes.data,
            C.cast(arr, C.c_void_p), len(names))
    _check(L.ldatm_relevant_words_format(*args, None, 0, C.byref(size)), "ldatm_relevant_words_format")
    buf = C.create_string_buffer(size.value + 1)
    _check(L.ldatm_relevant_words_format(*args, buf, size.value + 1, C.byref(size)), "ldatm_relevant_words_format")
    return buf.value.decode()


def classical_mds(dist) -> tuple:
    """Classical (Torgerson) scaling of a symmetric K x K distance matrix to
    two axes: B = -1/2 J D^2 J with J = I - 11'/K, numpy.linalg.eigh, the two
    largest eigenvalues' vectors times sqrt(max(eigenvalue, 0)).  Each axis's
    sign makes its entry of largest magnitude (the lowest index on a tie)
    positive.  K = 1: both axes 0; K = 2: the y axis 0.  Returns (x[K], y[K])."""
    D = np.asarray(dist, np.float64)
    K = D.shape[0]
    if D.ndim != 2 or D.shape[1] != K or K < 1:
        raise ValueError("dist must be a square matrix")
    x, y = np.zeros(K), np.zeros(K)
    if K == 1:
        return x, y
    J = np.eye(K) - np.full((K, K), 1.0 / K)
    w, v = np.linalg.eigh(-0.5 * (J @ (D * D) @ J))
    axes = []
    for j in (K - 1, K - 2)[:2 if K > 2 else 1]:
        a = v[:, j] * np.sqrt(max(w[j], 0.0))
        if a[int(np.argmax(np.abs(a)))] < 0:
            a = -a
        axes.append(a + 0.0)
    x = axes[0]
    if len(axes) > 1:
        y = axes[1]
    return x, y


def vis_lambdas(step: float) -> np.ndarray:
    """prepareVis' slider values 0, step, 2 step, ..., closed by 1.0: i * step
    for i = 0 .. floor(1 / step + 1e-9), values above 1 taken as 1, and 1.0
    appended when the last value is below it."""
    step = float(step)
    if not (np.isfinite(step) and 0.0 < step <= 1.0):
        raise ValueError("lambdaStep must be in (0, 1]")
    lam = [min(1.0, i * step) for i in range(int(np.floor(1.0 / step + 1e-9)) + 1)]
    if lam[-1] < 1.0:
        lam.append(1.0)
    return np.array(lam, np.float64)


class TopicRelevance:
    """relevantWords' result: lambdas[L]; wordIds, counts (nw[w, k]) int32,
    totals (tw[w]) int64, logprob, loglift float64, each [L, K, n], -1 / 0 / 0
    / 0.0 / 0.0 past a topic's last candidate.  relevance(l): plane l's
    [K, n] relevance, logprob - (1 - lambda) (logprob - loglift), NaN in an
    empty slot."""

    def __init__(self, lambdas, wordIds, counts, totals, logprob, loglift):
        self.lambdas, self.wordIds, self.counts, self.totals = lambdas, wordIds, counts, totals
        self.logprob, self.loglift = logprob, loglift

    def relevance(self, l: int = 0) -> np.ndarray:
        lp, ll = self.logprob[l], self.loglift[l]
        r = lp - (1.0 - float(self.lambdas[l])) * (lp - ll)
        return np.where(self.wordIds[l] >= 0, r, np.nan)


class TopicPhrases:
    """getTopicPhrases' result: phrases[k] = [(text, count), ...], wordIds[k] =
    [tuple of word ids, ...], counts[K, n], first[K, n] (smallest global token
    index; -1 in an empty slot), runs[K], distinct[K] (-1 with several
    shards), skippedLong, proven[K]."""

    def __init__(self, phrases, wordIds, counts, first, runs, distinct, skippedLong, proven):
        self.phrases, self.wordIds, self.counts, self.first = phrases, wordIds, counts, first
        self.runs, self.distinct, self.skippedLong, self.proven = runs, distinct, skippedLong, proven


# LDATM_CORR_* / LDATM_COOC_* of lda_topic_model.h, and the table each measure takes
CORR_MEASURES = {"pmi": 0, "npmi": 1, "jaccard": 2, "overlap": 3, "cosine": 4, "pearson": 5}
COOC_TABLES = {"codocs": 0, "overlap": 1, "product": 2}
MEASURE_TABLE = {"pmi": "codocs", "npmi": "codocs", "jaccard": "codocs", "overlap": "overlap",
                 "cosine": "product", "pearson": "product"}


def correlation_measure(measure) -> str:
    """A measure of topic co-occurrence by name."""
    if measure not in CORR_MEASURES:
        raise ValueError(f"unknown measure {measure!r}: one of {tuple(CORR_MEASURES)}")
    return measure


def topic_correlation_finish(measure, docs_used, tokens, present, table, kind=None) -> np.ndarray:
    """ldatm_topic_correlation_finish (host only, no device): the float64
    [K, K] matrix of a measure ("pmi", "npmi", "jaccard" from codocs; "overlap"
    from overlap; "cosine", "pearson" from product) out of
    topic_cooccurrence's integers.  kind names the table that `table` is
    (None: the measure's own); a wrong one is an error."""
    measure = correlation_measure(measure)
    kind = MEASURE_TABLE[measure] if kind is None else kind
    if kind not in COOC_TABLES:
        raise ValueError(f"unknown table {kind!r}: one of {tuple(COOC_TABLES)}")
    tok = np.ascontiguousarray(tokens, np.int64)
    pre = np.ascontiguousarray(present, np.int64)
    tab = np.ascontiguousarray(table, np.int64)
    K = tok.shape[0] if tok.ndim == 1 else -1
    if K < 1 or pre.shape != (K,) or tab.shape != (K, K):
        raise ValueError("tokens and present must be [K] and table [K, K]")
    out = np.zeros((K, K), np.float64)
    _check(load_tm().ldatm_topic_correlation_finish(CORR_MEASURES[measure], K, int(docs_used), tok.ctypes.data,
                                                    pre.ctypes.data, COOC_TABLES[kind], tab.ctypes.data,
                                                    out.ctypes.data), "ldatm_topic_correlation_finish")
    return out


def topic_partners_select(matrix, n: int):
    """ldatm_topic_partners_select (host only): per row k of a [K, K] matrix
    the n columns l != k with the largest finite values, larger first, equal
    values by smaller id.  Returns (ids int32 [K, n], values float64 [K, n]),
    -1 / NaN past the last."""
    mat = np.ascontiguousarray(matrix, np.float64)
    n = int(n)
    if mat.ndim != 2 or mat.shape[0] != mat.shape[1] or mat.shape[0] < 1:
        raise ValueError("matrix must be [K, K]")
    if n < 1:
        raise ValueError("n must be at least 1")
    K = mat.shape[0]
    ids = np.zeros((K, n), np.int32)
    values = np.zeros((K, n), np.float64)
    _check(load_tm().ldatm_topic_partners_select(K, n, mat.ctypes.data, ids.ctypes.data, values.ctypes.data),
           "ldatm_topic_partners_select")
    return ids, values


def format_topic_correlations(ids, values) -> str:
    """ldatm_topic_correlations_format (host only): printTopicCorrelations'
    text from [K, n] partner ids and values."""
    ids = np.ascontiguousarray(ids, np.int32)
    values = np.ascontiguousarray(values, np.float64)
    if ids.ndim != 2 or values.shape != ids.shape or ids.size == 0:
        raise ValueError("ids and values must be [K, n] arrays of one shape")
    K, n = ids.shape
    L = load_tm()
    size = C.c_size_t()
    args = (K, n, ids.ctypes.data, values.ctypes.data)
    _check(L.ldatm_topic_correlations_format(*args, None, 0, C.byref(size)), "ldatm_topic_correlations_format")
    buf = C.create_string_buffer(size.value + 1)
    _check(L.ldatm_topic_correlations_format(*args, buf, size.value + 1, C.byref(size)),
           "ldatm_topic_correlations_format")
    return buf.value.decode()


# LDATM_GROUP_* of lda_topic_model.h, and the optional table each kind takes
GROUP_KINDS = {"tokens": 0, "documents": 1, "mean": 2, "lift": 3}
GROUP_KIND_TABLE = {"tokens": None, "documents": "present", "mean": "shares", "lift": None}


def group_kind(kind) -> str:
    """A kind of group prevalence by name."""
    if kind not in GROUP_KINDS:
        raise ValueError(f"unknown kind {kind!r}: one of {tuple(GROUP_KINDS)}")
    return kind


def group_labels(groups) -> tuple:
    """(labels, ids int32 [D]) of one label per document: the sorted distinct
    labels that are not None, and per document its label's index, -1 for
    None."""
    groups = list(groups)
    distinct = {g for g in groups if g is not None}
    try:
        labels = sorted(distinct)
    except TypeError:                       # labels of several types: by type name, then text
        labels = sorted(distinct, key=lambda g: (type(g).__name__, str(g)))
    index = {g: i for i, g in enumerate(labels)}
    ids = np.fromiter((-1 if g is None else index[g] for g in groups), dtype=np.int32, count=len(groups))
    return labels, ids


def group_prevalence_finish(kind, group_docs, group_tokens, tokens, present=None, shares=None) -> np.ndarray:
    """ldatm_group_prevalence_finish (host only, no device): the float64
    [G, K] matrix of a kind out of group_topics' integers -- "tokens" =
    tokens / group_tokens, "documents" = present / group_docs, "mean" = shares /
    (2^32 group_docs), "lift" = log((tokens / group_tokens) / (N_k / N)).  NaN
    where a denominator is 0, lift -inf where tokens is 0.  A kind without its
    table is an error."""
    kind = group_kind(kind)
    gd = np.ascontiguousarray(group_docs, np.int64)
    gt = np.ascontiguousarray(group_tokens, np.int64)
    tok = np.ascontiguousarray(tokens, np.int64)
    if tok.ndim != 2 or tok.size == 0 or gd.shape != (tok.shape[0],) or gt.shape != (tok.shape[0],):
        raise ValueError("group_docs and group_tokens must be [G] and tokens [G, K]")
    pre = None if present is None else np.ascontiguousarray(present, np.int64)
    shr = None if shares is None else np.ascontiguousarray(shares, np.uint64)
    for t in (pre, shr):
        if t is not None and t.shape != tok.shape:
            raise ValueError("present and shares must be [G, K] as tokens")
    G, K = tok.shape
    out = np.zeros((G, K), np.float64)
    _check(load_tm().ldatm_group_prevalence_finish(GROUP_KINDS[kind], G, K, gd.ctypes.data, gt.ctypes.data,
                                                   tok.ctypes.data, None if pre is None else pre.ctypes.data,
                                                   None if shr is None else shr.ctypes.data, out.ctypes.data),
           "ldatm_group_prevalence_finish")
    return out


def group_top_topics_select(matrix, n: int):
    """ldatm_group_top_topics_select (host only): per row g of a [G, K] matrix
    the n columns with the largest finite values, larger first, equal values by
    smaller id.  Returns (ids int32 [G, n], values float64 [G, n]), -1 / NaN
    past the last."""
    mat = np.ascontiguousarray(matrix, np.float64)
    n = int(n)
    if mat.ndim != 2 or mat.size == 0:
        raise ValueError("matrix must be [G, K]")
    if n < 1:
        raise ValueError("n must be at least 1")
    G, K = mat.shape
    ids = np.zeros((G, n), np.int32)
    values = np.zeros((G, n), np.float64)
    _check(load_tm().ldatm_group_top_topics_select(G, K, n, mat.ctypes.data, ids.ctypes.data, values.ctypes.data),
           "ldatm_group_top_topics_select")
    return ids, values


def format_group_topics(ids, values) -> str:
    """ldatm_group_topics_format (host only): printGroupTopics' text from
    [G, n] topic ids and values."""
    ids = np.ascontiguousarray(ids, np.int32)
    values = np.ascontiguousarray(values, np.float64)
    if ids.ndim != 2 or values.shape != ids.shape or ids.size == 0:
        raise ValueError("ids and values must be [G, n] arrays of one shape")
    G, n = ids.shape
    L = load_tm()
    size = C.c_size_t()
    args = (G, n, ids.ctypes.data, values.ctypes.data)
    _check(L.ldatm_group_topics_format(*args, None, 0, C.byref(size)), "ldatm_group_topics_format")
    buf = C.create_string_buffer(size.value + 1)
    _check(L.ldatm_group_topics_format(*args, buf, size.value + 1, C.byref(size)), "ldatm_group_topics_format")
    return buf.value.decode()


class TopicsByGroup:
    """What ParallelTopicModel.topicsByGroup returns: labels (the groups, in
    the order of the rows), values (float64 [G, K] of the kind), groupDocs and
    groupTokens (int64 [G]: the used documents of each group and their tokens)
    and counts (the integer tables: "tokens" and, where counted, "present" and
    "shares", [G, K])."""

    def __init__(self, kind, labels, values, groupDocs, groupTokens, counts):
        self.kind, self.labels, self.values = kind, labels, values
        self.groupDocs, self.groupTokens, self.counts = groupDocs, groupTokens, counts


class Alphabet:
    """cc.mallet.types.Alphabet: word <-> id in insertion order."""

    def __init__(self, entries=()):
        self._ids: dict = {}
        self._words: list = []
        for e in entries:
            self.lookupIndex(e)

    def lookupIndex(self, entry, addIfNotPresent: bool = True) -> int:
        i = self._ids.get(entry)
        if i is None:
            if not addIfNotPresent:
                return -1
            i = len(self._words)
            self._ids[entry] = i
            self._words.append(entry)
        return i

    def lookupObject(self, index: int):
        return self._words[index]

    def size(self) -> int:
        return len(self._words)

    def toArray(self) -> list:
        return list(self._words)

    def __len__(self):
        return len(self._words)


class Instance:
    """Mallet Instance after the pipe: data = word ids (FeatureSequence)."""

    def __init__(self, data, target=None, name=None, source=None):
        self.data = np.ascontiguousarray(data, dtype=np.int32)
        self.target, self.name, self.source = target, name, source

    def getSource(self):
        return self.source


class InstanceList:
    """Tokenised documents over one data alphabet (InstanceList + its pipe).

    ``fromInverseDocs`` applies the reference's pipe: lines
    "<target>\\t<data>", tokens ``[^\\t]+`` lower-cased
    (src/cmu_ron/InstanceImporter.java:23-57, SFDCIterator.java:60-66).
    """

    def __init__(self, alphabet: Alphabet | None = None):
        self.alphabet = alphabet if alphabet is not None else Alphabet()
        self.instances: list = []

    def __len__(self):
        return len(self.instances)

    def __iter__(self):
        return iter(self.instances)

    def __getitem__(self, i):
        return self.instances[i]

    def getDataAlphabet(self) -> Alphabet:
        return self.alphabet

    def add(self, instance: Instance):
        self.instances.append(instance)

    def addTokens(self, tokens, target=None, name=None, source=None, grow: bool = True):
        ids = [self.alphabet.lookupIndex(t, grow) for t in tokens]
        self.add(Instance([i for i in ids if i >= 0], target, name, source))

    @classmethod
    def fromCorpus(cls, corpus: Corpus, alphabet: Alphabet | None = None) -> "InstanceList":
        if alphabet is None:
            alphabet = Alphabet(corpus.alphabet if corpus.alphabet else range(corpus.num_types))
        il = cls(alphabet)
        for d in range(corpus.num_docs):
            t = corpus.targets[d] if corpus.targets else None
            il.add(Instance(corpus.doc(d), t, f"example:{d}", None))
        return il

    @classmethod
    def fromInverseDocs(cls, path_or_text: str, alphabet: Alphabet | None = None,
                        grow: bool = True) -> "InstanceList":
        amap = None
        if alphabet is not None:
            amap = dict(alphabet._ids)
        is_path = "\n" not in path_or_text and os.path.exists(path_or_text)
        c = read_inverse_docs(path_or_text, amap, grow) if is_path else \
            parse_inverse_docs(path_or_text, amap, grow)
        if alphabet is not None:
            for w in c.alphabet[alphabet.size():]:
                alphabet.lookupIndex(w)
        return cls.fromCorpus(c, alphabet)


def _flatten(instances):
    lens = np.fromiter((len(i.data) for i in instances), dtype=np.int64, count=len(instances))
    off = np.zeros(len(instances) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    words = np.concatenate([i.data for i in instances]).astype(np.int32) if len(instances) \
        else np.zeros(0, np.int32)
    return off, np.ascontiguousarray(words)


class ParallelTopicModel:
    """Mallet 2.0.7 ParallelTopicModel over the GPU sampler (see module doc)."""

    def __init__(self, numberOfTopics: int, alphaSum: float | None = None, beta: float = 0.01):
        L = load_tm()
        self.numTopics = int(numberOfTopics)
        h = C.c_void_p()
        alpha_sum = float(numberOfTopics if alphaSum is None else alphaSum)
        _check(L.ldatm_create(C.byref(h), self.numTopics, alpha_sum, float(beta)), "ldatm_create")
        self._h, self._L = h, L
        self.alphabet: Alphabet | None = None
        self.data: list = []

    def close(self):
        if getattr(self, "_h", None):
            self._L.ldatm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ data
    def addInstances(self, training: InstanceList):
        """New documents get random topics; earlier documents keep theirs."""
        self.alphabet = training.getDataAlphabet()
        V = self.alphabet.size()
        words = (C.c_char_p * V)(*[str(w).encode() for w in self.alphabet.toArray()])
        _check(self._L.ldatm_set_alphabet(self._h, V, words), "ldatm_set_alphabet")
        new = [i for i in training]
        off, w = _flatten(new)
        src = (C.c_char_p * len(new))(*[None if i.source is None else str(i.source).encode()
                                        for i in new]) if new else None
        _check(self._L.ldatm_add_instances(self._h, len(new), off,
                                           w.ctypes.data if len(w) else None, src),
               "ldatm_add_instances")
        self.data.extend(new)

    def getAlphabet(self) -> Alphabet:
        return self.alphabet

    # ---------------------------------------------------------- options
    def setNumIterations(self, n): _check(self._L.ldatm_set_num_iterations(self._h, int(n)), "setNumIterations")
    def setOptimizeInterval(self, n): _check(self._L.ldatm_set_optimize_interval(self._h, int(n)), "setOptimizeInterval")
    def setBurninPeriod(self, n): _check(self._L.ldatm_set_burnin_period(self._h, int(n)), "setBurninPeriod")
    def setSaveSampleInterval(self, n): _check(self._L.ldatm_set_save_sample_interval(self._h, int(n)), "setSaveSampleInterval")
    def setSymmetricAlpha(self, on): _check(self._L.ldatm_set_symmetric_alpha(self._h, int(bool(on))), "setSymmetricAlpha")
    def setTopicDisplay(self, interval, n): _check(self._L.ldatm_set_topic_display(self._h, int(interval), int(n)), "setTopicDisplay")
    def setRandomSeed(self, seed): _check(self._L.ldatm_set_random_seed(self._h, int(seed)), "setRandomSeed")
    def setNumThreads(self, n): _check(self._L.ldatm_set_num_threads(self._h, int(n)), "setNumThreads")
    def setVerbosity(self, level): _check(self._L.ldatm_set_verbosity(self._h, int(level)), "setVerbosity")
    def setPrintLogLikelihood(self, on): _check(self._L.ldatm_set_print_log_likelihood(self._h, int(bool(on))), "setPrintLogLikelihood")

    def setSampler(self, kind: str):
        _check(self._L.ldatm_set_sampler(self._h, capi.SAMPLERS[kind]), "setSampler")

    def setExchangeParts(self, parts: int):
        """Split sweeps across GPU shards (exchange overlapped with sampling)."""
        _check(self._L.ldatm_set_exchange_parts(self._h, int(parts)), "setExchangeParts")

    def setDevices(self, devices):
        """Explicit shard placement: shard g on HIP device devices[g] (an empty
        list returns to setNumThreads' plan).  Shards that all share one device
        exchange through a device-side sum (the multi-shard path on one GPU)."""
        d = np.ascontiguousarray(list(devices), dtype=np.int32)
        _check(self._L.ldatm_set_devices(self._h, len(d), d.ctypes.data if len(d) else None),
               "setDevices")

    def setWarmStart(self, parts: int, sweeps: int):
        """Sweeps 0..sweeps-1 in `parts` sequential parts (default 4 x 50; (1, 0) = off)."""
        _check(self._L.ldatm_set_warm_start(self._h, int(parts), int(sweeps)), "setWarmStart")

    def setStalenessThreads(self, threads: int):
        """Sweeps past the warm start with the staleness of Mallet's T worker
        threads (0 = setNumThreads' T, the default; < 0 = snapshot sweeps)."""
        _check(self._L.ldatm_set_staleness_threads(self._h, int(threads)), "setStalenessThreads")

    def numShards(self) -> int:
        n = C.c_int32()
        _check(self._L.ldatm_num_shards(self._h, C.byref(n)), "numShards")
        return n.value

    def exchangeInfo(self) -> dict:
        """The shards' compact exchange (ldatm_exchange_info): cells per
        packed word (0: none), used-length escape lists, the largest escape
        count gathered, the count reads so far."""
        c, u, m, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        _check(self._L.ldatm_exchange_info(self._h, C.byref(c), C.byref(u), C.byref(m), C.byref(n)),
               "exchangeInfo")
        return {"cells_per_word": c.value, "used_lists": bool(u.value), "escapes_max": m.value,
                "list_exchanges": n.value}

    # --------------------------------------------------------- training
    def estimate(self):
        _check(self._L.ldatm_estimate(self._h), "estimate")

    def llTrace(self):
        """[(iteration, LL/token)] of the last estimate() (every 10 sweeps)."""
        n = C.c_int32()
        _check(self._L.ldatm_get_ll_trace(self._h, None, None, 0, C.byref(n)), "ldatm_get_ll_trace")
        it = np.zeros(n.value, np.int32)
        ll = np.zeros(n.value, np.float64)
        if n.value:
            _check(self._L.ldatm_get_ll_trace(self._h, it.ctypes.data, ll.ctypes.data, n.value,
                                              C.byref(n)), "ldatm_get_ll_trace")
        return list(zip(it.tolist(), ll.tolist()))

    def modelLogLikelihood(self) -> float:
        out = C.c_double()
        _check(self._L.ldatm_model_log_likelihood(self._h, C.byref(out)), "modelLogLikelihood")
        return out.value

    # ------------------------------------------------------------ state
    def _shape(self):
        K, V, D, N = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        _check(self._L.ldatm_get_shape(self._h, C.byref(K), C.byref(V), C.byref(D), C.byref(N)),
               "ldatm_get_shape")
        return K.value, V.value, D.value, N.value

    @property
    def alpha(self) -> np.ndarray:
        a = np.zeros(self.numTopics, np.float64)
        _check(self._L.ldatm_get_hyper(self._h, a.ctypes.data, None, None), "ldatm_get_hyper")
        return a

    @property
    def alphaSum(self) -> float:
        s = C.c_double()
        _check(self._L.ldatm_get_hyper(self._h, None, C.byref(s), None), "ldatm_get_hyper")
        return s.value

    @property
    def beta(self) -> float:
        b = C.c_double()
        _check(self._L.ldatm_get_hyper(self._h, None, None, C.byref(b)), "ldatm_get_hyper")
        return b.value

    def topicAssignments(self) -> np.ndarray:
        """z of every token (TopicAssignment.topicSequence, concatenated)."""
        z = np.zeros(self._shape()[3], np.int32)
        _check(self._L.ldatm_get_z(self._h, z), "ldatm_get_z")
        return z

    def typeTopicCounts(self):
        """(nw[V, K], tokensPerTopic[K]) dense."""
        K, V, _, _ = self._shape()
        nw = np.zeros((V, K), np.int32)
        nwsum = np.zeros(K, np.int32)
        _check(self._L.ldatm_get_counts(self._h, nw.ctypes.data, nwsum.ctypes.data), "ldatm_get_counts")
        return nw, nwsum

    def getTopicProbabilities(self, doc: int) -> np.ndarray:
        out = np.zeros(self.numTopics, np.float64)
        _check(self._L.ldatm_get_topic_probabilities(self._h, int(doc), out), "getTopicProbabilities")
        return out

    # ------------------------------- readouts selected on the device
    def topWords(self, numWords: int):
        """ldatm_top_words: (word_ids[K, numWords], counts[K, numWords]) int32,
        count descending, equal counts by ascending word id; -1 / 0 past a
        topic's last nonzero word.  Only these 2 K numWords numbers leave the
        device."""
        n = int(numWords)
        if not 1 <= n <= capi.TOP_WORDS_MAX:
            raise ValueError(f"numWords must be in [1, {capi.TOP_WORDS_MAX}]")
        ids = np.zeros((self.numTopics, n), np.int32)
        cnt = np.zeros((self.numTopics, n), np.int32)
        _check(self._L.ldatm_top_words(self._h, n, ids.ctypes.data, cnt.ctypes.data), "topWords")
        return ids, cnt

    def getTopWords(self, numWords: int) -> list:
        """Per topic a list of (word, count), at most numWords long, heaviest
        first: the alphabet's entry, or the word id without an alphabet."""
        ids, cnt = self.topWords(numWords)
        name = (lambda w: w) if self.alphabet is None else self.alphabet.lookupObject
        return [[(name(int(w)), int(c)) for w, c in zip(ids[k], cnt[k]) if w >= 0]
                for k in range(self.numTopics)]

    def docCounts(self, docs=None) -> np.ndarray:
        """ldatm_doc_counts: nd[M, K] (int32) of the documents `docs` (global
        ids, any order; None = all), built on the device from z."""
        ids, M = _doc_ids(docs, self)
        nd = np.zeros((M, self.numTopics), np.int32)
        _check(self._L.ldatm_doc_counts(self._h, M, ids.ctypes.data if ids is not None and M else None,
                                        nd.ctypes.data), "docCounts")
        return nd

    def docTopTopics(self, n: int, docs=None):
        """ldatm_doc_top_topics: (topics[M, n], counts[M, n]) int32 of the
        documents `docs` (global ids; None = all): the n topics with the largest
        weight, equal weights by ascending topic; -1 / 0 past K."""
        n = int(n)
        if not 1 <= n <= capi.TOP_TOPICS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOP_TOPICS_MAX}]")
        ids, M = _doc_ids(docs, self)
        topics = np.zeros((M, n), np.int32)
        cnt = np.zeros((M, n), np.int32)
        _check(self._L.ldatm_doc_top_topics(self._h, n, M, ids.ctypes.data if ids is not None and M else None,
                                            topics.ctypes.data, cnt.ctypes.data), "docTopTopics")
        return topics, cnt

    # ------------------------------- top documents per topic
    def topicDocuments(self, n: int, smoothing: float = 10.0, minTokens: int = 1):
        """ldatm_topic_top_docs: per topic the n documents with a token of the
        topic and at least minTokens tokens that have the largest weight
        (n_dk + smoothing) / (L_d + K smoothing), equal weights by ascending
        document id, selected on the device.  Returns (docs[K, n] int64 global
        ids, weights[K, n] float64, counts[K, n] int32, lengths[K, n] int32);
        -1 / NaN / 0 / 0 past a topic's last candidate.  The weights are
        recomputed here from the counts and lengths."""
        n = int(n)
        if not 1 <= n <= capi.TOPIC_DOCS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOPIC_DOCS_MAX}]")
        K = self.numTopics
        docs = np.zeros((K, n), np.int64)
        cnt = np.zeros((K, n), np.int32)
        lens = np.zeros((K, n), np.int32)
        _check(self._L.ldatm_topic_top_docs(self._h, n, float(smoothing), int(minTokens), docs.ctypes.data,
                                            cnt.ctypes.data, lens.ctypes.data), "topicDocuments")
        return docs, topic_document_weights(K, smoothing, docs, cnt, lens), cnt, lens

    def getTopicDocuments(self, n: int = 100, smoothing: float = 10.0, minTokens: int = 1) -> list:
        """Per topic a list of (doc, weight), at most n long, heaviest first."""
        docs, w, _, _ = self.topicDocuments(n, smoothing, minTokens)
        return [[(int(d), float(x)) for d, x in zip(docs[k], w[k]) if d >= 0] for k in range(self.numTopics)]

    # ------------------------------- relevance, saliency, LDAvis
    def relevantWords(self, n: int, lambdas=0.6) -> TopicRelevance:
        """ldatm_relevant_words: for each lambda (a scalar or up to
        RELEVANCE_LAMBDAS_MAX values in [0, 1]) and topic the n words with
        nw[w, k] > 0 of largest relevance lambda logprob + (1 - lambda) loglift,
        equal keys by ascending word id, selected on the device."""
        n = int(n)
        if not 1 <= n <= capi.TOP_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOP_WORDS_MAX}]")
        lam = capi.check_lambdas(lambdas)
        shape = (lam.size, self.numTopics, n)
        ids, cnt = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
        tot = np.zeros(shape, np.int64)
        lp, ll = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
        _check(self._L.ldatm_relevant_words(self._h, n, lam.size, lam.ctypes.data, ids.ctypes.data, cnt.ctypes.data,
                                            tot.ctypes.data, lp.ctypes.data, ll.ctypes.data), "relevantWords")
        return TopicRelevance(lam, ids, cnt, tot, lp, ll)

    def _word(self, w: int):
        return int(w) if self.alphabet is None else self.alphabet.lookupObject(int(w))

    def getRelevantWords(self, n: int = 10, lambda_: float = 0.6) -> list:
        """Per topic a list of (word, relevance), at most n long, most relevant
        first: the alphabet's entry, or the word id without an alphabet."""
        if np.ndim(lambda_) != 0:
            raise ValueError("lambda_ must be one value")
        r = self.relevantWords(n, lambda_)
        rel = r.relevance(0)
        return [[(self._word(w), float(x)) for w, x in zip(r.wordIds[0, k], rel[k]) if w >= 0]
                for k in range(self.numTopics)]

    def salientWords(self, n: int = 30):
        """ldatm_salient_words: (word_ids[n] int32, totals[n] int64,
        saliency[n], distinctiveness[n] float64) of the n most salient words
        (Chuang et al. 2012), equal values by ascending id; -1 / 0 / 0.0 / 0.0
        past the last word with a token."""
        n = int(n)
        if not 1 <= n <= capi.SALIENT_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.SALIENT_WORDS_MAX}]")
        ids, tot = np.zeros(n, np.int32), np.zeros(n, np.int64)
        sal, dist = np.zeros(n, np.float64), np.zeros(n, np.float64)
        _check(self._L.ldatm_salient_words(self._h, n, ids.ctypes.data, tot.ctypes.data, sal.ctypes.data,
                                           dist.ctypes.data), "salientWords")
        return ids, tot, sal, dist

    def getSalientWords(self, n: int = 30) -> list:
        """[(word, saliency), ...], at most n long, most salient first."""
        ids, _, sal, _ = self.salientWords(n)
        return [(self._word(w), float(x)) for w, x in zip(ids, sal) if w >= 0]

    def wordRows(self, ids):
        """ldatm_word_rows: (rows[M, K] int32, totals[M] int64) of the listed
        words (any order, duplicates allowed), gathered on the device."""
        w = np.ascontiguousarray(ids, np.int32).reshape(-1)
        if w.size and w.min() < 0:
            raise ValueError("word ids must not be negative")
        if w.size and self.alphabet is not None and w.max() >= self.alphabet.size():
            raise ValueError(f"word ids must be in [0, {self.alphabet.size()})")
        rows, tot = np.zeros((w.size, self.numTopics), np.int32), np.zeros(w.size, np.int64)
        if w.size:
            _check(self._L.ldatm_word_rows(self._h, w.size, w.ctypes.data, rows.ctypes.data, tot.ctypes.data),
                   "wordRows")
        return rows, tot

    def prepareVis(self, R: int = 30, lambdaStep: float = 0.01) -> dict:
        """The data of an LDAvis view as a dict in LDAvis's JSON layout
        (createJSON's keys: mdsDat, tinfo, token.table, R, lambda.step,
        plot.opts, topic.order), built from the device readouts: the R salient
        terms, per topic the union of its R most relevant terms under each
        lambda = 0, lambdaStep, ..., 1, the topics' token shares and a classical
        MDS of their Jensen-Shannon distances.  Topics are shown by nwsum
        descending (equal sums by ascending id); Freq of a topic's term is the
        exact count nw[w, k], Total the word's total.  Only the lists leave the
        device, never the V x K table."""
        R = int(R)
        if not 1 <= R <= capi.TOP_WORDS_MAX:
            raise ValueError(f"R must be in [1, {capi.TOP_WORDS_MAX}]")
        lam = vis_lambdas(lambdaStep)
        K = self.numTopics
        nwsum = np.zeros(K, np.int32)
        _check(self._L.ldatm_get_counts(self._h, None, nwsum.ctypes.data), "ldatm_get_counts")
        N = int(nwsum.astype(np.int64).sum())
        order = sorted(range(K), key=lambda k: (-int(nwsum[k]), k))
        rank = {k: i + 1 for i, k in enumerate(order)}
        x, y = classical_mds(self.topicDistances(None, "jensen_shannon"))
        sal_ids, sal_tot, _, _ = self.salientWords(R)
        terms = [[] for _ in range(K)]       # per topic (word, count, total, logprob, loglift), first seen
        seen = [set() for _ in range(K)]
        for l0 in range(0, lam.size, capi.RELEVANCE_LAMBDAS_MAX):
            r = self.relevantWords(R, lam[l0:l0 + capi.RELEVANCE_LAMBDAS_MAX])
            for l in range(r.lambdas.size):
                for k in range(K):
                    for i in range(R):
                        w = int(r.wordIds[l, k, i])
                        if w < 0:
                            break
                        if w not in seen[k]:
                            seen[k].add(w)
                            terms[k].append((w, int(r.counts[l, k, i]), int(r.totals[l, k, i]),
                                             float(r.logprob[l, k, i]), float(r.loglift[l, k, i])))
        name = lambda w: str(self._word(w))
        tinfo = {"Term": [], "Category": [], "Freq": [], "Total": [], "logprob": [], "loglift": []}

        def add(term, cat, freq, total, lp, ll):
            for key, v in zip(tinfo, (term, cat, freq, total, lp, ll)):
                tinfo[key].append(v)

        for i, (w, t) in enumerate(zip(sal_ids, sal_tot)):
            if w >= 0:
                add(name(w), "Default", int(t), int(t), float(R - i), float(R - i))
        for k in order:
            for w, c, t, lp, ll in terms[k]:
                add(name(w), "Topic%d" % rank[k], c, t, lp, ll)
        words = sorted({int(w) for w in sal_ids if w >= 0} | {w for k in range(K) for w in seen[k]})
        rows, tot = self.wordRows(words)
        table = {"Term": [], "Topic": [], "Freq": []}
        for j, w in enumerate(words):
            for k in order:
                if rows[j, k] >= 1:
                    table["Term"].append(name(w))
                    table["Topic"].append(rank[k])
                    table["Freq"].append(float(rows[j, k]) / float(tot[j]))
        return {
            "mdsDat": {"x": [float(x[k]) for k in order], "y": [float(y[k]) for k in order],
                       "topics": list(range(1, K + 1)), "cluster": [1] * K,
                       "Freq": [100.0 * float(nwsum[k]) / float(N) if N else 0.0 for k in order]},
            "tinfo": tinfo,
            "token.table": table,
            "R": R,
            "lambda.step": float(lambdaStep),
            "plot.opts": {"xlab": "PC1", "ylab": "PC2"},
            "topic.order": [k + 1 for k in order],
        }

    def saveVis(self, path, R: int = 30, lambdaStep: float = 0.01):
        """prepareVis(R, lambdaStep) written to `path` with json.dump."""
        import json
        vis = self.prepareVis(R, lambdaStep)
        with open(path, "w") as f:
            json.dump(vis, f)

    # ------------------------------- topic phrases
    def topicPhrases(self, n: int, minLength: int = 2, maxLength: int = 32, minCount: int = 1):
        """ldatm_topic_phrases: per topic the n most frequent same-topic token
        runs with minLength <= length <= maxLength and count >= minCount, by
        count descending, then word ids ascending, a prefix before its
        extension, counted on the device.  Returns (words[K, n, maxLength]
        int32 (-1 padded), lengths[K, n] int32, counts[K, n] int64, first[K, n]
        int64 global token index, runs[K] int64, distinct[K] int64 (-1 with
        several shards), skippedLong int, proven[K] int32)."""
        n, minLength, maxLength = int(n), int(minLength), int(maxLength)
        if not 1 <= n <= capi.PHRASES_MAX:
            raise ValueError(f"n must be in [1, {capi.PHRASES_MAX}]")
        if not 2 <= minLength <= maxLength <= capi.PHRASE_LEN_MAX:
            raise ValueError(f"the lengths must satisfy 2 <= minLength <= maxLength <= {capi.PHRASE_LEN_MAX}")
        K = self.numTopics
        words = np.zeros((K, n, maxLength), np.int32)
        lens = np.zeros((K, n), np.int32)
        cnt = np.zeros((K, n), np.int64)
        first = np.zeros((K, n), np.int64)
        runs = np.zeros(K, np.int64)
        distinct = np.zeros(K, np.int64)
        proven = np.zeros(K, np.int32)
        skipped = C.c_int64()
        _check(self._L.ldatm_topic_phrases(self._h, n, minLength, maxLength, int(minCount), words.ctypes.data,
                                           lens.ctypes.data, cnt.ctypes.data, first.ctypes.data, runs.ctypes.data,
                                           distinct.ctypes.data, C.addressof(skipped), proven.ctypes.data),
               "topicPhrases")
        return words, lens, cnt, first, runs, distinct, int(skipped.value), proven

    def getTopicPhrases(self, n: int = 10, minLength: int = 2, maxLength: int = 32, minCount: int = 1) -> TopicPhrases:
        words, lens, cnt, first, runs, distinct, skipped, proven = self.topicPhrases(n, minLength, maxLength, minCount)
        name = str if self.alphabet is None else (lambda w: str(self.alphabet.lookupObject(w)))
        ids = [[tuple(int(w) for w in words[k, i, :lens[k, i]]) for i in range(words.shape[1]) if lens[k, i] > 0]
               for k in range(self.numTopics)]
        phrases = [[(" ".join(name(w) for w in p), int(cnt[k, i])) for i, p in enumerate(ids[k])]
                   for k in range(self.numTopics)]
        return TopicPhrases(phrases, ids, cnt, first, runs, distinct, skipped, proven)

    # ------------------------------- topic co-occurrence in documents
    def topicCooccurrence(self, stats=capi.TOPIC_COOC_STATS, minTokens: int = 10, minCount: int = 2,
                          minProp: float = 0.05) -> dict:
        """ldatm_topic_cooccurrence: which topics share documents, counted on
        the device from z and summed over the shards.  A document is used with
        at least minTokens tokens; topic k is present in it with n_dk >=
        minCount and n_dk >= minProp * L_d (jsLDA's defaults).  Returns a dict:
        "docs_used" (int), "tokens" [K] and "present" [K] (int64), and of
        "codocs" / "overlap" / "product" ([K, K] int64: documents with both
        present, sum of min(n_dk, n_dl), sum of n_dk n_dl) those named in
        stats; only they are counted."""
        stats = capi.topic_cooc_stats(stats)
        thr = capi.topic_cooc_thresholds(minTokens, minCount, minProp)
        K = self.numTopics
        used = C.c_int64()
        out = {"tokens": np.zeros(K, np.int64), "present": np.zeros(K, np.int64)}
        for s in stats:
            out[s] = np.zeros((K, K), np.int64)
        tabs = [out[s].ctypes.data if s in out else None for s in capi.TOPIC_COOC_STATS]
        _check(self._L.ldatm_topic_cooccurrence(self._h, *thr, C.byref(used), out["tokens"].ctypes.data,
                                                out["present"].ctypes.data, *tabs), "topicCooccurrence")
        out["docs_used"] = int(used.value)
        return out

    def topicCorrelations(self, measure="npmi", minTokens: int = 10, minCount: int = 2,
                          minProp: float = 0.05) -> np.ndarray:
        """ldatm_topic_correlations: the float64 [K, K] matrix of a measure of
        co-occurrence in documents -- "pmi", "npmi", "jaccard" (documents with
        both topics present), "overlap" (shared tokens), "cosine", "pearson"
        (of the documents' topic counts) -- counting only the table it needs."""
        m = CORR_MEASURES[correlation_measure(measure)]
        thr = capi.topic_cooc_thresholds(minTokens, minCount, minProp)
        out = np.zeros((self.numTopics, self.numTopics), np.float64)
        _check(self._L.ldatm_topic_correlations(self._h, m, *thr, out.ctypes.data), "topicCorrelations")
        return out

    def topicPartners(self, n: int = 5, measure="npmi", minTokens: int = 10, minCount: int = 2,
                      minProp: float = 0.05):
        """ldatm_topic_partners: per topic its n strongest other topics by
        topicCorrelations(measure): (ids int32 [K, n], values float64 [K, n]),
        larger value first, equal values by smaller id, non-finite values left
        out, -1 / NaN past the last."""
        n = int(n)
        if n < 1:
            raise ValueError("n must be at least 1")
        m = CORR_MEASURES[correlation_measure(measure)]
        thr = capi.topic_cooc_thresholds(minTokens, minCount, minProp)
        ids = np.zeros((self.numTopics, n), np.int32)
        values = np.zeros((self.numTopics, n), np.float64)
        _check(self._L.ldatm_topic_partners(self._h, m, *thr, n, ids.ctypes.data, values.ctypes.data),
               "topicPartners")
        return ids, values

    def getTopicPartners(self, n: int = 5, measure="npmi", minTokens: int = 10, minCount: int = 2,
                         minProp: float = 0.05) -> list:
        """Per topic a list of (topic, value), at most n long, strongest first."""
        ids, values = self.topicPartners(n, measure, minTokens, minCount, minProp)
        return [[(int(t), float(v)) for t, v in zip(ids[k], values[k]) if t >= 0] for k in range(self.numTopics)]

    def topicGraph(self, measure="npmi", cutoff: float = 0.0, minTokens: int = 10, minCount: int = 2,
                   minProp: float = 0.05) -> list:
        """The edges (k, l, value), k < l, whose topicCorrelations(measure)
        value is at least cutoff (a NaN never is), by ascending (k, l)."""
        mat = self.topicCorrelations(measure, minTokens, minCount, minProp)
        cutoff = float(cutoff)
        with np.errstate(invalid="ignore"):
            k, l = np.nonzero(np.triu(mat >= cutoff, 1))
        return [(int(a), int(b), float(mat[a, b])) for a, b in zip(k, l)]

    # ------------------------------- topics by document group
    def _groups(self, groups):
        """(labels, ids int32 [D]) of one label per document; None takes each
        instance's target.  A document whose label is None is left out."""
        if groups is None:
            groups = [i.target for i in self.data]
        labels, ids = group_labels(groups)
        if len(ids) != len(self.data):
            raise ValueError(f"groups must hold one label per document ({len(self.data)})")
        if not labels:
            raise ValueError("no groups: every label is None")
        return labels, ids

    def groupTopics(self, doc_group, G=None, stats=capi.GROUP_TOPICS_STATS, minTokens: int = 10, minCount: int = 2,
                    minProp: float = 0.05) -> dict:
        """ldatm_group_topics: GibbsSampler.group_topics over the whole model,
        summed over the shards; doc_group holds one id in [-1, G) per document
        in the model's order."""
        stats = capi.group_topics_stats(stats)
        thr = capi.topic_cooc_thresholds(minTokens, minCount, minProp)
        ids, G = capi.group_ids(doc_group, len(self.data), G)
        K = self.numTopics
        out = {"group_docs": np.zeros(G, np.int64), "group_tokens": np.zeros(G, np.int64),
               "tokens": np.zeros((G, K), np.int64)}
        for s in stats:
            out[s] = np.zeros((G, K), np.uint64 if s == "shares" else np.int64)
        tabs = [out[s].ctypes.data if s in out else None for s in capi.GROUP_TOPICS_STATS]
        _check(self._L.ldatm_group_topics(self._h, ids.ctypes.data, G, *thr, out["group_docs"].ctypes.data,
                                          out["group_tokens"].ctypes.data, out["tokens"].ctypes.data, *tabs),
               "groupTopics")
        return out

    def topicsByGroup(self, groups=None, kind="mean", stats=None, minTokens: int = 10, minCount: int = 2,
                      minProp: float = 0.05) -> TopicsByGroup:
        """How much of each group of documents is each topic.  groups holds
        one label per document (None leaves a document out); groups = None
        takes each instance's target.  The sorted distinct labels are the rows.
        kind: "mean" (the mean over the group's documents of the topic's
        proportion, what jsLDA plots over time), "tokens" (the topic's share
        of the group's tokens), "documents" (the share of the group's documents
        in which the topic is present), "lift" (log of the token share over the
        topic's share of all groups).  A document counts with at least
        minTokens tokens; a topic is present with n_dk >= minCount and n_dk >=
        minProp * L_d.  Counted on the GPU from z; stats names further integer
        tables to count beside the kind's own."""
        kind = group_kind(kind)
        need = GROUP_KIND_TABLE[kind]
        stats = capi.group_topics_stats(() if stats is None else stats)
        if need is not None and need not in stats:
            stats = capi.group_topics_stats(stats + (need,))
        labels, ids = self._groups(groups)
        c = self.groupTopics(ids, len(labels), stats, minTokens, minCount, minProp)
        values = group_prevalence_finish(kind, c["group_docs"], c["group_tokens"], c["tokens"], c.get("present"),
                                         c.get("shares"))
        return TopicsByGroup(kind, labels, values, c.pop("group_docs"), c.pop("group_tokens"), c)

    def getGroupTopTopics(self, n: int = 5, groups=None, kind="mean", minTokens: int = 10, minCount: int = 2,
                          minProp: float = 0.05) -> dict:
        """Per label a list of (topic, value), at most n long, largest first
        (equal values by smaller topic, non-finite values left out)."""
        n = int(n)
        if n < 1:
            raise ValueError("n must be at least 1")
        r = self.topicsByGroup(groups, kind, None, minTokens, minCount, minProp)
        ids, values = group_top_topics_select(r.values, n)
        return {label: [(int(t), float(v)) for t, v in zip(ids[g], values[g]) if t >= 0]
                for g, label in enumerate(r.labels)}

    def subCorpusTopWords(self, mask, n: int):
        """ldatm_subcorpus_top_words: (word_ids[K, n], counts[K, n]) int32 and
        totals[K] int64 -- topWords' selection inside the documents whose mask
        entry is nonzero, counted on the GPU from z and added over the shards
        before selecting."""
        n = int(n)
        if not 1 <= n <= capi.TOP_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOP_WORDS_MAX}]")
        m = capi.doc_mask(mask, len(self.data))
        ids = np.zeros((self.numTopics, n), np.int32)
        cnt = np.zeros((self.numTopics, n), np.int32)
        tot = np.zeros(self.numTopics, np.int64)
        _check(self._L.ldatm_subcorpus_top_words(self._h, m.ctypes.data if len(m) else None, n, ids.ctypes.data,
                                                 cnt.ctypes.data, tot.ctypes.data), "subCorpusTopWords")
        return ids, cnt, tot

    def getSubCorpusTopWords(self, mask, n: int) -> list:
        """Per topic a list of (word, count), at most n long, heaviest first,
        inside the documents whose mask entry is nonzero."""
        ids, cnt, _ = self.subCorpusTopWords(mask, n)
        name = (lambda w: w) if self.alphabet is None else self.alphabet.lookupObject
        return [[(name(int(w)), int(c)) for w, c in zip(ids[k], cnt[k]) if w >= 0]
                for k in range(self.numTopics)]

    def getGroupTopWords(self, label, n: int, groups=None) -> list:
        """getSubCorpusTopWords over the documents whose label (groups, or the
        instances' targets) equals label."""
        labels, ids = self._groups(groups)
        if label not in labels:
            raise ValueError(f"unknown label {label!r}")
        return self.getSubCorpusTopWords(ids == labels.index(label), n)

    # ------------------------------- topic distances
    def _other_model(self, other):
        """(native handle or None, K2) of the other side of a topic
        comparison, checked before any native call."""
        if other is None or other is self:
            return None, self.numTopics
        if not isinstance(other, ParallelTopicModel):
            raise ValueError(f"other must be a ParallelTopicModel or None, not {type(other).__name__}")
        mine = None if self.alphabet is None else self.alphabet.toArray()
        theirs = None if other.alphabet is None else other.alphabet.toArray()
        if mine != theirs:
            raise ValueError("the two models' alphabets differ: word ids must mean the same words in both")
        return other._h, other.numTopics

    def topicDistances(self, other=None, metric="jensen_shannon") -> np.ndarray:
        """ldatm_topic_distances: the float64 (K, K2) matrix of a distance
        between this model's smoothed topics (rows) and `other`'s (columns;
        None: this model), computed on the device from the global counts.
        metric: "cosine" (a similarity), "hellinger", "jensen_shannon" (nats),
        "kullback_leibler" (KL(row || column)), or the LDA_TOPIC_* integer.
        `other`'s alphabet must equal this model's -- word ids must mean the
        same words; aligning two vocabularies is the caller's job."""
        m = capi.topic_metric(metric)
        oh, K2 = self._other_model(other)
        out = np.zeros((self.numTopics, K2), np.float64)
        _check(self._L.ldatm_topic_distances(self._h, oh, m, out.ctypes.data), "topicDistances")
        return out

    def nearestTopics(self, n: int, other=None, metric="jensen_shannon"):
        """ldatm_nearest_topics: per topic the n nearest topics of `other`
        (None: this model, the topic itself left out), selected on the device:
        value ascending (cosine: descending), ties by ascending topic id.
        Returns (topics int32 (K, n), values float64 (K, n)); -1 / NaN past the
        last candidate.  `other` as topicDistances takes it."""
        n = capi.topic_nearest_n(n)
        m = capi.topic_metric(metric)
        oh, _ = self._other_model(other)
        topics = np.zeros((self.numTopics, n), np.int32)
        values = np.zeros((self.numTopics, n), np.float64)
        _check(self._L.ldatm_nearest_topics(self._h, oh, m, n, topics.ctypes.data, values.ctypes.data),
               "nearestTopics")
        return topics, values

    # ------------------------------- topic diagnostics
    def topicCodocuments(self, word_ids, props=()):
        """ldatm_topic_codocuments: every shard's lda_topic_codocuments with
        the lists word_ids[K, n] (-1 = empty slot), summed: (codoc[K, n (n + 1)
        / 2] int64, doc_stats[K, 2 + P] int64)."""
        ids = np.ascontiguousarray(word_ids, dtype=np.int32)
        if ids.ndim != 2 or ids.shape[0] != self.numTopics:
            raise ValueError("word_ids must be [K, n]")
        n = ids.shape[1]
        if not 1 <= n <= capi.DIAG_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.DIAG_WORDS_MAX}]")
        p = np.ascontiguousarray(props, dtype=np.float64).reshape(-1)
        if len(p) > capi.DIAG_PROPS_MAX:
            raise ValueError(f"at most {capi.DIAG_PROPS_MAX} props")
        codoc = np.zeros((self.numTopics, n * (n + 1) // 2), np.int64)
        stats = np.zeros((self.numTopics, 2 + len(p)), np.int64)
        _check(self._L.ldatm_topic_codocuments(self._h, n, ids.ctypes.data, len(p), p.ctypes.data if len(p) else None,
                                               codoc.ctypes.data, stats.ctypes.data), "topicCodocuments")
        return codoc, stats

    def topicStatistics(self, numTopWords: int = 20) -> dict:
        """ldatm_topic_statistics: the integer statistics behind the
        diagnostics for each topic's numTopWords top words, as a dict of
        word_ids, counts, totals, share_sums [K, n], sumsq [K], codoc
        [K, n (n + 1) / 2] and doc_stats [K, 9]."""
        n = int(numTopWords)
        if not 1 <= n <= capi.DIAG_WORDS_MAX:
            raise ValueError(f"numTopWords must be in [1, {capi.DIAG_WORDS_MAX}]")
        K = self.numTopics
        s = {"word_ids": np.zeros((K, n), np.int32), "counts": np.zeros((K, n), np.int32),
             "totals": np.zeros((K, n), np.int64), "share_sums": np.zeros((K, n), np.float64),
             "sumsq": np.zeros(K, np.uint64), "codoc": np.zeros((K, n * (n + 1) // 2), np.int64),
             "doc_stats": np.zeros((K, 2 + len(DIAG_PROPS)), np.int64)}
        _check(self._L.ldatm_topic_statistics(self._h, n, *(a.ctypes.data for a in s.values())), "topicStatistics")
        return s

    def getDiagnostics(self, numTopWords: int = 20) -> "TopicDiagnostics":
        """Per-topic diagnostics after Mallet's TopicModelDiagnostics, counted on
        the device (ldatm_topic_diagnostics): a TopicDiagnostics with one array
        [K] per column of DIAG_COLUMNS."""
        n = int(numTopWords)
        if not 1 <= n <= capi.DIAG_WORDS_MAX:
            raise ValueError(f"numTopWords must be in [1, {capi.DIAG_WORDS_MAX}]")
        K = self.numTopics
        out = np.zeros((K, len(DIAG_COLUMNS)), np.float64)
        ids = np.zeros((K, n), np.int32)
        _check(self._L.ldatm_topic_diagnostics(self._h, n, out.ctypes.data, ids.ctypes.data), "getDiagnostics")
        # the triangles themselves, for the same lists (one more document pass)
        return TopicDiagnostics(self, out, ids, self.topicCodocuments(ids)[0])

    # ------------------------------- reference-corpus coherence
    def _reference(self, reference):
        """(Dh, doc_off or None, words or None) of a coherence corpus: None is
        the training corpus; an InstanceList goes up from the host, its tokens
        outside the model's alphabet as -1."""
        if reference is None:
            return 0, None, None
        if not isinstance(reference, InstanceList):
            raise ValueError(f"reference must be an InstanceList or None, not {type(reference).__name__}")
        off, w = _flatten(list(reference))
        V = self._shape()[1]
        if self.alphabet is not None and reference.alphabet is not self.alphabet:
            # the reference's ids mean its own alphabet's words
            to = np.array([self.alphabet.lookupIndex(e, False) for e in reference.alphabet.toArray()] + [-1], np.int32)
            w = to[np.where((w >= 0) & (w < len(to) - 1), w, len(to) - 1)]
        w = np.ascontiguousarray(np.where((w >= 0) & (w < V), w, -1), np.int32)
        return len(off) - 1, off, w

    def wordCooccurrences(self, word_ids, window: int = 0, reference=None):
        """ldatm_word_cooccurrences: units of a corpus (window 0: its non-empty
        documents; W >= 1: its windows of W tokens) that hold two words of a
        topic's list word_ids[K, n] (-1 = empty slot), whatever the tokens'
        topics, counted on the device.  reference None: the training corpus
        (every shard's documents, summed); else an InstanceList.  Returns
        (cooc[K, n (n + 1) / 2] int64, units)."""
        ids = np.ascontiguousarray(word_ids, dtype=np.int32)
        if ids.ndim != 2 or ids.shape[0] != self.numTopics:
            raise ValueError("word_ids must be [K, n]")
        n = ids.shape[1]
        if not 1 <= n <= capi.DIAG_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.DIAG_WORDS_MAX}]")
        if not 0 <= int(window) <= capi.COOC_WINDOW_MAX:
            raise ValueError(f"window must be in [0, {capi.COOC_WINDOW_MAX}]")
        Dh, off, w = self._reference(reference)
        cooc = np.zeros((self.numTopics, n * (n + 1) // 2), np.int64)
        units = C.c_int64(0)
        _check(self._L.ldatm_word_cooccurrences(self._h, n, ids.ctypes.data, int(window), Dh,
                                                off.ctypes.data if off is not None else None,
                                                w.ctypes.data if w is not None and len(w) else None,
                                                cooc.ctypes.data, C.addressof(units)), "wordCooccurrences")
        return cooc, int(units.value)

    def getCoherence(self, measure: str = "c_npmi", numTopWords: int = 10, window=None, reference=None,
                     epsilon=None) -> "TopicCoherence":
        """Coherence of each topic's numTopWords top words by co-occurrence in
        a corpus (ldatm_topic_coherence): measure "u_mass" (Mimno 2011),
        "c_uci" (Newman 2010) or "c_npmi" (Lau 2014).  window None: the
        measure's customary units, documents (0) for u_mass and windows of 10
        tokens for c_uci / c_npmi.  reference None: the training corpus; else
        an InstanceList (tokens outside the model's alphabet match nothing).
        epsilon None: 1 for u_mass, 1e-12 otherwise."""
        if measure not in COHERENCE_MEASURES:
            raise ValueError(f"measure must be one of {sorted(COHERENCE_MEASURES)}, not {measure!r}")
        n = int(numTopWords)
        if not 1 <= n <= capi.DIAG_WORDS_MAX:
            raise ValueError(f"numTopWords must be in [1, {capi.DIAG_WORDS_MAX}]")
        window = (0 if measure == "u_mass" else 10) if window is None else int(window)
        if not 0 <= window <= capi.COOC_WINDOW_MAX:
            raise ValueError(f"window must be in [0, {capi.COOC_WINDOW_MAX}]")
        eps = -1.0 if epsilon is None else float(epsilon)
        if epsilon is not None and not eps >= 0.0:
            raise ValueError("epsilon must be >= 0")
        Dh, off, w = self._reference(reference)
        K = self.numTopics
        values, pairs = np.zeros(K, np.float64), np.zeros(K, np.int64)
        ids, cooc = np.zeros((K, n), np.int32), np.zeros((K, n * (n + 1) // 2), np.int64)
        units = C.c_int64(0)
        _check(self._L.ldatm_topic_coherence(self._h, COHERENCE_MEASURES[measure], n, window, eps, Dh,
                                             off.ctypes.data if off is not None else None,
                                             w.ctypes.data if w is not None and len(w) else None,
                                             values.ctypes.data, pairs.ctypes.data, ids.ctypes.data, cooc.ctypes.data,
                                             C.addressof(units)), "getCoherence")
        return TopicCoherence(self, measure, window, epsilon, values, pairs, ids, cooc, int(units.value))

    def topTopics(self, docs=None, n: int = 10):
        """The n heaviest topics of the documents `docs` (global ids; None =
        all): (topics[M, n] int32, weights[M, n] fp64), weights
        (alpha_k + n_dk) / (n_d + alphaSum) as printDocumentTopics prints them;
        past K: topic -1, weight NaN."""
        topics, cnt = self.docTopTopics(n, docs)
        ids, M = _doc_ids(docs, self)
        if len(self.data) == self._shape()[2]:
            lens = np.array([len(i.data) for i in self.data], np.int64)
            lens = lens if ids is None else lens[ids]
        else:       # a loaded model holds no instances here: the rows' sums
            lens = self.docCounts(docs).sum(axis=1, dtype=np.int64)
        alpha = self.alpha
        w = (alpha[np.maximum(topics, 0)] + cnt) / (lens.astype(np.float64) + self.alphaSum)[:, None]
        return topics, np.where(topics >= 0, w, np.nan)

    # ---------------------------------------------------------- outputs
    def _text(self, fn, *args) -> str:
        n = C.c_size_t()
        _check(fn(self._h, *args, None, 0, C.byref(n)), fn.__name__)
        buf = C.create_string_buffer(n.value + 1)
        _check(fn(self._h, *args, buf, n.value + 1, C.byref(n)), fn.__name__)
        return buf.value.decode()

    def documentTopics(self, threshold: float = 0.0, max: int = -1) -> str:
        return self._text(self._L.ldatm_document_topics_text, float(threshold), int(max))

    def printDocumentTopics(self, path, threshold: float = 0.0, max: int = -1):
        _check(self._L.ldatm_print_document_topics(self._h, os.fsencode(path), float(threshold),
                                                   int(max)), "printDocumentTopics")

    def displayTopWords(self, numWords: int, usingNewLines: bool = False) -> str:
        return self._text(self._L.ldatm_top_words_text, int(numWords), int(bool(usingNewLines)))

    def printTopWords(self, path, numWords: int, usingNewLines: bool = False):
        _check(self._L.ldatm_print_top_words(self._h, os.fsencode(path), int(numWords),
                                             int(bool(usingNewLines))), "printTopWords")

    def topicDocumentsText(self, max: int = 100, smoothing: float = 10.0, minTokens: int = 1) -> str:
        """printTopicDocuments' text: "#topic doc name proportion ...", then
        per topic and rank "topic doc name weight"."""
        return self._text(self._L.ldatm_topic_documents_text, int(max), float(smoothing), int(minTokens))

    def printTopicDocuments(self, path, max: int = 100, smoothing: float = 10.0, minTokens: int = 1):
        _check(self._L.ldatm_print_topic_documents(self._h, os.fsencode(path), int(max), float(smoothing),
                                                   int(minTokens)), "printTopicDocuments")

    def relevantWordsText(self, n: int = 10, lambda_: float = 0.6) -> str:
        """printRelevantWords' text: "#topic rank word count total relevance
        logprob loglift", then one such line per topic and rank."""
        n, lam = self._relevance_args(n, lambda_)
        return self._text(self._L.ldatm_relevant_words_text, n, lam)

    def printRelevantWords(self, path, n: int = 10, lambda_: float = 0.6):
        n, lam = self._relevance_args(n, lambda_)
        _check(self._L.ldatm_print_relevant_words(self._h, os.fsencode(path), n, lam), "printRelevantWords")

    @staticmethod
    def _relevance_args(n, lambda_):
        n = int(n)
        if not 1 <= n <= capi.TOP_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOP_WORDS_MAX}]")
        if np.ndim(lambda_) != 0:
            raise ValueError("lambda_ must be one value")
        return n, float(capi.check_lambdas(lambda_)[0])

    def topicPhrasesText(self, n: int = 10, minLength: int = 2, maxLength: int = 32, minCount: int = 1) -> str:
        """printTopicPhrases' text: "#topic rank count phrase", then per topic
        and rank "topic rank count word word ..."."""
        return self._text(self._L.ldatm_topic_phrases_text, int(n), int(minLength), int(maxLength), int(minCount))

    def printTopicPhrases(self, path, n: int = 10, minLength: int = 2, maxLength: int = 32, minCount: int = 1):
        _check(self._L.ldatm_print_topic_phrases(self._h, os.fsencode(path), int(n), int(minLength), int(maxLength),
                                                 int(minCount)), "printTopicPhrases")

    def topicCorrelationsText(self, n: int = 5, measure="npmi", minTokens: int = 10, minCount: int = 2,
                              minProp: float = 0.05) -> str:
        """printTopicCorrelations' text: "#topic partner value", then per topic
        and rank "topic partner value"."""
        n = int(n)
        if n < 1:
            raise ValueError("n must be at least 1")
        m = CORR_MEASURES[correlation_measure(measure)]
        thr = capi.topic_cooc_thresholds(minTokens, minCount, minProp)
        return self._text(self._L.ldatm_topic_correlations_text, m, n, *thr)

    def printTopicCorrelations(self, path, n: int = 5, measure="npmi", minTokens: int = 10, minCount: int = 2,
                               minProp: float = 0.05):
        n = int(n)
        if n < 1:
            raise ValueError("n must be at least 1")
        m = CORR_MEASURES[correlation_measure(measure)]
        thr = capi.topic_cooc_thresholds(minTokens, minCount, minProp)
        _check(self._L.ldatm_print_topic_correlations(self._h, os.fsencode(path), m, n, *thr),
               "printTopicCorrelations")

    def groupTopicsText(self, n: int = 5, kind="mean", groups=None, minTokens: int = 10, minCount: int = 2,
                        minProp: float = 0.05) -> str:
        """printGroupTopics' text: "#group topic value", then per group and
        rank "group topic value"; a group is the index of its label among the
        sorted distinct labels (topicsByGroup(...).labels)."""
        n = int(n)
        if n < 1:
            raise ValueError("n must be at least 1")
        k = GROUP_KINDS[group_kind(kind)]
        thr = capi.topic_cooc_thresholds(minTokens, minCount, minProp)
        labels, ids = self._groups(groups)
        return self._text(self._L.ldatm_group_topics_text, ids.ctypes.data, len(labels), k, n, *thr)

    def printGroupTopics(self, path, n: int = 5, kind="mean", groups=None, minTokens: int = 10, minCount: int = 2,
                         minProp: float = 0.05):
        n = int(n)
        if n < 1:
            raise ValueError("n must be at least 1")
        k = GROUP_KINDS[group_kind(kind)]
        thr = capi.topic_cooc_thresholds(minTokens, minCount, minProp)
        labels, ids = self._groups(groups)
        _check(self._L.ldatm_print_group_topics(self._h, os.fsencode(path), ids.ctypes.data, len(labels), k, n, *thr),
               "printGroupTopics")

    # ------------------------------------------------ checkpoint / resume
    def save(self, path):
        """Everything needed to continue this run bit for bit."""
        _check(self._L.ldatm_save(self._h, os.fsencode(path)), "ldatm_save")

    @classmethod
    def load(cls, path) -> "ParallelTopicModel":
        L = load_tm()
        h = C.c_void_p()
        _check(L.ldatm_load(C.byref(h), os.fsencode(path)), "ldatm_load")
        m = cls.__new__(cls)
        m._h, m._L = h, L
        m.numTopics = m._shape()[0]
        m.alphabet = None
        m.data = []
        return m

    # -------------------------------------------------------- inference
    def getInferencer(self) -> "TopicInferencer":
        return TopicInferencer(self)

    # ------------------------------------------------ prediction scoring
    def scoreDistributions(self, theta, docs=None, metric="cosine") -> np.ndarray:
        """Similarity ("cosine" or "mse") of the rows of theta[Q, K] to
        getTopicProbabilities(d) of the training documents `docs` (global ids,
        any order; None = all), computed on the device: scores[Q, M]."""
        theta = capi.as_theta(theta, self.numTopics)
        m = capi.score_metric(metric)
        ids, M = _doc_ids(docs, self)
        scores = np.zeros((len(theta), M), np.float64)
        _check(self._L.ldatm_score_theta(self._h, m, len(theta), theta.ctypes.data, M,
                                         ids.ctypes.data if ids is not None and M else None,
                                         scores.ctypes.data), "scoreDistributions")
        return scores

    def topDocuments(self, theta, n: int, metric="cosine"):
        """The n best training documents per row of theta[Q, K]: (doc_ids[Q, n],
        scores[Q, n]), best first (largest cosine / smallest mse, ties by
        ascending id); past the number of documents: id -1, score NaN."""
        theta = capi.as_theta(theta, self.numTopics)
        m = capi.score_metric(metric)
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        ids = np.full((len(theta), n), -1, np.int64)
        scores = np.full((len(theta), n), np.nan, np.float64)
        _check(self._L.ldatm_score_top(self._h, m, len(theta), theta.ctypes.data, n, ids.ctypes.data,
                                       scores.ctypes.data), "topDocuments")
        return ids, scores

    # ------------------------------------------ nearest documents
    def documentDistances(self, theta=None, counts=None, docs=None, metric="hellinger") -> np.ndarray:
        """ldatm_document_distances: the float64 (Q, M) matrix of a metric
        ("cosine", "hellinger", "jensen_shannon" or the integer) between query
        rows -- theta[Q, K] as given, or counts[Q, K] smoothed with the model's
        alpha on the device; exactly one -- and the training documents `docs`
        (global ids, any order; None = all), computed on the device."""
        m = capi.doc_metric(metric)
        theta, counts = capi.doc_queries(theta, counts, self.numTopics)
        q = theta if theta is not None else counts
        ids, M = _doc_ids(docs, self)
        out = np.zeros((len(q), M), np.float64)
        _check(self._L.ldatm_document_distances(self._h, m, len(q), theta.ctypes.data if theta is not None else None,
                                                counts.ctypes.data if counts is not None else None, M,
                                                ids.ctypes.data if ids is not None and M else None,
                                                out.ctypes.data), "documentDistances")
        return out

    def nearestDocuments(self, theta=None, n: int = 10, metric="hellinger", minTokens: int = 1, counts=None,
                         skip=None):
        """ldatm_nearest_documents: per query row (theta or counts, as
        documentDistances takes them) the n nearest training documents with at
        least minTokens tokens, selected on the device: value ascending
        (cosine: descending), ties by ascending id; skip[Q] names a document
        each query leaves out (-1: none).  Returns (docs int64 (Q, n), values
        float64 (Q, n)); -1 / NaN past the last candidate."""
        n = capi.doc_nearest_n(n)
        m = capi.doc_metric(metric)
        theta, counts = capi.doc_queries(theta, counts, self.numTopics)
        q = theta if theta is not None else counts
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, dtype=np.int64).reshape(-1)
            if len(sk) != len(q):
                raise ValueError(f"skip must hold one id per query ({len(q)}), not {len(sk)}")
        ids = np.zeros((len(q), n), np.int64)
        values = np.zeros((len(q), n), np.float64)
        _check(self._L.ldatm_nearest_documents(self._h, m, n, len(q), theta.ctypes.data if theta is not None else None,
                                               counts.ctypes.data if counts is not None else None,
                                               sk.ctypes.data if sk is not None and len(sk) else None, int(minTokens),
                                               ids.ctypes.data, values.ctypes.data), "nearestDocuments")
        return ids, values

    def documentNeighbors(self, n: int = 10, docs=None, metric="hellinger", minTokens: int = 1):
        """ldatm_document_neighbors: per training document of `docs` (global
        ids; None = all) its n nearest other documents with at least minTokens
        tokens, rows built and neighbours selected on the device.  Returns
        (ids int64 (M, n), values float64 (M, n)); -1 / NaN past the last
        candidate."""
        n = capi.doc_nearest_n(n)
        m = capi.doc_metric(metric)
        q, M = _doc_ids(docs, self)
        ids = np.zeros((M, n), np.int64)
        values = np.zeros((M, n), np.float64)
        _check(self._L.ldatm_document_neighbors(self._h, m, n, M, q.ctypes.data if q is not None and M else None,
                                                int(minTokens), ids.ctypes.data, values.ctypes.data),
               "documentNeighbors")
        return ids, values

    def getDocumentNeighbors(self, doc: int, n: int = 10, metric="hellinger", minTokens: int = 1) -> list:
        """The neighbours of one document as [(doc id, name, value), ...],
        nearest first; name is the instance's name (None without one)."""
        ids, values = self.documentNeighbors(n, [int(doc)], metric, minTokens)
        name = lambda d: self.data[d].name if d < len(self.data) else None
        return [(int(d), name(int(d)), float(v)) for d, v in zip(ids[0], values[0]) if d >= 0]

    def documentNeighborsText(self, n: int = 10, metric="hellinger", minTokens: int = 1) -> str:
        """printDocumentNeighbors' text: "#doc neighbor name value", then per
        document and rank "doc neighbor name value"."""
        n, m = capi.doc_nearest_n(n), capi.doc_metric(metric)
        return self._text(self._L.ldatm_document_neighbors_text, n, m, int(minTokens))

    def printDocumentNeighbors(self, path, n: int = 10, metric="hellinger", minTokens: int = 1):
        n, m = capi.doc_nearest_n(n), capi.doc_metric(metric)
        _check(self._L.ldatm_print_document_neighbors(self._h, os.fsencode(path), n, m, int(minTokens)),
               "printDocumentNeighbors")

    # ------------------------------------------------ held-out evaluation
    def getHeldOutEvaluator(self) -> "HeldOutEvaluator":
        return HeldOutEvaluator(self)

    def getProbEstimator(self) -> "MarginalProbEstimator":
        return MarginalProbEstimator(self)

    def heldOutLogLikelihood(self, theta, doc_off, words):
        """ldatm_heldout_loglik: (doc_ll[Dh], total) of the scored tokens
        (doc_off[Dh + 1], words, ids in [0, V)) under theta[Dh, K] and the
        model's current counts, computed on the device."""
        theta = capi.as_theta(theta, self.numTopics)
        off, w = capi.as_docs(doc_off, words, len(theta))
        doc_ll = np.zeros(len(theta), np.float64)
        total = C.c_double(0.0)
        _check(self._L.ldatm_heldout_loglik(self._h, len(theta), theta.ctypes.data, off.ctypes.data,
                                            w.ctypes.data if len(w) else None, doc_ll.ctypes.data,
                                            C.addressof(total)), "heldOutLogLikelihood")
        return doc_ll, total.value

    def setHeldOut(self, instances, interval: int, numIterations: int = 100, thinning: int = 10,
                   burnIn: int = 10, seed: int = 0):
        """estimate() evaluates `instances` as getHeldOutEvaluator().evaluate
        does after every sweep it with it % interval == 0 (0 = off) and keeps
        (it, held-out LL/token) in heldOutTrace().  Training is unchanged."""
        interval = int(interval)
        if interval < 0:
            raise ValueError("interval must be >= 0")
        off, w = _flatten(list(instances))
        _check(self._L.ldatm_set_held_out(self._h, len(off) - 1, off.ctypes.data, w.ctypes.data if len(w) else None,
                                          interval, int(numIterations), int(thinning), int(burnIn),
                                          int(seed) & (2**64 - 1)), "setHeldOut")

    def heldOutTrace(self):
        """[(iteration, held-out LL/token)] of the last estimate()."""
        n = C.c_int32()
        _check(self._L.ldatm_get_held_out_trace(self._h, None, None, 0, C.byref(n)), "ldatm_get_held_out_trace")
        it = np.zeros(n.value, np.int32)
        ll = np.zeros(n.value, np.float64)
        if n.value:
            _check(self._L.ldatm_get_held_out_trace(self._h, it.ctypes.data, ll.ctypes.data, n.value,
                                                    C.byref(n)), "ldatm_get_held_out_trace")
        return list(zip(it.tolist(), ll.tolist()))


# LDATM_DIAG_* of lda_topic_model.h: the columns in order, Mallet's proportions
DIAG_COLUMNS = ("tokens", "document_entropy", "coherence", "uniform_dist", "corpus_dist", "eff_num_words",
                "token_doc_diff", "rank_1_docs", "allocation_ratio", "allocation_count", "exclusivity")
DIAG_PROPS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)


def diagnostics_finish(V: int, beta: float, nwsum, topic_doc_counts, word_ids, counts, totals, share_sums, sumsq,
                       codoc, doc_stats) -> np.ndarray:
    """ldatm_diagnostics_finish (host only, no device): the columns
    out[K, len(DIAG_COLUMNS)] from the integer statistics; topic_doc_counts is
    [K, max_len + 1], doc_stats [K, 9]."""
    ids = np.ascontiguousarray(word_ids, np.int32)
    K, n = ids.shape
    a = [np.ascontiguousarray(nwsum, np.int32), np.ascontiguousarray(topic_doc_counts, np.int64), ids,
         np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(totals, np.int64),
         np.ascontiguousarray(share_sums, np.float64), np.ascontiguousarray(sumsq, np.uint64),
         np.ascontiguousarray(codoc, np.int64), np.ascontiguousarray(doc_stats, np.int64)]
    if (a[0].shape != (K,) or a[1].ndim != 2 or a[1].shape[0] != K or any(x.shape != (K, n) for x in a[3:6])
            or a[6].shape != (K,) or a[7].shape != (K, n * (n + 1) // 2) or a[8].shape != (K, 2 + len(DIAG_PROPS))):
        raise ValueError("statistics of the wrong shape")
    out = np.zeros((K, len(DIAG_COLUMNS)), np.float64)
    p = [x.ctypes.data for x in a]
    _check(load_tm().ldatm_diagnostics_finish(K, int(V), n, float(beta), p[0], a[1].shape[1] - 1, *p[1:],
                                              out.ctypes.data), "ldatm_diagnostics_finish")
    return out


# LDATM_COHERENCE_* of lda_topic_model.h
COHERENCE_MEASURES = {"u_mass": 0, "c_uci": 1, "c_npmi": 2}


def coherence_finish(measure, cooc, units: int, n: int | None = None, epsilon=None):
    """ldatm_coherence_finish (host only, no device): (sums[K] fp64 over the
    kept pairs, pairs[K] int64) of a measure ("u_mass", "c_uci", "c_npmi" or
    the LDATM_COHERENCE_* integer) from the triangles cooc[K, n (n + 1) / 2]
    and the number of units; epsilon None: the measure's default."""
    m = COHERENCE_MEASURES.get(measure, measure) if isinstance(measure, str) else int(measure)
    if m not in COHERENCE_MEASURES.values():
        raise ValueError(f"measure must be one of {sorted(COHERENCE_MEASURES)}, not {measure!r}")
    c = np.ascontiguousarray(cooc, np.int64)
    if c.ndim != 2 or c.shape[0] < 1:
        raise ValueError("cooc must be [K, n (n + 1) / 2]")
    K, T = c.shape
    if n is None:
        n = int(round((np.sqrt(8.0 * T + 1.0) - 1.0) / 2.0))
    if n * (n + 1) // 2 != T:
        raise ValueError("cooc must be [K, n (n + 1) / 2]")
    sums, pairs = np.zeros(K, np.float64), np.zeros(K, np.int64)
    _check(load_tm().ldatm_coherence_finish(K, int(n), m, -1.0 if epsilon is None else float(epsilon), c.ctypes.data,
                                            int(units), sums.ctypes.data, pairs.ctypes.data),
           "ldatm_coherence_finish")
    return sums, pairs


class TopicCoherence:
    """What ParallelTopicModel.getCoherence returns: values [K] (each topic's
    mean term over its kept pairs, 0 without one), sums and pairs [K], mean
    (over the topics with a kept pair), wordIds [K, n] and topWords (the lists
    the counts were taken over), cooc [K, n (n + 1) / 2] (the packed
    co-occurrence triangles) and units."""

    def __init__(self, model, measure, window, epsilon, values, pairs, word_ids, cooc, units):
        self.measure, self.window = measure, window
        self.values, self.pairs = values, pairs
        self.sums = coherence_finish(measure, cooc, units, word_ids.shape[1], epsilon)[0]
        self.wordIds, self.cooc, self.units = word_ids, cooc, units
        name = (lambda w: w) if model.alphabet is None else model.alphabet.lookupObject
        self.topWords = [[name(int(w)) for w in row if w >= 0] for row in word_ids]
        kept = pairs > 0
        self.mean = float(values[kept].mean()) if kept.any() else 0.0


class TopicDiagnostics:
    """What ParallelTopicModel.getDiagnostics returns: one array [K] per column
    of DIAG_COLUMNS (tokens, document_entropy, coherence, ...), topWords (per
    topic the (word, ...) list the figures were taken over, heaviest first) and
    codocuments [K, n, n], the symmetric co-document counts of those words
    under the topic (the diagonal: the word's document frequency)."""

    def __init__(self, model, columns, word_ids, codoc):
        self.columns = columns
        self.wordIds = word_ids
        for i, name in enumerate(DIAG_COLUMNS):
            setattr(self, name, columns[:, i].copy())
        name = (lambda w: w) if model.alphabet is None else model.alphabet.lookupObject
        self.topWords = [[name(int(w)) for w in row if w >= 0] for row in word_ids]
        K, n = word_ids.shape
        i, j = np.tril_indices(n)            # row-major lower triangle: i (i + 1) / 2 + j
        self.codocuments = np.zeros((K, n, n), np.int64)
        self.codocuments[:, i, j] = codoc
        self.codocuments[:, j, i] = codoc

    def as_rows(self) -> list:
        """One dict per topic: 'topic', every column, and 'words'."""
        return [dict(topic=k, words=self.topWords[k], **{c: float(self.columns[k, i]) for i, c in enumerate(DIAG_COLUMNS)})
                for k in range(len(self.columns))]


class HeldOutResult:
    """What HeldOutEvaluator.evaluate returns."""

    def __init__(self, logLikelihood: float, tokens: int, perDocument, theta):
        self.logLikelihood = float(logLikelihood)
        self.tokens = int(tokens)
        self.perDocument = perDocument
        self.theta = theta

    @property
    def perplexity(self) -> float:
        return float(np.exp(-self.logLikelihood / self.tokens)) if self.tokens else float("nan")

    def __repr__(self):
        return (f"HeldOutResult(logLikelihood={self.logLikelihood!r}, tokens={self.tokens}, "
                f"perplexity={self.perplexity!r})")


def completion_split(instances, num_types: int):
    """The split HeldOutEvaluator.evaluate makes (ldatm_completion_split,
    host-only): ids outside [0, num_types) are dropped, then the first
    floor(L/2) tokens of each document are observed and the rest scored.
    Returns (obs_off, obs_words, sc_off, sc_words)."""
    off, w = _flatten(list(instances))
    Dh = len(off) - 1
    obs_off, sc_off = np.zeros(Dh + 1, np.int64), np.zeros(Dh + 1, np.int64)
    obs, sc = np.zeros(len(w), np.int32), np.zeros(len(w), np.int32)
    _check(load_tm().ldatm_completion_split(int(num_types), Dh, off.ctypes.data, w.ctypes.data if len(w) else None,
                                            obs_off.ctypes.data, obs.ctypes.data, sc_off.ctypes.data,
                                            sc.ctypes.data), "ldatm_completion_split")
    return obs_off, obs[:obs_off[-1]].copy(), sc_off, sc[:sc_off[-1]].copy()


class HeldOutEvaluator:
    """Held-out log likelihood and perplexity by document completion against
    the model's current counts, on the device (ldatm_evaluate)."""

    def __init__(self, model: ParallelTopicModel):
        self.model = model

    def evaluate(self, instances, numIterations: int = 100, thinning: int = 10, burnIn: int = 10,
                 seed: int = 0) -> HeldOutResult:
        """Each document's first floor(L/2) in-vocabulary tokens are observed
        (getSampledDistribution with these arguments), the rest are scored."""
        off, w = _flatten(list(instances))
        Dh = len(off) - 1
        doc_ll = np.zeros(Dh, np.float64)
        theta = np.zeros((Dh, self.model.numTopics), np.float64)
        total, tokens = C.c_double(0.0), C.c_int64(0)
        _check(self.model._L.ldatm_evaluate(self.model._h, Dh, off.ctypes.data, w.ctypes.data if len(w) else None,
                                            int(numIterations), int(thinning), int(burnIn),
                                            int(seed) & (2**64 - 1), doc_ll.ctypes.data, C.addressof(total),
                                            C.addressof(tokens), theta.ctypes.data), "evaluate")
        return HeldOutResult(total.value, tokens.value, doc_ll, theta)


class LeftToRightResult:
    """What MarginalProbEstimator.leftToRight returns."""

    def __init__(self, logLikelihood: float, tokens: int, perDocument):
        self.logLikelihood = float(logLikelihood)
        self.tokens = int(tokens)
        self.perDocument = perDocument

    @property
    def perplexity(self) -> float:
        return float(np.exp(-self.logLikelihood / self.tokens)) if self.tokens else float("nan")

    def __repr__(self):
        return (f"LeftToRightResult(logLikelihood={self.logLikelihood!r}, tokens={self.tokens}, "
                f"perplexity={self.perplexity!r})")


class MarginalProbEstimator:
    """Mallet's MarginalProbEstimator (ParallelTopicModel.getProbEstimator()):
    the left-to-right particle estimator of log p(w | model) of held-out
    documents against the model's current counts, on the device
    (ldatm_left_to_right)."""

    def __init__(self, model: ParallelTopicModel):
        self.model = model

    def leftToRight(self, instances, numParticles: int = 10, usingResampling: bool = True,
                    seed: int = 0) -> LeftToRightResult:
        """Ids outside the model's vocabulary are dropped and not counted; a
        token whose type has no training tokens is skipped."""
        numParticles = int(numParticles)
        if numParticles < 1:
            raise ValueError("numParticles must be at least 1")
        off, w = _flatten(list(instances))
        Dh = len(off) - 1
        doc_ll = np.zeros(Dh, np.float64)
        total, tokens = C.c_double(0.0), C.c_int64(0)
        _check(self.model._L.ldatm_left_to_right(self.model._h, Dh, off.ctypes.data, w.ctypes.data if len(w) else None,
                                                 numParticles, 1 if usingResampling else 0, int(seed) & (2**64 - 1),
                                                 doc_ll.ctypes.data, C.addressof(total), C.addressof(tokens)),
               "evaluateLeftToRight")
        return LeftToRightResult(total.value, tokens.value, doc_ll)

    def evaluateLeftToRight(self, instances, numParticles: int, usingResampling: bool,
                            docProbabilityStream=None) -> float:
        """Mallet's signature: the total log likelihood; each document's log
        likelihood goes to docProbabilityStream, one line per document (Java's
        Double.toString, as println writes it)."""
        r = self.leftToRight(instances, numParticles, usingResampling)
        if docProbabilityStream is not None:
            for x in r.perDocument:
                docProbabilityStream.write(format_double(float(x)) + "\n")
        return r.logLikelihood


def _doc_ids(docs, model):
    """(int64 ids or None, M) of a scoring call's document list."""
    if docs is None:
        return None, model._shape()[2]
    ids = np.ascontiguousarray(docs, dtype=np.int64).reshape(-1)
    return ids, len(ids)


class TopicInferencer:
    """getSampledDistribution against the model's current (frozen) counts."""

    def __init__(self, model: ParallelTopicModel):
        self.model = model

    def getSampledDistributions(self, instances, numIterations: int = 100, thinning: int = 10,
                                burnIn: int = 10, seed: int = 0) -> np.ndarray:
        off, w = _flatten(list(instances))
        theta = np.zeros((len(off) - 1, self.model.numTopics), np.float64)
        _check(self.model._L.ldatm_infer(self.model._h, len(off) - 1, off,
                                         w.ctypes.data if len(w) else None, int(numIterations),
                                         int(thinning), int(burnIn), int(seed) & (2**64 - 1), theta),
               "getSampledDistribution")
        return theta

    def scoreInstances(self, instances, numIterations: int = 100, thinning: int = 10,
                       burnIn: int = 10, seed: int = 0, docs=None, metric="cosine"):
        """getSampledDistributions of `instances`, then their similarity to the
        training documents `docs` (None = all) as scoreDistributions, in one
        native call: (scores[Q, M], theta[Q, K])."""
        m = capi.score_metric(metric)
        off, w = _flatten(list(instances))
        ids, M = _doc_ids(docs, self.model)
        Q = len(off) - 1
        theta = np.zeros((Q, self.model.numTopics), np.float64)
        scores = np.zeros((Q, M), np.float64)
        _check(self.model._L.ldatm_score(self.model._h, m, Q, off.ctypes.data, w.ctypes.data if len(w) else None,
                                         int(numIterations), int(thinning), int(burnIn),
                                         int(seed) & (2**64 - 1), M,
                                         ids.ctypes.data if ids is not None and M else None,
                                         scores.ctypes.data, theta.ctypes.data), "scoreInstances")
        return scores, theta

    def nearestInstances(self, instances, n: int = 10, metric="hellinger", numIterations: int = 100,
                         thinning: int = 10, burnIn: int = 10, seed: int = 0, minTokens: int = 1):
        """getSampledDistributions of `instances`, then the model's
        nearestDocuments of those rows: (docs[Q, n], values[Q, n])."""
        n = capi.doc_nearest_n(n)
        m = capi.doc_metric(metric)
        theta = self.getSampledDistributions(instances, numIterations, thinning, burnIn, seed)
        return self.model.nearestDocuments(theta, n, m, minTokens)

    def getSampledDistribution(self, instance, numIterations: int = 100, thinning: int = 10,
                               burnIn: int = 10, seed: int = 0) -> np.ndarray:
        if not isinstance(instance, Instance):
            instance = Instance(instance)
        return self.getSampledDistributions([instance], numIterations, thinning, burnIn, seed)[0]


def plan_shards(num_threads: int, num_devices: int, num_tokens: int, num_types: int,
                num_topics: int, num_docs: int) -> int:
    """GPU shards setNumThreads(num_threads) becomes for this corpus
    (ldatm_plan_shards; host-only)."""
    return int(load_tm().ldatm_plan_shards(int(num_threads), int(num_devices), int(num_tokens),
                                           int(num_types), int(num_topics), int(num_docs)))
