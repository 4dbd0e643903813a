"""GibbsSampler: one document shard on one MI355X, driven through the C ABI.

This is the thin host object over ``lda_ctx`` (include/lda_mi355x.h).  It is
what ParallelTopicModel.estimate() (topic_model.py) and the AD-LDA driver
(distributed.py) run; it has no CPU path — every call goes to
liblda_mi355x.so and raises LdaError on failure.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


def staleness_schedule(threads: int):
    """lda_staleness_schedule: (parts, fractions) of the sequential sweeps that
    give every token the mean live fraction of Mallet's `threads` worker
    threads (the native ParallelTopicModel's default schedule
    past the warm start, what the Java drop-in runs)."""
    L = capi.load()
    parts = C.c_int32()
    fr = np.zeros(capi.MAX_EXCHANGE_PARTS, dtype=np.float64)
    capi.check(L.lda_staleness_schedule(int(threads), C.byref(parts), fr.ctypes.data),
               "lda_staleness_schedule")
    return int(parts.value), fr[:parts.value].copy()


class _DeviceArray:
    """Exposes a device pointer through __cuda_array_interface__ (zero-copy
    torch.as_tensor view of the delta buffer for torch.distributed)."""

    def __init__(self, ptr: int, count: int, typestr: str = "<i4"):
        self.__cuda_array_interface__ = {
            "shape": (count,),
            "typestr": typestr,
            "data": (ptr, False),
            "version": 3,
            "strides": None,
        }


class GibbsSampler:
    def __init__(self, num_topics: int, num_types: int, doc_off, words, alpha, beta: float,
                 seed: int = 0, z_init=None, device: int = 0, token_base: int = 0,
                 tokens_per_range: int = 0, sampler: str = "dense"):
        L = capi.load()
        self.K = int(num_topics)
        self.V = int(num_types)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
        words = np.ascontiguousarray(words, dtype=np.int32)
        if len(doc_off) < 1:
            raise ValueError("doc_off needs at least one entry")
        self.D = len(doc_off) - 1
        self.N = int(doc_off[-1] - doc_off[0])
        if len(words) < self.N:
            raise ValueError(f"words holds {len(words)} ids, doc_off spans {self.N}")
        if z_init is not None and len(z_init) != self.N:
            raise ValueError(f"z_init must hold {self.N} topics")
        alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (self.K,)))
        self._alpha = alpha
        cfg = capi.lda_config()
        cfg.num_topics = self.K
        cfg.num_types = self.V
        cfg.num_docs = self.D
        cfg.alpha = alpha.ctypes.data_as(C.POINTER(C.c_double))
        cfg.beta = float(beta)
        cfg.seed = int(seed) & (2**64 - 1)
        cfg.device = int(device)
        cfg.sampler = capi.SAMPLERS[sampler]
        self.sampler_kind = sampler
        cfg.token_base = int(token_base)
        cfg.tokens_per_range = int(tokens_per_range)
        zp = None
        if z_init is not None:
            self._z_init = np.ascontiguousarray(z_init, dtype=np.int32)
            zp = self._z_init.ctypes.data
        h = C.c_void_p()
        capi.check(L.lda_create(C.byref(h), C.byref(cfg), doc_off,
                                words.ctypes.data if self.N else None, zp), "lda_create")
        self._h = h
        self._L = L
        self.device = int(device)
        kp = C.c_int32()
        capi.check(L.lda_get_shape(h, None, C.byref(kp), None, None, None), "lda_get_shape")
        self.Kp = kp.value
        self.beta = float(beta)

    # ---------------------------------------------------------------- life
    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.lda_destroy(h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # --------------------------------------------------------------- sweeps
    def sweep(self, n: int = 1):
        capi.check(self._L.lda_sweep(self._h, int(n)), "lda_sweep")

    def sample(self):
        capi.check(self._L.lda_sample(self._h), "lda_sample")

    def apply(self):
        capi.check(self._L.lda_apply(self._h), "lda_apply")

    def delta_buffer(self, part: int = 0):
        ptr, cnt = C.c_void_p(), C.c_size_t()
        capi.check(self._L.lda_delta_buffer_part(self._h, int(part), C.byref(ptr), C.byref(cnt)),
                   "lda_delta_buffer_part")
        return int(ptr.value), int(cnt.value)

    def delta_tensor(self, part: int = 0):
        """Zero-copy torch int32 view of the pending delta of split-sweep part
        `part` (device memory; part 0 is lda_delta_buffer)."""
        import torch

        ptr, cnt = self.delta_buffer(part)
        t = torch.as_tensor(_DeviceArray(ptr, cnt), device=f"cuda:{self.device}")
        assert t.data_ptr() == ptr and t.dtype == torch.int32
        return t

    # ------------------------------------------------ compact exchange (§5)
    def exchange_sizes(self, world: int, max_tokens: int):
        """(packed int32 words, escape-list int32 words) of lda_exchange_pack."""
        a, b = C.c_size_t(), C.c_size_t()
        capi.check(self._L.lda_exchange_sizes(self._h, int(world), int(max_tokens), C.byref(a),
                                              C.byref(b)), "lda_exchange_sizes")
        return int(a.value), int(b.value)

    def set_exchange_cells(self, cells_per_word: int):
        """lda_set_exchange_cells: 2 (default) or 4 cells per packed exchange
        word (half the bytes, narrower fields, more escapes)."""
        capi.check(self._L.lda_set_exchange_cells(self._h, int(cells_per_word)), "lda_set_exchange_cells")

    @property
    def exchange_cells(self) -> int:
        n = C.c_int32()
        capi.check(self._L.lda_get_exchange_cells(self._h, C.byref(n)), "lda_get_exchange_cells")
        return int(n.value)

    def exchange_pack(self, part: int, world: int, max_tokens: int):
        """Pack part `part`'s exchange buffer (lda_exchange_pack, on this
        context's stream): zero-copy torch int32 views (packed words to
        SUM-all-reduce, this rank's escape list to all-gather)."""
        import torch
        pk, es = C.c_void_p(), C.c_void_p()
        capi.check(self._L.lda_exchange_pack(self._h, int(part), int(world), int(max_tokens),
                                             C.byref(pk), C.byref(es)), "lda_exchange_pack")
        n_pk, n_es = self.exchange_sizes(world, max_tokens)
        dev = f"cuda:{self.device}"
        return (torch.as_tensor(_DeviceArray(int(pk.value), n_pk), device=dev),
                torch.as_tensor(_DeviceArray(int(es.value), n_es), device=dev))

    def exchange_unpack(self, part: int, world: int, max_tokens: int, escapes_all, list_cap=None):
        """lda_exchange_unpack: the part's buffer = the summed packed words +
        every rank's escapes (escapes_all: device int32 [world x escape len]).
        list_cap: the lists were all-gathered at 1 + 3 list_cap int32 each
        (lda_exchange_unpack_lists; 0 with escapes_all None: no rank had one)."""
        if list_cap is None:
            assert escapes_all.dtype.itemsize == 4 and escapes_all.is_contiguous()
            capi.check(self._L.lda_exchange_unpack(self._h, int(part), int(world), int(max_tokens),
                                                   C.c_void_p(escapes_all.data_ptr())),
                       "lda_exchange_unpack")
            return
        ptr = None
        if escapes_all is not None:
            assert escapes_all.dtype.itemsize == 4 and escapes_all.is_contiguous()
            assert escapes_all.numel() == world * (1 + 3 * int(list_cap))
            ptr = C.c_void_p(escapes_all.data_ptr())
        capi.check(self._L.lda_exchange_unpack_lists(self._h, int(part), int(world), int(max_tokens), ptr,
                                                     int(list_cap)), "lda_exchange_unpack_lists")

    # ------------------------------------------------- split sweep (§5)
    def set_exchange_parts(self, parts: int, reserve_cus: int = 0):
        """Cut each sweep into `parts` token-balanced parts with their own delta
        buffers, so one part's all-reduce can overlap the next part's sampling
        (lda_set_exchange_parts)."""
        capi.check(self._L.lda_set_exchange_parts(self._h, int(parts), int(reserve_cus)),
                   "lda_set_exchange_parts")

    @property
    def exchange_parts(self) -> int:
        n = C.c_int32()
        capi.check(self._L.lda_get_exchange_parts(self._h, C.byref(n)), "lda_get_exchange_parts")
        return n.value

    def sample_part(self, part: int):
        capi.check(self._L.lda_sample_part(self._h, int(part)), "lda_sample_part")

    def set_stream(self, stream_handle: int | None):
        capi.check(self._L.lda_set_stream(self._h, stream_handle), "lda_set_stream")

    def stream_handle(self) -> int:
        """The hipStream_t every call of this context is ordered on."""
        h = C.c_void_p()
        capi.check(self._L.lda_get_stream(self._h, C.byref(h)), "lda_get_stream")
        return int(h.value or 0)

    def synchronize(self):
        capi.check(self._L.lda_synchronize(self._h), "lda_synchronize")

    @property
    def sweep_index(self) -> int:
        s = C.c_uint32()
        capi.check(self._L.lda_get_sweep(self._h, C.byref(s)), "lda_get_sweep")
        return s.value

    @sweep_index.setter
    def sweep_index(self, v: int):
        capi.check(self._L.lda_set_sweep(self._h, int(v)), "lda_set_sweep")

    def last_sample_ms(self) -> float:
        ms = C.c_float()
        capi.check(self._L.lda_last_sample_ms(self._h, C.byref(ms)), "lda_last_sample_ms")
        return float(ms.value)

    def sample_times(self, last: int) -> np.ndarray:
        """Kernel durations (ms) of the last `last` lda_sample launches."""
        ms = np.zeros(max(int(last), 0), dtype=np.float32)
        n = C.c_int32()
        capi.check(self._L.lda_sample_times(self._h, len(ms), ms.ctypes.data if len(ms) else None,
                                            C.byref(n)), "lda_sample_times")
        return ms[:n.value]

    def recount_times(self, last: int) -> np.ndarray:
        """Kernel durations (ms) of the recount after each of the last `last`
        lda_sample launches (zeros in the delta mode)."""
        ms = np.zeros(max(int(last), 0), dtype=np.float32)
        n = C.c_int32()
        capi.check(self._L.lda_recount_times(self._h, len(ms), ms.ctypes.data if len(ms) else None,
                                             C.byref(n)), "lda_recount_times")
        return ms[:n.value]

    def set_warm_start(self, parts: int = 4, sweeps: int = 50, corpus_first_token: int = 0,
                       corpus_tokens: int = 0):
        """lda_set_warm_start: sweeps whose sweep counter is below `sweeps` run in
        `parts` sequential parts (parts = 1: off), cut in the whole corpus of
        global tokens [corpus_first_token, + corpus_tokens) (0: this shard)."""
        capi.check(self._L.lda_set_warm_start(self._h, int(parts), int(sweeps), int(corpus_first_token),
                                              int(corpus_tokens)), "lda_set_warm_start")

    def set_sequential_sweeps(self, parts: int = 1, fractions=None, corpus_first_token: int = 0,
                              corpus_tokens: int = 0):
        """lda_set_sequential_sweeps: every sweep past the warm start in `parts`
        sequential parts, part i the fraction fractions[i] of every block
        (None: equal parts; parts = 1: plain snapshot sweeps)."""
        fr = None
        if parts > 1 and fractions is not None:
            self._seq_fr = np.ascontiguousarray(fractions, dtype=np.float64)
            assert self._seq_fr.shape == (parts,)
            fr = self._seq_fr.ctypes.data
        capi.check(self._L.lda_set_sequential_sweeps(self._h, int(parts), fr, int(corpus_first_token),
                                                     int(corpus_tokens)), "lda_set_sequential_sweeps")

    def sequential_sweeps(self):
        """(parts, cumulative cuts in units of 1/LDA_SEQ_FRACTION_UNIT)."""
        n = C.c_int32()
        cum = np.zeros(capi.MAX_EXCHANGE_PARTS + 1, dtype=np.int64)
        capi.check(self._L.lda_get_sequential_sweeps(self._h, C.byref(n), cum.ctypes.data),
                   "lda_get_sequential_sweeps")
        return int(n.value), cum[:n.value + 1].tolist()

    def sweep_parts(self):
        """(parts, sequential) of the sweep in progress or the next one."""
        p, q = C.c_int32(), C.c_int32()
        capi.check(self._L.lda_sweep_parts(self._h, C.byref(p), C.byref(q)), "lda_sweep_parts")
        return p.value, bool(q.value)

    def set_count_update(self, mode: str = "auto", recount_sweeps: int = -1):
        """Which sweeps recount (lda_set_count_update): "auto" (the first
        `recount_sweeps` sweeps after the counts are seeded; -1 keeps the
        library's choice), "recount" (all) or "delta" (none)."""
        capi.check(self._L.lda_set_count_update(self._h, capi.COUNT_UPDATE[mode], int(recount_sweeps)),
                   "lda_set_count_update")

    def count_update(self):
        """(mode name, recount_sweeps)."""
        m, r = C.c_int32(), C.c_int32()
        capi.check(self._L.lda_get_count_update(self._h, C.byref(m), C.byref(r)), "lda_get_count_update")
        return {v: k for k, v in capi.COUNT_UPDATE.items()}[m.value], r.value

    @property
    def recount(self) -> bool:
        """True when the exchange buffer holds recounted counts (dense samplers),
        False when it holds a delta (lda_count_update_mode)."""
        r = C.c_int32()
        capi.check(self._L.lda_count_update_mode(self._h, C.byref(r)), "lda_count_update_mode")
        return bool(r.value)

    # ---------------------------------------------------------------- state
    def z(self) -> np.ndarray:
        out = np.empty(self.N, dtype=np.int32)
        capi.check(self._L.lda_get_z(self._h, out), "lda_get_z")
        return out

    def set_z(self, z):
        z = np.ascontiguousarray(z, dtype=np.int32)
        if z.shape != (self.N,):
            raise ValueError(f"z must hold {self.N} topics, got shape {z.shape}")
        capi.check(self._L.lda_set_z(self._h, z), "lda_set_z")

    def counts(self, with_nd: bool = False):
        nw = np.empty((self.V, self.K), dtype=np.int32)
        nwsum = np.empty(self.K, dtype=np.int32)
        nd = np.empty((self.D, self.K), dtype=np.int32) if with_nd else None
        ndsum = np.empty(self.D, dtype=np.int32)
        capi.check(self._L.lda_get_counts(self._h, nw.ctypes.data, nwsum.ctypes.data,
                                          nd.ctypes.data if with_nd else None,
                                          ndsum.ctypes.data), "lda_get_counts")
        return nw, nwsum, nd, ndsum

    def counts_checksum(self) -> int:
        """lda_counts_checksum: a hash of the applied nw / nwsum (equal on every
        replica; oracle.counts_checksum of counts()'s nw, nwsum)."""
        h = C.c_uint64()
        capi.check(self._L.lda_counts_checksum(self._h, C.byref(h)), "lda_counts_checksum")
        return int(h.value)

    def set_alpha_beta(self, alpha, beta: float):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (self.K,)))
        capi.check(self._L.lda_set_alpha_beta(self._h, a, float(beta)), "lda_set_alpha_beta")
        self._alpha = a
        self.beta = float(beta)

    @property
    def alpha(self) -> np.ndarray:
        return self._alpha.copy()

    def log_likelihood_parts(self):
        a, b = C.c_double(), C.c_double()
        capi.check(self._L.lda_log_likelihood_parts(self._h, C.byref(a), C.byref(b)),
                   "lda_log_likelihood_parts")
        return a.value, b.value

    def log_likelihood(self) -> float:
        out = C.c_double()
        capi.check(self._L.lda_log_likelihood(self._h, C.byref(out)), "lda_log_likelihood")
        return out.value

    def infer(self, doc_off, words, n_iter: int = 100, thin: int = 10, burn_in: int = 10,
              seed: int = 0) -> np.ndarray:
        """TopicInferencer.getSampledDistribution(inst, numIterations, thinning,
        burnIn) over a batch of documents (positional order as Mallet's)."""
        doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
        words = np.ascontiguousarray(words, dtype=np.int32)
        if len(doc_off) < 1:
            raise ValueError("doc_off needs at least one entry")
        if len(words) < int(doc_off[-1] - doc_off[0]):
            raise ValueError("words is shorter than doc_off says")
        Dh = len(doc_off) - 1
        theta = np.zeros((Dh, self.K), dtype=np.float64)
        capi.check(self._L.lda_infer(self._h, Dh, doc_off, words, int(n_iter), int(thin),
                                     int(burn_in), int(seed) & (2**64 - 1), theta), "lda_infer")
        return theta

    def score_docs(self, theta, metric="cosine", docs=None, doc_begin: int = 0,
                   num_docs: int | None = None) -> np.ndarray:
        """lda_score_docs: similarity ("cosine" or "mse") of the rows of
        theta[Q, K] to this shard's documents' topic distributions, computed on
        the device from z.  docs: document ids (any order, duplicates allowed);
        None: documents [doc_begin, doc_begin + num_docs) (default: to the
        end).  Returns scores[Q, M] (fp64)."""
        theta = capi.as_theta(theta, self.K)
        m = capi.score_metric(metric)
        if docs is not None:
            ids = np.ascontiguousarray(docs, dtype=np.int64).reshape(-1)
            M, begin, idp = len(ids), 0, (ids.ctypes.data if len(ids) else None)
        else:
            begin = int(doc_begin)
            M, idp = (self.D - begin if num_docs is None else int(num_docs)), None
        scores = np.zeros((len(theta), max(M, 0)), dtype=np.float64)
        capi.check(self._L.lda_score_docs(self._h, m, len(theta), theta.ctypes.data, begin, M, idp,
                                          scores.ctypes.data), "lda_score_docs")
        return scores

    def _doc_list(self, docs, doc_begin, num_docs):
        """(begin, M, ids or None) of a document argument as score_docs takes it."""
        if docs is not None:
            ids = np.ascontiguousarray(docs, dtype=np.int64).reshape(-1)
            return 0, len(ids), ids
        begin = int(doc_begin)
        return begin, (self.D - begin if num_docs is None else int(num_docs)), None

    def top_words(self, n: int):
        """lda_top_words: per topic the n words with the largest count (count
        descending, equal counts by ascending word id), selected on the device.
        Returns (word_ids[K, n], counts[K, n]) int32; slots past a topic's last
        nonzero word hold -1 / 0."""
        n = int(n)
        if not 1 <= n <= capi.TOP_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOP_WORDS_MAX}]")
        ids = np.zeros((self.K, n), dtype=np.int32)
        cnt = np.zeros((self.K, n), dtype=np.int32)
        capi.check(self._L.lda_top_words(self._h, n, ids.ctypes.data, cnt.ctypes.data), "lda_top_words")
        return ids, cnt

    def relevant_words(self, n: int, lambdas=0.6):
        """lda_relevant_words: for each lambda (a scalar or a sequence of up to
        RELEVANCE_LAMBDAS_MAX values in [0, 1]) and topic, the n words with
        nw[w, k] > 0 of largest relevance lambda logprob + (1 - lambda) loglift
        (Sievert & Shirley 2014), equal keys by ascending word id, selected on
        the device.  Returns (word_ids, counts int32, totals int64, logprob,
        loglift float64), each [L, K, n]; slots past a topic's last candidate
        hold -1 / 0 / 0 / 0.0 / 0.0."""
        n = int(n)
        if not 1 <= n <= capi.TOP_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOP_WORDS_MAX}]")
        lam = capi.check_lambdas(lambdas)
        shape = (lam.size, self.K, n)
        ids = np.zeros(shape, dtype=np.int32)
        cnt = np.zeros(shape, dtype=np.int32)
        tot = np.zeros(shape, dtype=np.int64)
        lp = np.zeros(shape, dtype=np.float64)
        ll = np.zeros(shape, dtype=np.float64)
        capi.check(self._L.lda_relevant_words(self._h, n, lam.size, lam.ctypes.data, ids.ctypes.data, cnt.ctypes.data,
                                              tot.ctypes.data, lp.ctypes.data, ll.ctypes.data), "lda_relevant_words")
        return ids, cnt, tot, lp, ll

    def salient_words(self, n: int):
        """lda_salient_words: the n words of largest saliency (Chuang et al.
        2012), equal values by ascending word id, selected on the device.
        Returns (word_ids[n] int32, totals[n] int64, saliency[n],
        distinctiveness[n] float64); -1 / 0 / 0.0 / 0.0 past the last word
        with a token."""
        n = int(n)
        if not 1 <= n <= capi.SALIENT_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.SALIENT_WORDS_MAX}]")
        ids = np.zeros(n, dtype=np.int32)
        tot = np.zeros(n, dtype=np.int64)
        sal = np.zeros(n, dtype=np.float64)
        dist = np.zeros(n, dtype=np.float64)
        capi.check(self._L.lda_salient_words(self._h, n, ids.ctypes.data, tot.ctypes.data, sal.ctypes.data,
                                             dist.ctypes.data), "lda_salient_words")
        return ids, tot, sal, dist

    def word_rows(self, word_ids):
        """lda_word_rows: (rows[M, K] int32, totals[M] int64) of the listed
        words (any order, duplicates allowed), gathered on the device."""
        ids = np.ascontiguousarray(word_ids, dtype=np.int32).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= self.V):
            raise ValueError(f"word ids must be in [0, {self.V})")
        rows = np.zeros((ids.size, self.K), dtype=np.int32)
        tot = np.zeros(ids.size, dtype=np.int64)
        capi.check(self._L.lda_word_rows(self._h, ids.size, ids.ctypes.data if ids.size else None,
                                         rows.ctypes.data if ids.size else None,
                                         tot.ctypes.data if ids.size else None), "lda_word_rows")
        return rows, tot

    def doc_top_topics(self, m: int, docs=None, doc_begin: int = 0, num_docs: int | None = None):
        """lda_doc_top_topics: the m topics of each listed document with the
        largest weight (alpha_k + n_dk) / (n_d + alphaSum), equal weights by
        ascending topic id, selected on the device from z.  docs as score_docs
        takes them.  Returns (topics[M, m], counts[M, m]) int32; slots past K
        hold -1 / 0."""
        m = int(m)
        if not 1 <= m <= capi.TOP_TOPICS_MAX:
            raise ValueError(f"m must be in [1, {capi.TOP_TOPICS_MAX}]")
        begin, M, ids = self._doc_list(docs, doc_begin, num_docs)
        topics = np.zeros((max(M, 0), m), dtype=np.int32)
        cnt = np.zeros((max(M, 0), m), dtype=np.int32)
        capi.check(self._L.lda_doc_top_topics(self._h, m, begin, M, ids.ctypes.data if ids is not None and M else None,
                                              topics.ctypes.data, cnt.ctypes.data), "lda_doc_top_topics")
        return topics, cnt

    def doc_counts(self, docs=None, doc_begin: int = 0, num_docs: int | None = None) -> np.ndarray:
        """lda_doc_counts: the topic counts nd[M, K] (int32) of the listed
        documents from the current z on the device; docs as score_docs takes
        them."""
        begin, M, ids = self._doc_list(docs, doc_begin, num_docs)
        nd = np.zeros((max(M, 0), self.K), dtype=np.int32)
        capi.check(self._L.lda_doc_counts(self._h, begin, M, ids.ctypes.data if ids is not None and M else None,
                                          nd.ctypes.data), "lda_doc_counts")
        return nd

    def topic_top_docs(self, n: int, smoothing: float = 0.0, min_tokens: int = 1):
        """lda_topic_top_docs: per topic the n documents of this shard with at
        least one token of the topic and at least min_tokens tokens that have
        the largest weight (n_dk + smoothing) / (L_d + K smoothing), equal
        weights by ascending document id, selected on the device from z.
        Returns (docs[K, n] int64, counts[K, n] int32, lengths[K, n] int32);
        slots past a topic's last candidate hold -1 / 0 / 0."""
        n = int(n)
        if not 1 <= n <= capi.TOPIC_DOCS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOPIC_DOCS_MAX}]")
        docs = np.zeros((self.K, n), dtype=np.int64)
        cnt = np.zeros((self.K, n), dtype=np.int32)
        lens = np.zeros((self.K, n), dtype=np.int32)
        capi.check(self._L.lda_topic_top_docs(self._h, n, float(smoothing), int(min_tokens), docs.ctypes.data,
                                              cnt.ctypes.data, lens.ctypes.data), "lda_topic_top_docs")
        return docs, cnt, lens

    def topic_phrases(self, n: int, min_len: int = 2, max_len: int = 32, min_count: int = 1):
        """lda_topic_phrases: per topic the n most frequent same-topic token
        runs (phrases) of this shard with min_len <= length <= max_len and
        count >= min_count, by count descending, then word ids ascending, a
        prefix before its extension, counted on the device from words and z.
        Returns (words[K, n, max_len] int32 (-1 padded), lengths[K, n] int32,
        counts[K, n] int64, first[K, n] int64 (smallest token index of the
        phrase; -1 in an empty slot), runs[K] int64, distinct[K] int64,
        skipped_long int)."""
        n, min_len, max_len = int(n), int(min_len), int(max_len)
        if not 1 <= n <= capi.PHRASES_MAX:
            raise ValueError(f"n must be in [1, {capi.PHRASES_MAX}]")
        if not 2 <= min_len <= max_len <= capi.PHRASE_LEN_MAX:
            raise ValueError(f"the lengths must satisfy 2 <= min_len <= max_len <= {capi.PHRASE_LEN_MAX}")
        words = np.zeros((self.K, n, max_len), dtype=np.int32)
        lens = np.zeros((self.K, n), dtype=np.int32)
        cnt = np.zeros((self.K, n), dtype=np.int64)
        first = np.zeros((self.K, n), dtype=np.int64)
        runs = np.zeros(self.K, dtype=np.int64)
        distinct = np.zeros(self.K, dtype=np.int64)
        skipped = C.c_int64()
        capi.check(self._L.lda_topic_phrases(self._h, n, min_len, max_len, int(min_count), words.ctypes.data,
                                             lens.ctypes.data, cnt.ctypes.data, first.ctypes.data, runs.ctypes.data,
                                             distinct.ctypes.data, C.addressof(skipped)), "lda_topic_phrases")
        return words, lens, cnt, first, runs, distinct, int(skipped.value)

    def phrase_counts(self, topics, phrases, min_len: int = 2, max_len: int = 32, with_first: bool = False):
        """lda_phrase_counts: the exact number of qualifying runs of each
        (topics[q], phrases[q]) in this shard, phrases[q] a sequence of word
        ids; 0 for one never seen or of a length outside [min_len, max_len].
        Returns counts[Q] int64; with_first (lda_phrase_lookup) also the
        smallest token index of each phrase, -1 where the count is 0."""
        topics = np.ascontiguousarray(topics, dtype=np.int32).reshape(-1)
        Q = len(topics)
        if len(phrases) != Q:
            raise ValueError("one phrase per topic entry")
        off = np.zeros(Q + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(p) for p in phrases])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32).reshape(-1) for p in phrases])
                                    if Q else np.zeros(0), dtype=np.int32)
        cnt = np.zeros(Q, dtype=np.int64)
        first = np.full(Q, -1, dtype=np.int64)
        if with_first:
            capi.check(self._L.lda_phrase_lookup(self._h, int(min_len), int(max_len), Q, topics.ctypes.data,
                                                 off.ctypes.data, flat.ctypes.data, cnt.ctypes.data,
                                                 first.ctypes.data), "lda_phrase_lookup")
            return cnt, first
        capi.check(self._L.lda_phrase_counts(self._h, int(min_len), int(max_len), Q, topics.ctypes.data,
                                             off.ctypes.data, flat.ctypes.data, cnt.ctypes.data), "lda_phrase_counts")
        return cnt

    def topic_cooccurrence(self, stats=capi.TOPIC_COOC_STATS, min_tokens: int = 10, min_count: int = 2,
                           min_prop: float = 0.05) -> dict:
        """lda_topic_cooccurrence: which topics share this shard's documents,
        counted on the device from z.  A document is used with at least
        min_tokens tokens; topic k is present in it with n_dk >= min_count and
        n_dk >= min_prop * L_d.  Returns a dict: "docs_used" (int), "tokens"
        [K] and "present" [K] (int64), and of "codocs" / "overlap" / "product"
        ([K, K] int64: documents with both present, sum of min(n_dk, n_dl), sum
        of n_dk n_dl) those named in stats; only they are counted."""
        stats = capi.topic_cooc_stats(stats)
        min_tokens, min_count, min_prop = capi.topic_cooc_thresholds(min_tokens, min_count, min_prop)
        used = C.c_int64()
        out = {"tokens": np.zeros(self.K, np.int64), "present": np.zeros(self.K, np.int64)}
        for s in stats:
            out[s] = np.zeros((self.K, self.K), np.int64)
        tabs = [out[s].ctypes.data if s in out else None for s in capi.TOPIC_COOC_STATS]
        capi.check(self._L.lda_topic_cooccurrence(self._h, min_tokens, min_count, min_prop, C.byref(used),
                                                  out["tokens"].ctypes.data, out["present"].ctypes.data, *tabs),
                   "lda_topic_cooccurrence")
        out["docs_used"] = int(used.value)
        return out

    def group_topics(self, doc_group, G=None, stats=capi.GROUP_TOPICS_STATS, min_tokens: int = 10,
                     min_count: int = 2, min_prop: float = 0.05) -> dict:
        """lda_group_topics: how much of each group of this shard's documents is
        each topic, counted on the device from z.  doc_group holds one id in
        [-1, G) per document (-1 leaves it out; G = None: the largest id plus
        one).  A document is used with a group >= 0 and at least min_tokens
        tokens; topic k is present in it with n_dk >= min_count and n_dk >=
        min_prop * L_d.  Returns a dict: "group_docs" [G] and "group_tokens"
        [G] (int64: the used documents and their tokens), "tokens" [G, K]
        (int64: sum of n_dk) and, of "present" ([G, K] int64: documents with k
        present) and "shares" ([G, K] uint64: sum of floor(n_dk 2^32 / L_d))
        those named in stats; only they are counted."""
        stats = capi.group_topics_stats(stats)
        min_tokens, min_count, min_prop = capi.topic_cooc_thresholds(min_tokens, min_count, min_prop)
        ids, G = capi.group_ids(doc_group, self.D, G)
        out = {"group_docs": np.zeros(G, np.int64), "group_tokens": np.zeros(G, np.int64),
               "tokens": np.zeros((G, self.K), np.int64)}
        for s in stats:
            out[s] = np.zeros((G, self.K), np.uint64 if s == "shares" else np.int64)
        tabs = [out[s].ctypes.data if s in out else None for s in capi.GROUP_TOPICS_STATS]
        capi.check(self._L.lda_group_topics(self._h, ids.ctypes.data, G, min_tokens, min_count, min_prop,
                                            out["group_docs"].ctypes.data, out["group_tokens"].ctypes.data,
                                            out["tokens"].ctypes.data, *tabs), "lda_group_topics")
        return out

    def subcorpus_count(self, mask, accumulate: bool = False):
        """lda_subcorpus_count: the context's sub-corpus table sub[V, Kp]
        becomes (accumulate: grows by) the (word, topic) counts of this shard's
        documents whose mask entry is nonzero.  The table is a snapshot of z
        now; sampling never touches it."""
        m = capi.doc_mask(mask, self.D)
        capi.check(self._L.lda_subcorpus_count(self._h, m.ctypes.data, 1 if accumulate else 0),
                   "lda_subcorpus_count")

    def subcorpus_merge(self, other: "GibbsSampler"):
        """lda_subcorpus_merge: this context's table += other's (same V and K,
        a table each); other's is unchanged."""
        if not isinstance(other, GibbsSampler):
            raise TypeError("other must be a GibbsSampler")
        capi.check(self._L.lda_subcorpus_merge(self._h, other._h), "lda_subcorpus_merge")

    def subcorpus_top_words(self, n: int):
        """lda_subcorpus_top_words: top_words' selection on the sub-corpus
        table.  Returns (word_ids[K, n], counts[K, n]) int32, -1 / 0 past a
        topic's last nonzero word, and totals[K] int64, each topic's tokens in
        the sub-corpus."""
        n = int(n)
        if not 1 <= n <= capi.TOP_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.TOP_WORDS_MAX}]")
        ids = np.zeros((self.K, n), dtype=np.int32)
        cnt = np.zeros((self.K, n), dtype=np.int32)
        tot = np.zeros(self.K, dtype=np.int64)
        capi.check(self._L.lda_subcorpus_top_words(self._h, n, ids.ctypes.data, cnt.ctypes.data, tot.ctypes.data),
                   "lda_subcorpus_top_words")
        return ids, cnt, tot

    def subcorpus_release(self):
        """lda_subcorpus_release: frees the sub-corpus table, if there is one."""
        capi.check(self._L.lda_subcorpus_release(self._h), "lda_subcorpus_release")

    def _word_lists(self, word_ids):
        """(ids[K, n] int32, n) of K word lists, -1 = an empty slot."""
        ids = np.ascontiguousarray(word_ids, dtype=np.int32)
        if ids.ndim != 2 or ids.shape[0] != self.K:
            raise ValueError("word_ids must be [K, n]")
        if not 1 <= ids.shape[1] <= capi.DIAG_WORDS_MAX:
            raise ValueError(f"n must be in [1, {capi.DIAG_WORDS_MAX}]")
        return ids, ids.shape[1]

    def topic_codocuments(self, word_ids, props=()):
        """lda_topic_codocuments over this shard's documents and current z.
        word_ids[K, n] (-1 = empty slot), props ascending in (0, 1].  Returns
        (codoc[K, n (n + 1) / 2] int32, each topic's packed lower triangle,
        cell (i, j), j <= i, at i (i + 1) / 2 + j: documents holding both words
        under that topic; doc_stats[K, 2 + P] int64: documents with the topic,
        documents it ranks first in, documents where its weight reaches each
        proportion)."""
        ids, n = self._word_lists(word_ids)
        p = np.ascontiguousarray(props, dtype=np.float64).reshape(-1)
        if len(p) > capi.DIAG_PROPS_MAX:
            raise ValueError(f"at most {capi.DIAG_PROPS_MAX} props")
        codoc = np.zeros((self.K, n * (n + 1) // 2), dtype=np.int32)
        stats = np.zeros((self.K, 2 + len(p)), dtype=np.int64)
        capi.check(self._L.lda_topic_codocuments(self._h, n, ids.ctypes.data, len(p), p.ctypes.data if len(p) else None,
                                                 codoc.ctypes.data, stats.ctypes.data), "lda_topic_codocuments")
        return codoc, stats

    def topic_word_stats(self, word_ids):
        """lda_topic_word_stats from the global counts: (counts[K, n] int32 =
        nw[w, k], totals[K, n] int64 = the word's total, share_sums[K, n] fp64 =
        sum over topics of (beta + nw[w, k']) / (V beta + nwsum[k']),
        sumsq[K] uint64 = sum over words of nw[w, k]^2); empty slots 0."""
        ids, n = self._word_lists(word_ids)
        counts = np.zeros((self.K, n), dtype=np.int32)
        totals = np.zeros((self.K, n), dtype=np.int64)
        shares = np.zeros((self.K, n), dtype=np.float64)
        sumsq = np.zeros(self.K, dtype=np.uint64)
        capi.check(self._L.lda_topic_word_stats(self._h, n, ids.ctypes.data, counts.ctypes.data, totals.ctypes.data,
                                                shares.ctypes.data, sumsq.ctypes.data), "lda_topic_word_stats")
        return counts, totals, shares, sumsq

    def word_cooccurrences(self, word_ids, window: int = 0, doc_off=None, words=None):
        """lda_word_cooccurrences: units of a corpus that hold two listed
        words, whatever their topics.  word_ids[K, n] (-1 = empty slot).
        window 0: every non-empty document is a unit; window W >= 1: the
        max(1, L - W + 1) ranges of W tokens of a document of L tokens.
        doc_off None: this shard's training documents; else a host corpus
        (doc_off[Dh + 1], words with ids in [-1, V), -1 matching nothing).
        Returns (cooc[K, n (n + 1) / 2] int64, each topic's packed lower
        triangle, cell (i, j), j <= i, at i (i + 1) / 2 + j; units).  It reads
        neither z nor the counts, so it may run between sample and apply."""
        ids, n = self._word_lists(word_ids)
        if not 0 <= int(window) <= capi.COOC_WINDOW_MAX:
            raise ValueError(f"window must be in [0, {capi.COOC_WINDOW_MAX}]")
        off = w = None
        Dh = 0
        if doc_off is not None:
            off = np.ascontiguousarray(doc_off, dtype=np.int64).reshape(-1)
            if len(off) < 1:
                raise ValueError("doc_off must hold Dh + 1 offsets")
            Dh = len(off) - 1
            w = np.ascontiguousarray(words if words is not None else [], dtype=np.int32).reshape(-1)
            if len(w) < off[-1] - off[0]:
                raise ValueError("words is shorter than doc_off says")
        cooc = np.zeros((self.K, n * (n + 1) // 2), dtype=np.int64)
        units = C.c_int64(0)
        capi.check(self._L.lda_word_cooccurrences(self._h, n, ids.ctypes.data, int(window), Dh,
                                                  off.ctypes.data if off is not None else None,
                                                  w.ctypes.data if w is not None and len(w) else None,
                                                  cooc.ctypes.data, C.addressof(units)), "lda_word_cooccurrences")
        return cooc, int(units.value)

    def _other_sampler(self, other):
        """The native handle of the other side of a topic comparison (None:
        this sampler), checked before any native call."""
        if other is None or other is self:
            return None, self.K
        if not isinstance(other, GibbsSampler):
            raise ValueError(f"other must be a GibbsSampler or None, not {type(other).__name__}")
        if other.V != self.V:
            raise ValueError(f"other holds {other.V} word types, this sampler {self.V}")
        return other._h, other.K

    def topic_distances(self, metric="jensen_shannon", other=None) -> np.ndarray:
        """lda_topic_distances: the float64 (K, K2) matrix of a distance between
        the smoothed topics phi_k(w) = (nw[w, k] + beta) / (nwsum[k] + V beta)
        of this sampler (rows) and of `other` (columns; None: this sampler,
        K2 = K), computed on the device.  metric: "cosine" (a similarity),
        "hellinger", "jensen_shannon" (nats) or "kullback_leibler"
        (KL(row || column)), or the LDA_TOPIC_* integer.  Each side uses its own
        beta; both must hold the same V, and word ids must mean the same words
        on both sides: aligning vocabularies is the caller's job."""
        m = capi.topic_metric(metric)
        oh, K2 = self._other_sampler(other)
        out = np.zeros((self.K, K2), dtype=np.float64)
        capi.check(self._L.lda_topic_distances(self._h, oh, m, out.ctypes.data), "lda_topic_distances")
        return out

    def nearest_topics(self, n: int, metric="jensen_shannon", other=None):
        """lda_topic_nearest: per topic of this sampler the n nearest topics of
        `other` (None: this sampler, the topic itself left out), selected on
        the device from topic_distances' matrix: value ascending (cosine:
        descending), equal values by ascending topic id.  Returns (topics
        int32 (K, n), values float64 (K, n)); slots past the last candidate
        hold -1 / NaN."""
        n = capi.topic_nearest_n(n)
        m = capi.topic_metric(metric)
        oh, _ = self._other_sampler(other)
        topics = np.zeros((self.K, n), dtype=np.int32)
        values = np.zeros((self.K, n), dtype=np.float64)
        capi.check(self._L.lda_topic_nearest(self._h, oh, m, n, topics.ctypes.data, values.ctypes.data),
                   "lda_topic_nearest")
        return topics, values

    def doc_distances(self, metric, theta=None, counts=None, docs=None, doc_begin: int = 0,
                      num_docs: int | None = None) -> np.ndarray:
        """lda_doc_distances: the float64 (Q, M) matrix of a metric ("cosine",
        a similarity; "hellinger"; "jensen_shannon", nats; or the integer)
        between query rows and the topic distributions p_d = (n_dk + alpha_k) /
        (L_d + A) of this shard's documents, computed on the device from z.
        Queries: theta[Q, K] used as given, or counts[Q, K] (int32) turned into
        (c_k + alpha_k) / (sum c + A) on the device -- exactly one of them.
        docs as score_docs takes them."""
        m = capi.doc_metric(metric)
        theta, counts = capi.doc_queries(theta, counts, self.K)
        q = theta if theta is not None else counts
        begin, M, ids = self._doc_list(docs, doc_begin, num_docs)
        out = np.zeros((len(q), max(M, 0)), dtype=np.float64)
        capi.check(self._L.lda_doc_distances(self._h, m, len(q), theta.ctypes.data if theta is not None else None,
                                             counts.ctypes.data if counts is not None else None, begin, M,
                                             ids.ctypes.data if ids is not None and M else None, out.ctypes.data),
                   "lda_doc_distances")
        return out

    def nearest_docs(self, n: int, metric="hellinger", theta=None, counts=None, skip=None, min_tokens: int = 1):
        """lda_doc_nearest: per query row (theta or counts, as doc_distances
        takes them) the n nearest of this shard's documents with at least
        min_tokens tokens, selected on the device: value ascending (cosine:
        descending), equal values by ascending document id.  skip[Q] names a
        document each query leaves out (-1: none).  Returns (docs int64 (Q, n),
        values float64 (Q, n)); slots past the last candidate hold -1 / NaN."""
        n = capi.doc_nearest_n(n)
        m = capi.doc_metric(metric)
        theta, counts = capi.doc_queries(theta, counts, self.K)
        q = theta if theta is not None else counts
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, dtype=np.int64).reshape(-1)
            if len(sk) != len(q):
                raise ValueError(f"skip must hold one id per query ({len(q)}), not {len(sk)}")
        ids = np.zeros((len(q), n), dtype=np.int64)
        values = np.zeros((len(q), n), dtype=np.float64)
        capi.check(self._L.lda_doc_nearest(self._h, m, n, len(q), theta.ctypes.data if theta is not None else None,
                                           counts.ctypes.data if counts is not None else None,
                                           sk.ctypes.data if sk is not None and len(sk) else None, int(min_tokens),
                                           ids.ctypes.data, values.ctypes.data), "lda_doc_nearest")
        return ids, values

    def doc_neighbors(self, n: int, metric="hellinger", docs=None, min_tokens: int = 1):
        """lda_doc_neighbors: per listed document of this shard (None: all) its
        n nearest other documents with at least min_tokens tokens; the query
        rows are built on the device from z.  Bit-identical to doc_counts
        followed by nearest_docs(counts=..., skip=own id).  Returns (docs int64
        (M, n), values float64 (M, n))."""
        n = capi.doc_nearest_n(n)
        m = capi.doc_metric(metric)
        begin, M, ids = self._doc_list(docs, 0, None)
        out = np.zeros((M, n), dtype=np.int64)
        values = np.zeros((M, n), dtype=np.float64)
        capi.check(self._L.lda_doc_neighbors(self._h, m, n, begin, M, ids.ctypes.data if ids is not None and M else None,
                                             int(min_tokens), out.ctypes.data, values.ctypes.data),
                   "lda_doc_neighbors")
        return out, values

    def heldout_loglik(self, theta, doc_off, words):
        """lda_heldout_loglik: the log likelihood of the scored tokens of Dh
        held-out documents (doc_off[Dh + 1], words) under their topic
        distributions theta[Dh, K] and the model's current counts, computed on
        the device.  Returns (doc_ll[Dh], total) with total == sum of doc_ll
        added in order."""
        theta = capi.as_theta(theta, self.K)
        off, w = capi.as_docs(doc_off, words, len(theta))
        doc_ll = np.zeros(len(theta), dtype=np.float64)
        total = C.c_double(0.0)
        capi.check(self._L.lda_heldout_loglik(self._h, len(theta), theta.ctypes.data, off.ctypes.data,
                                              w.ctypes.data if len(w) else None, doc_ll.ctypes.data,
                                              C.addressof(total)), "lda_heldout_loglik")
        return doc_ll, total.value

    def doc_completion(self, obs_off, obs_words, sc_off, sc_words, n_iter: int = 100, thin: int = 10,
                       burn_in: int = 10, seed: int = 0, return_theta: bool = False):
        """lda_doc_completion: infer() on the observed halves, then
        heldout_loglik() of the result on the scored halves, in one native
        call.  Returns (doc_ll[Dh], total), and theta[Dh, K] (what infer()
        gives for the same arguments) as a third value with return_theta."""
        ooff, ow = capi.as_docs(obs_off, obs_words, what="obs_off")
        Dh = len(ooff) - 1
        soff, sw = capi.as_docs(sc_off, sc_words, Dh, what="sc_off")
        doc_ll = np.zeros(Dh, dtype=np.float64)
        theta = np.zeros((Dh, self.K), dtype=np.float64) if return_theta else None
        total = C.c_double(0.0)
        capi.check(self._L.lda_doc_completion(
            self._h, Dh, ooff.ctypes.data, ow.ctypes.data if len(ow) else None, soff.ctypes.data,
            sw.ctypes.data if len(sw) else None, int(n_iter), int(thin), int(burn_in),
            int(seed) & (2**64 - 1), doc_ll.ctypes.data, C.addressof(total),
            theta.ctypes.data if return_theta else None), "lda_doc_completion")
        return (doc_ll, total.value, theta) if return_theta else (doc_ll, total.value)

    def left_to_right(self, doc_off, words, particles: int = 10, resampling: bool = True, seed: int = 0,
                      token_prob: bool = False, z: bool = False):
        """lda_left_to_right: Mallet's MarginalProbEstimator.evaluateLeftToRight
        (Wallach et al.'s left-to-right particle estimator of log p(w | model))
        of Dh held-out documents (doc_off[Dh + 1], words, ids in [0, V)) against
        the model's current counts, on the device.  Returns (doc_ll[Dh], total,
        tokens_scored), then with token_prob the per-token estimate phat[N] (0
        for a skipped token) and with z each particle's final topics
        [particles, N] (-1 for a skipped token)."""
        off, w = capi.as_docs(doc_off, words)
        particles = int(particles)
        if particles < 1:
            raise ValueError("particles must be at least 1")
        Dh, N = len(off) - 1, len(w)
        doc_ll = np.zeros(Dh, dtype=np.float64)
        total, tokens = C.c_double(0.0), C.c_int64(0)
        tp = np.zeros(N, dtype=np.float64) if token_prob else None
        zo = np.full((particles, N), -1, dtype=np.int32) if z else None
        capi.check(self._L.lda_left_to_right(
            self._h, Dh, off.ctypes.data, w.ctypes.data if N else None, particles, 1 if resampling else 0,
            int(seed) & (2**64 - 1), doc_ll.ctypes.data, C.addressof(total), C.addressof(tokens),
            tp.ctypes.data if token_prob else None, zo.ctypes.data if z else None), "lda_left_to_right")
        out = (doc_ll, total.value, tokens.value)
        if token_prob:
            out += (tp,)
        if z:
            out += (zo,)
        return out

    # ------------------------------------------- hyperparameter statistics
    def max_doc_length(self) -> int:
        m = C.c_int32()
        capi.check(self._L.lda_max_doc_length(self._h, C.byref(m)), "lda_max_doc_length")
        return m.value

    def doc_topic_histograms(self, doc_len_counts=None, topic_doc_counts=None, max_len=None):
        """Add this shard's (docLengthCounts, topicDocCounts) from the current z
        into the given int32 arrays (allocated when None) and return them."""
        if max_len is None:
            max_len = self.max_doc_length() if doc_len_counts is None else len(doc_len_counts) - 1
        if doc_len_counts is None:
            doc_len_counts = np.zeros(max_len + 1, dtype=np.int32)
        if topic_doc_counts is None:
            topic_doc_counts = np.zeros((self.K, max_len + 1), dtype=np.int32)
        assert doc_len_counts.dtype == np.int32 and topic_doc_counts.dtype == np.int32
        assert doc_len_counts.shape == (max_len + 1,) and topic_doc_counts.shape == (self.K, max_len + 1)
        capi.check(self._L.lda_doc_topic_histograms(self._h, int(max_len), doc_len_counts,
                                                    topic_doc_counts), "lda_doc_topic_histograms")
        return doc_len_counts, topic_doc_counts

    def count_histogram(self, max_count: int, out=None):
        """optimizeBeta's countHistogram of the global nw (added into `out`)."""
        if out is None:
            out = np.zeros(int(max_count) + 1, dtype=np.int32)
        assert out.dtype == np.int32 and len(out) == int(max_count) + 1
        capi.check(self._L.lda_count_histogram(self._h, int(max_count), out), "lda_count_histogram")
        return out

    def row_stats(self) -> float:
        """Token-weighted mean nonzeros per word row of the snapshot."""
        v = C.c_double()
        capi.check(self._L.lda_row_stats(self._h, C.byref(v)), "lda_row_stats")
        return v.value

    def mallet_packed(self):
        """typeTopicCounts in Mallet's packed layout: (rows, row_off, topic_bits)."""
        row_off = np.zeros(self.V + 1, dtype=np.int64)
        bits = C.c_int32()
        capi.check(self._L.lda_to_mallet_packed(self._h, None, row_off, C.byref(bits)),
                   "lda_to_mallet_packed")
        rows = np.zeros(int(row_off[-1]), dtype=np.int32)
        capi.check(self._L.lda_to_mallet_packed(self._h, rows.ctypes.data if len(rows) else None,
                                                row_off, C.byref(bits)), "lda_to_mallet_packed")
        return rows, row_off, bits.value
