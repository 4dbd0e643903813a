/*
 * lda_topic_model.h — C ABI of the native host mirror of Mallet 2.0.7's
 * ParallelTopicModel / TopicInferencer, built on the sampler ABI in
 * lda_mi355x.h (liblda_topic_model.so, C++: ldagibbssampling_amd/host/).
 *
 * The reference drives Mallet through exactly this surface
 * (src/cmu_ron/TrainAndPredict.java:159-177, 230-234, 108-156;
 * src/cmu/TrainAndPredict.java:93-114, 258-274, 436):
 *   new ParallelTopicModel(K, alphaSum, beta)     -> ldatm_create
 *   addInstances(InstanceList)                    -> ldatm_set_alphabet + ldatm_add_instances
 *   setOptimizeInterval / setNumThreads /
 *   setNumIterations / setTopicDisplay            -> ldatm_set_*
 *   estimate()                                    -> ldatm_estimate
 *   modelLogLikelihood()                          -> ldatm_model_log_likelihood
 *   getTopicProbabilities(topicSequence)          -> ldatm_get_topic_probabilities
 *   printDocumentTopics(File)                     -> ldatm_print_document_topics
 *   printTopWords(File, n, newLines)              -> ldatm_print_top_words
 *   printTopicDocuments(File, max)                -> ldatm_print_topic_documents
 *   topicPhraseXMLReport's phrases, as text       -> ldatm_print_topic_phrases
 *   getInferencer().getSampledDistribution(...)   -> ldatm_infer
 *   the predict loop's similarity to every
 *   training document (Predictor.predict)        -> ldatm_score / ldatm_score_theta / ldatm_score_top
 *   the same question for cosine, Hellinger and
 *   Jensen-Shannon with the nearest documents
 *   selected on the device                       -> ldatm_document_distances / ldatm_nearest_documents /
 *                                                   ldatm_document_neighbors / ldatm_print_document_neighbors
 *   held-out log likelihood / perplexity by
 *   document completion, and its trace
 *   during estimate()                            -> ldatm_evaluate / ldatm_heldout_loglik / ldatm_set_held_out
 *   getProbEstimator().evaluateLeftToRight(...)   -> ldatm_left_to_right
 * Word ids index the model's alphabet (Mallet's Alphabet: insertion order).
 * Errors: lda_status codes of lda_mi355x.h, message in ldatm_last_error().
 */
#ifndef LDA_TOPIC_MODEL_H
#define LDA_TOPIC_MODEL_H

#include <stddef.h>
#include <stdint.h>

#include "lda_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ldatm ldatm;

/* ParallelTopicModel(numberOfTopics, alphaSum, beta): alpha_k = alphaSum/K. */
lda_status ldatm_create(ldatm** out, int32_t num_topics, double alpha_sum, double beta);
void ldatm_destroy(ldatm* m);

/* The InstanceList's data alphabet (UTF-8 words, index = word id).  words may
 * be NULL: ids only (top-words output then prints the ids).  Growing the
 * alphabet between addInstances calls is allowed (updateModel). */
lda_status ldatm_set_alphabet(ldatm* m, int32_t num_types, const char* const* words);
/* addInstances: D documents (doc_off[D+1], words[...] word ids < num_types of
 * the alphabet), sources[D] (Instance.getSource(), NULL or NULL entries ->
 * "null-source").  New documents get random topics (Philox, keyed by the
 * global token index); documents already added keep theirs. */
lda_status ldatm_add_instances(ldatm* m, int64_t D, const int64_t* doc_off, const int32_t* words,
                               const char* const* sources);

lda_status ldatm_set_num_iterations(ldatm* m, int32_t n);      /* setNumIterations   */
lda_status ldatm_set_optimize_interval(ldatm* m, int32_t n);   /* setOptimizeInterval */
lda_status ldatm_set_burnin_period(ldatm* m, int32_t n);       /* setBurninPeriod (200) */
lda_status ldatm_set_save_sample_interval(ldatm* m, int32_t n);/* saveSampleInterval (10) */
lda_status ldatm_set_symmetric_alpha(ldatm* m, int32_t on);    /* setSymmetricAlpha  */
lda_status ldatm_set_topic_display(ldatm* m, int32_t interval, int32_t n); /* setTopicDisplay */
lda_status ldatm_set_random_seed(ldatm* m, int64_t seed);      /* setRandomSeed      */
/* setNumThreads: Mallet's document blocks.  Here a block is a GPU shard:
 * ldatm_plan_shards(n, visible devices, corpus) GPUs -- at most n and the
 * devices, and ONE when the sweep is too short to pay for the exchange (the
 * reference's own ~16k-token corpus with setNumThreads(4)) -- with an RCCL
 * all-reduce of the exchange buffer between them.  Results do not depend on
 * it (integer sums, global Philox counters). */
lda_status ldatm_set_num_threads(ldatm* m, int32_t n);
/* The shard plan of setNumThreads (host-only): min(num_threads, num_devices,
 * num_docs) shards, reduced while (1 - 1/G) of the estimated sweep time
 * (num_tokens x (2 Kp + 16) bytes at 5 TB/s) does not exceed the estimated
 * ring all-reduce of 4 (V Kp + Kp) bytes (100 GB/s per link + 100 us). */
int32_t ldatm_plan_shards(int32_t num_threads, int32_t num_devices, int64_t num_tokens,
                          int32_t num_types, int32_t num_topics, int64_t num_docs);
/* Explicit shard placement: n shards, shard g on HIP device devices[g]
 * (n = 0: back to setNumThreads' plan).  Shards on distinct devices exchange
 * through RCCL; shards that ALL share one device exchange through a
 * device-side sum with the same streams, events and apply ordering (the
 * multi-shard path on a one-GPU box).  Other mixes: LDA_ERR_UNSUPPORTED. */
lda_status ldatm_set_devices(ldatm* m, int32_t n, const int32_t* devices);
/* Shards the next estimate() runs on (creates them if needed). */
lda_status ldatm_num_shards(ldatm* m, int32_t* shards);
/* The shards' compact exchange (lda_exchange_pack; creates the shards if
 * needed): cells per packed word (lda_set_exchange_cells: 4 for K > 1024 up
 * to 64 shards, else 2; 0 when the shards do not exchange packed words --
 * one shard, or shards on one device without LDA_LOCAL_COMPACT=1), whether
 * the escape lists travel at their used length (1, the default: the counts
 * are read on the host behind each pack, overlapping the packed words'
 * all-reduce) or whole (0, LDA_ESCAPE_LISTS=capacity), the largest per-shard
 * escape count gathered so far and the number of count reads.  Any pointer
 * may be NULL. */
lda_status ldatm_exchange_info(ldatm* m, int32_t* cells_per_word, int32_t* used_lists, int32_t* escapes_max,
                               int64_t* list_exchanges);
/* LDA_SAMPLER_* (default: DENSE for K <= 1024, SPARSE above) */
lda_status ldatm_set_sampler(ldatm* m, int32_t sampler);
/* With more than one GPU shard: cut every sweep into `parts` parts
 * (1..LDA_MAX_EXCHANGE_PARTS) whose all-reduces overlap the next part's
 * sampling (lda_set_exchange_parts).  No effect on one GPU or on results. */
lda_status ldatm_set_exchange_parts(ldatm* m, int32_t parts);
/* Warm start (lda_set_warm_start): sweeps 0 .. sweeps-1 of the model's sweep
 * counter run in `parts` sequential parts, so that the early sweeps see part
 * of their own changes as Mallet's worker threads do.  Default 4 parts x 50
 * sweeps (held-out perplexity at K = 20 over 48 seeds: 10 / 48 seeds in a
 * worse local optimum instead of 18 / 48; cpu_mallet 16 / 48).
 * (1, 0) turns it off.  Carried by checkpoints and by the sweep counter. */
lda_status ldatm_set_warm_start(ldatm* m, int32_t parts, int32_t sweeps);
/* Sweeps past the warm start show each token the share of the sweep's other
 * changes that Mallet's T worker threads would (lda_set_sequential_sweeps /
 * lda_staleness_schedule): threads = 0 (the default) takes T
 * from ldatm_set_num_threads (the reference's setNumThreads(4)), threads > 0
 * sets T, threads < 0 runs plain snapshot sweeps.  Without it the learned
 * hyperparameters drift from Mallet's at the reference's settings (beta
 * ~9% high, alphaSum ~4% low) and K = 500 traps more chains.  Carried by
 * checkpoints (files before format v3 continue with snapshot sweeps). */
lda_status ldatm_set_staleness_threads(ldatm* m, int32_t threads);
/* State a Java-side ParallelTopicModel already holds, for GpuParallelTopicModel
 * (integration/): the topics Mallet's own addInstances drew (z[n], n = every
 * token of the model), alpha[K] / alphaSum / beta after an earlier optimisation,
 * and the Philox sweep counter, which must continue across estimate() calls
 * (updateModel, src/cmu_ron/TrainAndPredict.java:173-177) so that a second
 * estimate() does not replay the first one's uniforms. */
lda_status ldatm_set_topics(ldatm* m, int64_t n, const int32_t* z);
lda_status ldatm_set_hyper(ldatm* m, const double* alpha, double alpha_sum, double beta);
lda_status ldatm_get_sweep(ldatm* m, uint32_t* sweep);
lda_status ldatm_set_sweep(ldatm* m, uint32_t sweep);
/* printLogLikelihood / logging: 0 = silent, 1 = Mallet's INFO lines on stderr */
lda_status ldatm_set_verbosity(ldatm* m, int32_t level);
lda_status ldatm_set_print_log_likelihood(ldatm* m, int32_t on);

/* estimate(): numIterations sweeps; statistics every saveSampleInterval and
 * optimizeAlpha/optimizeBeta every optimizeInterval sweeps after the burn-in;
 * LL/token every 10 sweeps (kept in the trace below). */
lda_status ldatm_estimate(ldatm* m);
/* (iteration, LL/token) pairs of the last estimate(): n = number available;
 * copies min(cap, n). */
lda_status ldatm_get_ll_trace(ldatm* m, int32_t* iterations, double* ll_per_token, int32_t cap,
                              int32_t* n);

lda_status ldatm_model_log_likelihood(ldatm* m, double* out);
lda_status ldatm_get_shape(ldatm* m, int32_t* K, int32_t* V, int64_t* D, int64_t* N);
lda_status ldatm_get_hyper(ldatm* m, double* alpha /*[K]*/, double* alpha_sum, double* beta);
lda_status ldatm_get_z(ldatm* m, int32_t* z /*[N]*/);
lda_status ldatm_get_counts(ldatm* m, int32_t* nw /*[V*K] or NULL*/, int32_t* nwsum /*[K]*/);
/* getTopicProbabilities(doc): (n_dk + alpha_k) / sum_k (n_dk + alpha_k). */
lda_status ldatm_get_topic_probabilities(ldatm* m, int64_t doc, double* out /*[K]*/);

/* The readouts of a trained model, selected on the device (lda_top_words,
 * lda_doc_top_topics, lda_doc_counts of lda_mi355x.h): no V x K
 * table and no copy of the topic assignments crosses to the host.
 *
 * ldatm_top_words: per topic k < K the n words with the largest count, count
 * descending, equal counts by ascending word id (displayTopWords' order);
 * word_ids[K*n] and counts[K*n], slots past a topic's last nonzero word -1 and
 * 0.  Runs on shard 0: every shard holds the same global counts, so the result
 * does not depend on the number of shards, bit for bit.
 * Errors: LDA_ERR_INVALID_ARG for a NULL model or output, or n outside
 * [1, LDA_TOP_WORDS_MAX] (checked before any device work).  Scratch as
 * lda_top_words.  Waits for shard 0's stream. */
lda_status ldatm_top_words(ldatm* m, int32_t n, int32_t* word_ids /*[K*n]*/, int32_t* counts /*[K*n]*/);
/* ldatm_doc_top_topics: for the global document ids docs[M] (any order,
 * duplicates allowed), or docs == NULL: all documents, M = the model's D, the
 * mtop topics with the largest weight (alpha_k + n_dk) / (n_d + alphaSum),
 * equal weights by ascending topic id; topics[M*mtop] and the topics' counts
 * counts[M*mtop], slots past K -1 and 0.  alphaSum is the sum of the model's
 * alpha added in topic order (lda_doc_top_topics), which is what
 * ldatm_get_hyper reports after an optimisation; see documentTopics in DESIGN
 * 9d for a model whose alpha_sum holds other bits.
 * ldatm_doc_counts: the same documents' dense count rows nd[M*K].
 * Both map the global ids onto the shards' document ranges as
 * ldatm_score_theta does; each shard answers for its own documents on its own
 * device and the rows are scattered back into the caller's order.  A
 * document's row depends on that document alone: not on M, the list or the
 * number of shards, bit for bit.
 * Errors: LDA_ERR_INVALID_ARG for a NULL model, mtop outside
 * [1, LDA_TOP_TOPICS_MAX], M < 0, a document id outside [0, D), M != D without
 * a list, or a NULL output with M > 0.  M = 0 succeeds and touches nothing.
 * Device scratch per shard as the lda_ calls bound it; the host holds one
 * shard's rows while it scatters them.  Waits for the shards' streams. */
lda_status ldatm_doc_top_topics(ldatm* m, int32_t mtop, int64_t M, const int64_t* docs,
                                int32_t* topics /*[M*mtop]*/, int32_t* counts /*[M*mtop]*/);
lda_status ldatm_doc_counts(ldatm* m, int64_t M, const int64_t* docs, int32_t* nd /*[M*K]*/);

/* Topic distances and nearest topics within one model or between two
 * (lda_topic_distances / lda_topic_nearest of lda_mi355x.h; the
 * metrics are LDA_TOPIC_COSINE, _HELLINGER, _JS, _KL as defined there).
 * other == NULL or other == m: the model against itself (K2 = K); else topic a
 * of m against topic b of other, each side with its own beta.  The two
 * models must hold the same num_types, and word ids must mean the same words
 * in both: aligning vocabularies is the caller's job.  Both calls run on
 * shard 0 of each model -- every shard holds the same global counts, so the
 * result does not depend on the number of shards, bit for bit.
 * ldatm_topic_distances: out[K*K2], row a = topic a of m.
 * ldatm_nearest_topics: per topic a of m the n nearest topics of other,
 * value ascending (cosine: descending), ties by ascending topic id, the topic
 * itself left out when the model is compared with itself; topics[K*n],
 * values[K*n]; id -1 and NaN past the last candidate.
 * Errors, checked in this order before any device work (a model without a
 * GPU names its bad argument, not the missing device): LDA_ERR_INVALID_ARG for
 * a NULL model, a metric outside [0, 3], n outside [1, LDA_TOPIC_NEAREST_MAX],
 * a NULL output, num_types differing.  When shard 0 of the two models sit on
 * different devices, lda_topic_distances' LDA_ERR_UNSUPPORTED is passed on
 * with its message.  Waits for shard 0's streams. */
lda_status ldatm_topic_distances(ldatm* m, ldatm* other /* NULL = m */, int32_t metric, double* out /*[K*K2]*/);
lda_status ldatm_nearest_topics(ldatm* m, ldatm* other /* NULL = m */, int32_t metric, int32_t n,
                                int32_t* topics /*[K*n]*/, double* values /*[K*n]*/);

/* Nearest documents (lda_doc_distances / lda_doc_nearest / lda_doc_neighbors
 * of lda_mi355x.h, DESIGN 9n: the rows, the metrics LDA_TOPIC_COSINE,
 * _HELLINGER, _JS, the selection order and the determinism contract are
 * stated there).  Document ids are GLOBAL; queries are theta[Q*K] or
 * counts[Q*K], exactly one of them.
 * ldatm_document_distances: out[Q*M] against docs[M] (NULL: every document,
 * M = the number of documents), routed to the shards as ldatm_score_theta
 * routes.
 * ldatm_nearest_documents: per query the n nearest of all documents with at
 * least min_tokens tokens, document skip[q] left out (-1 or skip NULL: none);
 * doc_ids[Q*n], values[Q*n], -1 / NaN past the last candidate.  Every shard
 * selects among its own documents and the host merges the shards' lists by
 * (value, global id): the result does not depend on the number of shards, bit
 * for bit.
 * ldatm_document_neighbors: the queries are the model's own documents docs[M]
 * (NULL: all, M = the number of documents), each left out of its own list;
 * doc_ids[M*n], values[M*n].  Neither theta nor counts cross to the host with
 * one shard; with several, the counts of a chunk of queries do.  The same
 * bits either way.
 * ldatm_print_document_neighbors / ldatm_document_neighbors_text: the
 * neighbours of every document as text, "#doc neighbor name value\n", then
 * "<doc> <neighbor> <source|null-source of the neighbour> <value>\n" per
 * document and rank, Java Double.toString values; empty slots print nothing.
 * ldatm_document_neighbors_format: that text from the caller's M x n arrays
 * (host only; docs NULL: the query of row j is j; names as
 * ldatm_topic_documents_format).
 * Errors, checked in this order before any device work (a model without a
 * GPU names its bad argument): LDA_ERR_INVALID_ARG for a NULL model, a metric
 * outside [0, 2], n outside [1, LDA_DOC_NEAREST_MAX], both or neither of
 * theta / counts, a NULL output with work to do, Q < 0 or M < 0, M not the
 * number of documents without a list, a document id outside [0, D),
 * min_tokens < 1, a skip id outside [-1, D), a bad theta row, a negative
 * count. */
lda_status ldatm_document_distances(ldatm* m, int32_t metric, int64_t Q, const double* theta /*[Q*K] or NULL*/,
                                    const int32_t* counts /*[Q*K] or NULL*/, int64_t M, const int64_t* docs,
                                    double* out /*[Q*M]*/);
lda_status ldatm_nearest_documents(ldatm* m, int32_t metric, int32_t n, int64_t Q, const double* theta,
                                   const int32_t* counts, const int64_t* skip /*[Q] or NULL*/, int32_t min_tokens,
                                   int64_t* doc_ids /*[Q*n]*/, double* values /*[Q*n]*/);
lda_status ldatm_document_neighbors(ldatm* m, int32_t metric, int32_t n, int64_t M, const int64_t* docs,
                                    int32_t min_tokens, int64_t* doc_ids /*[M*n]*/, double* values /*[M*n]*/);
lda_status ldatm_document_neighbors_text(ldatm* m, int32_t n, int32_t metric, int32_t min_tokens, char* buf,
                                         size_t cap, size_t* len);
lda_status ldatm_print_document_neighbors(ldatm* m, const char* path, int32_t n, int32_t metric,
                                          int32_t min_tokens);
lda_status ldatm_document_neighbors_format(int64_t M, int32_t n, const int64_t* docs, const int64_t* doc_ids,
                                           const double* values, const char* const* names, int64_t num_names,
                                           char* buf, size_t cap, size_t* len);

/* Topic diagnostics: per topic the figures Mallet's
 * TopicModelDiagnostics reports (train-topics --diagnostics-file), from
 * integer statistics counted on the device (lda_topic_codocuments,
 * lda_topic_word_stats, lda_doc_topic_histograms); no copy of z and no V x K
 * table crosses to the host.  The definitions are written after Mallet's and
 * are stated here in full; they are not pinned against Mallet itself.
 *
 * ldatm_topic_codocuments: lda_topic_codocuments on every shard with the
 * caller's lists word_ids[K*n] (-1 = empty slot) and thresholds props[P],
 * summed in int64: codoc[K * n(n+1)/2] (cell (i, j), j <= i, of a topic at
 * i(i+1)/2 + j) and doc_stats[K * (2 + P)].  Integer sums: the result does not
 * depend on the number of shards, bit for bit.
 * Errors (checked before any device work, against the model's K and V):
 * LDA_ERR_INVALID_ARG for a NULL model, word_ids, props (P > 0) or output, n
 * outside [1, LDA_DIAG_WORDS_MAX], an id outside [-1, V), the same id twice in
 * one topic's list, P outside [0, LDA_DIAG_PROPS_MAX], props not strictly
 * ascending in (0, 1].
 *
 * ldatm_topic_statistics: ldatm_top_words(n) and lda_topic_word_stats on
 * shard 0 (word_ids, counts, totals, share_sums [K*n], sumsq [K], all
 * outputs), then ldatm_topic_codocuments with those lists and Mallet's
 * LDATM_DIAG_PROPS = 7 proportions {0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5}
 * (doc_stats [K * 9]).
 *
 * ldatm_diagnostics_finish: host only, no model and no device.  From K, V, n,
 * beta, nwsum[K], the summed topicDocCounts topic_doc_counts[K*(max_len+1)]
 * (row k, cell c: documents in which topic k has count c; lda_doc_topic_
 * histograms) and the statistics above it writes out[K * LDATM_DIAG_COLUMNS],
 * column c of topic k at out[k * LDATM_DIAG_COLUMNS + c].  With T = nwsum[k],
 * N = sum of nwsum, D_k = doc_stats[k][0], the topic's m non-empty slots in
 * list order (c_i, t_i, s_i their counts, totals, share_sums; C its triangle,
 * H its histogram row), natural logarithms, a ratio with a zero denominator
 * and a term x log(..) with x = 0 both 0, and every column 0 when T = 0:
 *   TOKENS            T
 *   DOCUMENT_ENTROPY  log T - (sum_{c=1..max_len} H[c] (c log c)) / T,
 *                     added in ascending c
 *   COHERENCE         sum_{i=1..m-1} sum_{j=0..i-1}
 *                     log((C[i,j] + beta) / (C[j,j] + beta)), i outer
 *   UNIFORM_DIST      sum_i p_i log(p_i V), p_i = c_i / T
 *   CORPUS_DIST       sum_i p_i log(p_i / (t_i / N))
 *   EFF_NUM_WORDS     T T / sumsq[k]
 *   TOKEN_DOC_DIFF    sum_i (p_i log(p_i / mu_i) + q_i log(q_i / mu_i)) / 2,
 *                     here p_i = c_i / sum_j c_j, q_i = C[i,i] / sum_j C[j,j],
 *                     mu_i = (p_i + q_i) / 2
 *   RANK_1_DOCS       doc_stats[k][1] / D_k
 *   ALLOCATION_RATIO  documents at 0.5 / documents at 0.02
 *   ALLOCATION_COUNT  documents at 0.3 / D_k
 *   EXCLUSIVITY       (1 / m) sum_i ((beta + c_i) / (V beta + T)) / s_i
 * LDA_ERR_INTERNAL when a topic's histogram row does not add up to D_k (the
 * two are counted by different kernels); LDA_ERR_INVALID_ARG for a NULL
 * argument or n outside [1, LDA_DIAG_WORDS_MAX].
 *
 * ldatm_topic_diagnostics: ldatm_topic_statistics, nwsum, the shards'
 * histograms of the current z and ldatm_diagnostics_finish; out
 * [K * LDATM_DIAG_COLUMNS], and the lists used in word_ids[K*n] unless NULL.
 * Errors: LDA_ERR_INVALID_ARG for a NULL model or out, or n out of range
 * (before any device work). */
#define LDATM_DIAG_PROPS 7
#define LDATM_DIAG_COLUMNS 11
#define LDATM_DIAG_TOKENS 0
#define LDATM_DIAG_DOCUMENT_ENTROPY 1
#define LDATM_DIAG_COHERENCE 2
#define LDATM_DIAG_UNIFORM_DIST 3
#define LDATM_DIAG_CORPUS_DIST 4
#define LDATM_DIAG_EFF_NUM_WORDS 5
#define LDATM_DIAG_TOKEN_DOC_DIFF 6
#define LDATM_DIAG_RANK_1_DOCS 7
#define LDATM_DIAG_ALLOCATION_RATIO 8
#define LDATM_DIAG_ALLOCATION_COUNT 9
#define LDATM_DIAG_EXCLUSIVITY 10
lda_status ldatm_topic_codocuments(ldatm* m, int32_t n, const int32_t* word_ids /*[K*n]*/, int32_t P,
                                   const double* props /*[P]*/, int64_t* codoc /*[K*n(n+1)/2]*/,
                                   int64_t* doc_stats /*[K*(2+P)]*/);
lda_status ldatm_topic_statistics(ldatm* m, int32_t n, int32_t* word_ids /*[K*n]*/, int32_t* counts /*[K*n]*/,
                                  int64_t* totals /*[K*n]*/, double* share_sums /*[K*n]*/, uint64_t* sumsq /*[K]*/,
                                  int64_t* codoc /*[K*n(n+1)/2]*/, int64_t* doc_stats /*[K*9]*/);
lda_status ldatm_diagnostics_finish(int32_t K, int32_t V, int32_t n, double beta, const int32_t* nwsum /*[K]*/,
                                    int32_t max_len, const int64_t* topic_doc_counts /*[K*(max_len+1)]*/,
                                    const int32_t* word_ids, const int32_t* counts, const int64_t* totals,
                                    const double* share_sums, const uint64_t* sumsq, const int64_t* codoc,
                                    const int64_t* doc_stats, double* out /*[K*LDATM_DIAG_COLUMNS]*/);
lda_status ldatm_topic_diagnostics(ldatm* m, int32_t n, double* out /*[K*LDATM_DIAG_COLUMNS]*/,
                                   int32_t* word_ids /*[K*n] or NULL*/);

/* Reference-corpus topic coherence: UMass (Mimno et al. 2011),
 * UCI / PMI (Newman et al. 2010) and NPMI (Lau et al. 2014) of each topic's
 * top words, by plain co-occurrence in a corpus -- whatever the tokens'
 * topics -- counted on the device (lda_word_cooccurrences).  The corpus is
 * the training corpus or any corpus over the same alphabet.
 *
 * ldatm_word_cooccurrences: lda_word_cooccurrences with the caller's lists
 * word_ids[K*n] (-1 = empty slot) and window (0 = documents are the units,
 * W >= 1 = sliding windows of W tokens).  doc_off == NULL: the training
 * corpus; every shard counts its own documents and the results are summed
 * (Dh and words are ignored).  Otherwise Dh documents in host memory, ids in
 * [-1, V) (-1 = a token outside the alphabet), counted by shard 0 alone.
 * cooc[K * n(n+1)/2] (cell (i, j), j <= i, of a topic at i(i+1)/2 + j) and
 * *units.  Integer sums: the result does not depend on the number of shards,
 * bit for bit.  It reads neither z nor the counts and leaves the model's
 * state untouched.
 * Errors (checked before any device work, against the model's K and V):
 * LDA_ERR_INVALID_ARG for a NULL model, word_ids, cooc or units, n outside
 * [1, LDA_DIAG_WORDS_MAX], an id outside [-1, V), the same id twice in one
 * topic's list, window outside [0, LDA_COOC_WINDOW_MAX], and with a host
 * corpus Dh < 0, a non-monotone doc_off, NULL words when there are tokens or
 * a token id outside [-1, V).
 *
 * ldatm_coherence_finish: host only, no model and no device.  From the
 * triangles cooc[K * n(n+1)/2] and N = units it writes, per topic, sums[k] =
 * the sum of the measure's term over the kept pairs and pairs[k] = their
 * number; the topic's coherence is sums[k] / pairs[k], and 0.0 when no pair is
 * kept.  With D(i) = the diagonal cell (i, i), D(i,j) = the cell (i, j), every
 * count converted to fp64, natural logarithms, the pairs (i, j), j < i, added
 * in fp64 with i ascending and then j ascending from 0.0, and a pair skipped
 * when D(i) = 0 or D(j) = 0 (an empty slot has D = 0):
 *   LDATM_COHERENCE_UMASS  log((D(i,j) + eps) / D(j));           default eps 1
 *   LDATM_COHERENCE_UCI    log((D(i,j) / N + eps) / ((D(i) / N) * (D(j) / N))),
 *                          also skipped when D(i,j) = N;     default eps 1e-12
 *   LDATM_COHERENCE_NPMI   the UCI term / (-log(D(i,j) / N + eps)), the same
 *                          skips and default
 * epsilon < 0 selects the measure's default.  N = 0 gives all zeros.
 * LDA_ERR_INVALID_ARG for K < 1, units < 0, n outside [1, LDA_DIAG_WORDS_MAX],
 * a measure outside [0, 2] or a NULL argument.
 *
 * ldatm_topic_coherence: ldatm_top_words(n) on the device, then
 * ldatm_word_cooccurrences with those lists, then ldatm_coherence_finish:
 * values[K] = sums / pairs (0.0 without a kept pair) and pairs[K]; the lists
 * in word_ids_out[K*n] and the counts in cooc_out[K * n(n+1)/2] unless NULL;
 * *units.  Errors: LDA_ERR_INVALID_ARG for a NULL model, values, pairs or
 * units, a measure, n or window out of range, or a bad host corpus as above
 * (all before any device work). */
#define LDATM_COHERENCE_UMASS 0
#define LDATM_COHERENCE_UCI 1
#define LDATM_COHERENCE_NPMI 2
lda_status ldatm_word_cooccurrences(ldatm* m, int32_t n, const int32_t* word_ids /*[K*n]*/, int32_t window,
                                    int64_t Dh, const int64_t* doc_off, const int32_t* words,
                                    int64_t* cooc /*[K*n(n+1)/2]*/, int64_t* units);
lda_status ldatm_coherence_finish(int32_t K, int32_t n, int32_t measure, double epsilon,
                                  const int64_t* cooc /*[K*n(n+1)/2]*/, int64_t units, double* sums /*[K]*/,
                                  int64_t* pairs /*[K]*/);
lda_status ldatm_topic_coherence(ldatm* m, int32_t measure, int32_t n, int32_t window,
                                 double epsilon /*<0 = the measure's default*/, int64_t Dh, const int64_t* doc_off,
                                 const int32_t* words, double* values /*[K]*/, int64_t* pairs /*[K]*/,
                                 int32_t* word_ids_out /*[K*n] or NULL*/, int64_t* cooc_out /*[K*n(n+1)/2] or NULL*/,
                                 int64_t* units);

/* printDocumentTopics(File) (threshold 0, max -1 = all) and its text:
 * "#doc source topic proportion ...", then per document
 * "<doc> <source|null-source> <topic> <weight> ... \n" (weights descending,
 * Java Double.toString).  printTopWords(File, numWords, usingNewLines):
 * displayTopWords text ("<topic>\t<alpha>\t<word> <word> ...\n").
 * The *_text variants write into buf (cap bytes incl. NUL) and report the
 * full length in *len (call with buf = NULL to size it). */
lda_status ldatm_print_document_topics(ldatm* m, const char* path, double threshold, int32_t max);
lda_status ldatm_document_topics_text(ldatm* m, double threshold, int32_t max, char* buf,
                                      size_t cap, size_t* len);
lda_status ldatm_print_top_words(ldatm* m, const char* path, int32_t num_words,
                                 int32_t using_new_lines);
lda_status ldatm_top_words_text(ldatm* m, int32_t num_words, int32_t using_new_lines, char* buf,
                                size_t cap, size_t* len);

/* The documents in which each topic is heaviest, selected on the device
 * (lda_topic_top_docs of lda_mi355x.h; the question Mallet's
 * printTopicDocuments answers, by this library's definition: only documents
 * with a token of the topic are candidates).
 * ldatm_topic_top_docs: per topic k < K the n documents with n_dk > 0 and
 * length >= min_tokens that have the largest weight
 *     ((double) n_dk + smoothing) / ((double) L_d + (double) K * smoothing),
 * weight descending, equal weights by ascending document id; GLOBAL document
 * ids in doc_ids[K*n], n_dk in counts[K*n], L_d in lengths[K*n]; -1 / 0 / 0
 * past a topic's last candidate.  Each shard selects among its own documents
 * on its own device and stream; the local ids become global through the
 * shards' document ranges and the host merges the shards' K x n lists by
 * (weight descending, id ascending), each weight recomputed from (count,
 * length) with the expression above.  A shard's list holds every one of its
 * documents that belongs to the global best n, so the result does not depend
 * on the number of shards, bit for bit.
 * Errors, checked before any device work (a model without a GPU names its bad
 * argument): LDA_ERR_INVALID_ARG for a NULL model, n outside
 * [1, LDA_TOPIC_DOCS_MAX], smoothing negative or not finite, min_tokens < 1,
 * or a NULL output.  Device scratch per shard as lda_topic_top_docs bounds
 * it; the host holds shards x K x n entries.  Waits for the shards' streams.
 * ldatm_print_topic_documents / ldatm_topic_documents_text: the selection
 * with n = max as text, "#topic doc name proportion ...\n", then per topic
 * and rank "<topic> <doc> <source|null-source> <weight>\n" (the name column
 * and Java Double.toString of ldatm_print_document_topics); padded slots
 * print nothing.  Same errors; buf / cap / len as the other *_text calls.
 * ldatm_topic_documents_format: that text from the caller's K x n arrays
 * (host only, no model and no device); names[num_names] gives the name column
 * (NULL entry or an id >= num_names: "null-source"). */
lda_status ldatm_topic_top_docs(ldatm* m, int32_t n, double smoothing, int32_t min_tokens,
                                int64_t* doc_ids /*[K*n]*/, int32_t* counts /*[K*n]*/, int32_t* lengths /*[K*n]*/);
lda_status ldatm_print_topic_documents(ldatm* m, const char* path, int32_t max, double smoothing,
                                       int32_t min_tokens);
lda_status ldatm_topic_documents_text(ldatm* m, int32_t max, double smoothing, int32_t min_tokens, char* buf,
                                      size_t cap, size_t* len);
lda_status ldatm_topic_documents_format(int32_t K, int32_t n, double smoothing, const int64_t* doc_ids,
                                        const int32_t* counts, const int32_t* lengths, const char* const* names,
                                        int64_t num_names, char* buf, size_t cap, size_t* len);

/* Topic co-occurrence in documents: which topics are used together
 * (lda_topic_cooccurrence of lda_mi355x.h; the question of
 * stm::topicCorr and jsLDA's topic correlations).
 * ldatm_topic_cooccurrence: lda_topic_cooccurrence's outputs summed over the
 * model's shards -- integer sums, so the result does not depend on the number
 * of shards.  A document is used with at least min_tokens tokens; topic k is
 * present in it with n_dk >= min_count and (double) n_dk >= min_prop *
 * (double) L_d.  *docs_used, tokens[K] (N_k), present[K] (C_k) are required;
 * codocs (C_kl), overlap (M_kl = sum of min(n_dk, n_dl)) and product (S_kl =
 * sum of n_dk n_dl), full symmetric K x K, are each counted only when the
 * pointer is not NULL.
 * ldatm_topic_correlation_finish (host only, no model and no device): a K x K
 * matrix of doubles from those integers, D' = docs_used:
 *   LDATM_CORR_PMI      codocs   log(D' C_kl / (C_k C_l))
 *   LDATM_CORR_NPMI     codocs   pmi / -log(C_kl / D')
 *   LDATM_CORR_JACCARD  codocs   C_kl / (C_k + C_l - C_kl)
 *   LDATM_CORR_OVERLAP  overlap  M_kl / (N_k + N_l - M_kl)
 *   LDATM_CORR_COSINE   product  S_kl / (sqrt(S_kk) sqrt(S_ll))
 *   LDATM_CORR_PEARSON  product  (D' S_kl - N_k N_l) /
 *                                sqrt((D' S_kk - N_k^2) (D' S_ll - N_l^2))
 * pmi is -inf when C_kl = 0 and NaN when C_k or C_l is 0; npmi is -1 when
 * C_kl = 0, 1 when C_kl = D', NaN when C_k or C_l is 0; the others are NaN
 * when a denominator term is 0.  Every integer becomes a double once, then one
 * rounding per operation; Pearson's three terms are formed exactly in 128-bit
 * integers before that one conversion, so the measure has no cancellation
 * error.  table_kind says which table `table` is (LDATM_COOC_*): one that is
 * not the measure's, or an unknown measure, is LDA_ERR_INVALID_ARG with a
 * message.
 * ldatm_topic_correlations: counts only the table the measure needs, then
 * finishes; out[K*K].
 * ldatm_topic_partners: per topic its n strongest other topics by that
 * matrix: larger value first, equal values by smaller id, non-finite values
 * left out; ids / values [K*n], -1 / NaN past the last partner (n > K - 1
 * always has such slots).  The selection is on the host from the K x K matrix
 * (ldatm_topic_partners_select, host only, does it from a given matrix).
 * ldatm_topic_correlations_text / ldatm_print_topic_correlations: the partners
 * as text, "#topic partner value\n", then "<topic> <partner> <value>\n" per
 * topic and rank (Java Double.toString, as ldatm_format_double style 0);
 * empty slots print nothing.  ldatm_topic_correlations_format: that text from
 * the caller's K x n arrays (host only).
 * Errors, checked before any device work (a model without a GPU names its bad
 * argument): LDA_ERR_INVALID_ARG for a NULL model, an unknown measure,
 * min_tokens < 1, min_count < 1, min_prop outside [0, 1] or NaN, n < 1, a NULL
 * output. */
#define LDATM_CORR_PMI 0
#define LDATM_CORR_NPMI 1
#define LDATM_CORR_JACCARD 2
#define LDATM_CORR_OVERLAP 3
#define LDATM_CORR_COSINE 4
#define LDATM_CORR_PEARSON 5
#define LDATM_COOC_CODOCS 0
#define LDATM_COOC_OVERLAP 1
#define LDATM_COOC_PRODUCT 2
lda_status ldatm_topic_cooccurrence(ldatm* m, int64_t min_tokens, int32_t min_count, double min_prop,
                                    int64_t* docs_used, int64_t* tokens /*[K]*/, int64_t* present /*[K]*/,
                                    int64_t* codocs /*[K*K] or NULL*/, int64_t* overlap /*[K*K] or NULL*/,
                                    int64_t* product /*[K*K] or NULL*/);
lda_status ldatm_topic_correlation_finish(int32_t measure, int32_t K, int64_t docs_used, const int64_t* tokens,
                                          const int64_t* present, int32_t table_kind, const int64_t* table,
                                          double* out /*[K*K]*/);
lda_status ldatm_topic_correlations(ldatm* m, int32_t measure, int64_t min_tokens, int32_t min_count,
                                    double min_prop, double* out /*[K*K]*/);
lda_status ldatm_topic_partners(ldatm* m, int32_t measure, int64_t min_tokens, int32_t min_count, double min_prop,
                                int32_t n, int32_t* ids /*[K*n]*/, double* values /*[K*n]*/);
lda_status ldatm_topic_partners_select(int32_t K, int32_t n, const double* matrix /*[K*K]*/, int32_t* ids /*[K*n]*/,
                                       double* values /*[K*n]*/);
lda_status ldatm_topic_correlations_text(ldatm* m, int32_t measure, int32_t n, int64_t min_tokens,
                                         int32_t min_count, double min_prop, char* buf, size_t cap, size_t* len);
lda_status ldatm_print_topic_correlations(ldatm* m, const char* path, int32_t measure, int32_t n,
                                          int64_t min_tokens, int32_t min_count, double min_prop);
lda_status ldatm_topic_correlations_format(int32_t K, int32_t n, const int32_t* ids, const double* values,
                                           char* buf, size_t cap, size_t* len);

/* Topics by document group: how the topics differ between groups of documents
 * (years, sources, labels), and a topic's top words inside a group only
 * (lda_group_topics and lda_subcorpus_* of lda_mi355x.h, which state the
 * definitions; the question of jsLDA's time series and of stm's
 * estimateEffect plots).
 * ldatm_group_topics: lda_group_topics' outputs summed over the model's shards
 * -- integer sums, so the result does not depend on the number of shards.
 * doc_group[D] holds a group id in [-1, G) for every document of the model in
 * its global order (-1 leaves the document out); each shard gets its slice.
 * group_docs[G], group_tokens[G] and tokens[G*K] are required; present[G*K]
 * and shares[G*K] are each counted only when the pointer is not NULL.
 * ldatm_group_prevalence_finish (host only, no model and no device): a G x K
 * matrix of doubles from those integers:
 *   LDATM_GROUP_TOKENS     tokens_gk / group_tokens_g
 *   LDATM_GROUP_DOCUMENTS  present_gk / group_docs_g           (needs present)
 *   LDATM_GROUP_MEAN       shares_gk / (2^32 * group_docs_g)   (needs shares)
 *   LDATM_GROUP_LIFT       log((tokens_gk / group_tokens_g) / (N_k / N)),
 *                          N_k = sum over g of tokens_gk, N = sum over g of
 *                          group_tokens_g
 * Every integer becomes a double once, then one rounding per operation in the
 * order written (mean's denominator is the product 4294967296.0 * (double)
 * group_docs_g).  A value is NaN where a denominator (group_tokens_g,
 * group_docs_g, N_k, N) is 0; lift is -inf where tokens_gk = 0 and no
 * denominator is.  An unknown kind, or a kind without the table it needs, is
 * LDA_ERR_INVALID_ARG with a message.
 * ldatm_group_prevalence: counts only the table the kind needs, then finishes;
 * out[G*K].
 * ldatm_group_top_topics_select (host only): per group the n largest values
 * of a G x K matrix, ldatm_topic_partners_select's rule: larger value first,
 * equal values by smaller topic id, non-finite values left out; ids / values
 * [G*n], -1 / NaN past the last.
 * ldatm_group_topics_text / ldatm_print_group_topics: that selection of
 * ldatm_group_prevalence's matrix as text, "#group topic value\n", then
 * "<group> <topic> <value>\n" per group and rank (Java Double.toString);
 * empty slots print nothing.  ldatm_group_topics_format: the text from the
 * caller's G x n arrays (host only).
 * ldatm_subcorpus_top_words: each topic's top n words inside the documents
 * whose byte of doc_mask[D] (global order) is nonzero: every shard counts its
 * slice (lda_subcorpus_count), the tables are added into the first shard's
 * (lda_subcorpus_merge), which selects (lda_subcorpus_top_words: word_ids /
 * counts [K*n] as ldatm_top_words gives them, totals[K] the topic's tokens in
 * the sub-corpus), and the tables are released whatever the outcome.
 * Errors, checked before any device work (a model without a GPU names its bad
 * argument): LDA_ERR_INVALID_ARG for a NULL model, an unknown kind, G < 1, a
 * NULL required output, min_tokens < 1, min_count < 1, min_prop outside [0, 1]
 * or NaN, n < 1 (n outside [1, LDA_TOP_WORDS_MAX] for the words), a NULL
 * doc_group / doc_mask with documents, a group id outside [-1, G) (the
 * message names the first such document); LDA_ERR_UNSUPPORTED for G * K >
 * LDA_GROUP_TOPICS_MAX_CELLS. */
#define LDATM_GROUP_TOKENS 0
#define LDATM_GROUP_DOCUMENTS 1
#define LDATM_GROUP_MEAN 2
#define LDATM_GROUP_LIFT 3
lda_status ldatm_group_topics(ldatm* m, const int32_t* doc_group /*[D]*/, int32_t G, int64_t min_tokens,
                              int32_t min_count, double min_prop, int64_t* group_docs /*[G]*/,
                              int64_t* group_tokens /*[G]*/, int64_t* tokens /*[G*K]*/,
                              int64_t* present /*[G*K] or NULL*/, uint64_t* shares /*[G*K] or NULL*/);
lda_status ldatm_group_prevalence_finish(int32_t kind, int32_t G, int32_t K, const int64_t* group_docs,
                                         const int64_t* group_tokens, const int64_t* tokens,
                                         const int64_t* present /*or NULL*/, const uint64_t* shares /*or NULL*/,
                                         double* out /*[G*K]*/);
lda_status ldatm_group_prevalence(ldatm* m, const int32_t* doc_group /*[D]*/, int32_t G, int32_t kind,
                                  int64_t min_tokens, int32_t min_count, double min_prop, double* out /*[G*K]*/);
lda_status ldatm_group_top_topics_select(int32_t G, int32_t K, int32_t n, const double* matrix /*[G*K]*/,
                                         int32_t* ids /*[G*n]*/, double* values /*[G*n]*/);
lda_status ldatm_group_topics_text(ldatm* m, const int32_t* doc_group /*[D]*/, int32_t G, int32_t kind, int32_t n,
                                   int64_t min_tokens, int32_t min_count, double min_prop, char* buf, size_t cap,
                                   size_t* len);
lda_status ldatm_print_group_topics(ldatm* m, const char* path, const int32_t* doc_group /*[D]*/, int32_t G,
                                    int32_t kind, int32_t n, int64_t min_tokens, int32_t min_count, double min_prop);
lda_status ldatm_group_topics_format(int32_t G, int32_t n, const int32_t* ids, const double* values, char* buf,
                                     size_t cap, size_t* len);
lda_status ldatm_subcorpus_top_words(ldatm* m, const uint8_t* doc_mask /*[D]*/, int32_t n,
                                     int32_t* word_ids /*[K*n]*/, int32_t* counts /*[K*n]*/, int64_t* totals /*[K]*/);

/* Relevance-ranked topic words, salient terms and word rows: what an LDAvis
 * view shows (lda_relevant_words, lda_salient_words and lda_word_rows of
 * lda_mi355x.h, which states the definitions).  They run on shard 0
 * as ldatm_top_words does: after the exchange every shard's nw is global, so
 * the result does not depend on the number of shards.
 * ldatm_relevant_words: planes [L][K][n] of word_ids / counts (nw[w,k]) /
 * totals (tw[w]) / logprob / loglift, per lambda and topic the words with
 * nw[w,k] > 0 by key = logprob - (1 - lambda) logtp descending, equal keys by
 * ascending id; -1 / 0 / 0 / 0.0 / 0.0 past a topic's last candidate.
 * ldatm_salient_words: the n words of largest saliency, descending, equal
 * values by ascending id; -1 / 0 / 0.0 / 0.0 past the last word with a token.
 * ldatm_word_rows: rows[M*K] and totals[M] of the listed words (any order,
 * duplicates allowed); M = 0 succeeds and touches nothing.
 * Errors, checked before any device work in the order of the sampler's calls
 * (a model without documents or without a GPU names its bad argument):
 * LDA_ERR_INVALID_ARG for a NULL model, n outside [1, LDA_TOP_WORDS_MAX]
 * (salient: [1, LDA_SALIENT_WORDS_MAX]), L outside
 * [1, LDA_RELEVANCE_LAMBDAS_MAX], a NULL lambdas, a lambda not finite or
 * outside [0, 1], M < 0, a NULL list, a word id outside [0, V), a NULL output.
 * Waits for shard 0's stream.
 * ldatm_print_relevant_words / ldatm_relevant_words_text: the selection for
 * one lambda as text, "#topic rank word count total relevance logprob
 * loglift\n", then per topic and rank "<topic> <rank> <word> <nw[w,k]> <tw[w]>
 * <relevance> <logprob> <loglift>\n" (the alphabet's word, else the id; the
 * numbers as ldatm_format_double's Java Double.toString; relevance recomputed
 * as logprob - (1 - lambda) (logprob - loglift)); padded slots print nothing.
 * Same errors; buf / cap / len as the other *_text calls.
 * ldatm_relevant_words_format: that text from the caller's K x n arrays (host
 * only, no model and no device); names[num_names] gives the word column (NULL
 * entry or an id >= num_names: the id). */
lda_status ldatm_relevant_words(ldatm* m, int32_t n, int32_t L, const double* lambdas /*[L]*/,
                                int32_t* word_ids /*[L*K*n]*/, int32_t* counts /*[L*K*n]*/,
                                int64_t* totals /*[L*K*n]*/, double* logprob /*[L*K*n]*/,
                                double* loglift /*[L*K*n]*/);
lda_status ldatm_salient_words(ldatm* m, int32_t n, int32_t* word_ids /*[n]*/, int64_t* totals /*[n]*/,
                               double* saliency /*[n]*/, double* distinctiveness /*[n]*/);
lda_status ldatm_word_rows(ldatm* m, int64_t M, const int32_t* word_ids /*[M]*/, int32_t* rows /*[M*K]*/,
                           int64_t* totals /*[M]*/);
lda_status ldatm_print_relevant_words(ldatm* m, const char* path, int32_t n, double lambda);
lda_status ldatm_relevant_words_text(ldatm* m, int32_t n, double lambda, char* buf, size_t cap, size_t* len);
lda_status ldatm_relevant_words_format(int32_t K, int32_t n, double lambda, const int32_t* word_ids,
                                       const int32_t* counts, const int64_t* totals, const double* logprob,
                                       const double* loglift, const char* const* names, int64_t num_names,
                                       char* buf, size_t cap, size_t* len);

/* Topic phrases: each topic's most frequent same-topic token runs, counted on
 * the device (lda_topic_phrases of lda_mi355x.h; the question
 * Mallet's --xml-topic-phrase-report answers, by this library's definition: a
 * run is a maximal range of consecutive tokens of one document with one
 * topic, it qualifies with min_len <= length <= max_len, a longer run counts
 * toward skipped_long alone; Mallet's own loop, as recalled and not tested
 * against, never counts a run that reaches a document's last token and does
 * not let a phrase's closing token start the next one).
 * ldatm_topic_phrases: per topic k < K the first n phrases with count >=
 * min_count by count descending, then word id sequence ascending, a prefix
 * before its extension: phrase_words[K*n*max_len] (-1 padded), lengths[K*n],
 * counts[K*n], first[K*n] (the smallest GLOBAL token index at which the phrase
 * starts, tokens numbered through the documents in order), empty slots -1 / 0
 * / 0 / -1; topic_runs[K] the qualifying runs, topic_distinct[K] the distinct
 * phrases before min_count, *skipped_long the runs longer than max_len.
 * One shard: lda_topic_phrases passed through, proven[k] = n.
 * Several shards (contiguous document ranges): every shard lists its best
 * LDA_PHRASES_MAX = 128 phrases per topic; the lists are united by content;
 * every candidate's exact total and smallest start come from
 * lda_phrase_lookup on every shard; the candidates are ordered by the rule
 * above on their totals.  A phrase outside the union is outside every shard's
 * list, so its total is at most B_k = sum over the shards g of tau_g, tau_g
 * being shard g's 128th count for the topic (0 if its list is not full).
 * proven[k] is the number of leading entries whose total is strictly above
 * B_k: those, in that order, are the topic's true leading phrases.  B_k = 0
 * (no shard's list is full): the union is everything and proven[k] = n.
 * topic_runs and skipped_long are sums over the shards; topic_distinct is not
 * a sum, a phrase may live in several shards: it is -1 with several shards.
 * Errors, checked before any device work: LDA_ERR_INVALID_ARG for a NULL
 * model or output, n outside [1, LDA_PHRASES_MAX], limits outside 2 <= min_len
 * <= max_len <= LDA_PHRASE_LEN_MAX, min_count < 1.
 * ldatm_topic_phrases_text / ldatm_print_topic_phrases: the lists as text,
 * "#topic rank count phrase\n", then per topic and rank (from 0)
 * "<topic> <rank> <count> <word> <word> ...\n", single spaces, the alphabet's
 * words (the ids without an alphabet); empty slots print nothing.
 * ldatm_topic_phrases_format: that text from the caller's arrays (host only);
 * names[num_names] names the words (NULL or no entry: the id).
 * ldatm_topic_phrases_bound: B_k and proven[k] from the shards' listed counts
 * shard_counts[shards][K][LDA_PHRASES_MAX] and totals[K*n] (host only). */
lda_status ldatm_topic_phrases(ldatm* m, int32_t n, int32_t min_len, int32_t max_len, int32_t min_count,
                               int32_t* phrase_words /*[K*n*max_len]*/, int32_t* lengths /*[K*n]*/,
                               int64_t* counts /*[K*n]*/, int64_t* first /*[K*n]*/, int64_t* topic_runs /*[K]*/,
                               int64_t* topic_distinct /*[K]*/, int64_t* skipped_long, int32_t* proven /*[K]*/);
lda_status ldatm_topic_phrases_text(ldatm* m, int32_t n, int32_t min_len, int32_t max_len, int32_t min_count,
                                    char* buf, size_t cap, size_t* len);
lda_status ldatm_print_topic_phrases(ldatm* m, const char* path, int32_t n, int32_t min_len, int32_t max_len,
                                     int32_t min_count);
lda_status ldatm_topic_phrases_format(int32_t K, int32_t n, int32_t max_len, const int32_t* phrase_words,
                                      const int32_t* lengths, const int64_t* counts, const char* const* names,
                                      int64_t num_names, char* buf, size_t cap, size_t* len);
lda_status ldatm_topic_phrases_bound(int32_t K, int32_t n, int32_t shards, const int64_t* shard_counts,
                                     const int64_t* totals, int64_t* bound /*[K]*/, int32_t* proven /*[K]*/);

/* Checkpoint / resume: the reference's save()/load() of its model
 * (src/cmu_ron/TrainAndPredict.java:179-200) as a native binary file holding
 * every field needed to continue bit for bit (documents, alphabet, sources,
 * topics, alpha/beta, options, pending optimisation statistics and the
 * Philox sweep counter).  ldatm_load creates a new model. */
lda_status ldatm_save(ldatm* m, const char* path);
lda_status ldatm_load(ldatm** out, const char* path);

/* getInferencer().getSampledDistribution(instance, numIterations, thinning,
 * burnIn) [src/cmu_ron/TrainAndPredict.java:144], batched over Dh documents
 * (word ids of the model alphabet; ids >= V are dropped like Mallet's
 * unknown-type tokens).  theta[Dh*K]. */
lda_status ldatm_infer(ldatm* m, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                       int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed,
                       double* theta);

/* Prediction scoring: the reference compares a changelist's inferred
 * distribution with getTopicProbabilities of every training document
 * [src/cmu_ron/TrainAndPredict.java Predictor.predict with
 * Metrics.cosineSimilarity; src/cmu/TrainAndPredict.java
 * scoresForChangelistOnTests, whose "mse" is taken as the mean squared
 * difference it evidently means].  Here that is one batched call per shard on
 * the device (lda_score_docs; metric LDA_SCORE_COSINE / LDA_SCORE_MSE); no
 * copy of z and no Q x D x K loop on the host.
 *
 * ldatm_score_theta: precomputed distributions theta[Q*K] against the global
 * document ids docs[M] (any order, duplicates allowed), or docs == NULL: all
 * documents, M = the model's D.  scores[Q*M] row-major.  Global ids are mapped
 * onto the shards' document ranges; each shard scores its own documents on
 * its own device and stream and the results are scattered back into the
 * caller's order; they do not depend on the number of shards, bit for bit.
 * Errors: LDA_ERR_INVALID_ARG for a NULL model or scores, an unknown metric, a
 * document id outside [0, D), M != D without a list, or a theta row with a
 * negative / non-finite entry or a zero sum.  Q = 0 or M = 0 succeeds. */
lda_status ldatm_score_theta(ldatm* m, int32_t metric, int64_t Q, const double* theta,
                             int64_t M, const int64_t* docs, double* scores);
/* ldatm_infer (same arguments) followed by ldatm_score_theta of its result:
 * scores[Dh*M]; theta_out[Dh*K] receives the inferred distributions when not
 * NULL. */
lda_status ldatm_score(ldatm* m, int32_t metric, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                       int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed,
                       int64_t M, const int64_t* docs, double* scores, double* theta_out);
/* The n best documents of the whole model per query: doc_ids[Q*n] (global
 * ids) and scores[Q*n], best first -- the largest cosine, the smallest mse --
 * equal scores by ascending document id.  Scored shard by shard in chunks of
 * at most 2^22 scores; the n best per query are kept on the host.  With n
 * above D the first D entries are filled and the rest are id -1, score NaN.
 * Errors as ldatm_score_theta (NULL doc_ids / scores, n < 0: INVALID_ARG). */
lda_status ldatm_score_top(ldatm* m, int32_t metric, int64_t Q, const double* theta, int32_t n,
                           int64_t* doc_ids, double* scores);

/* Held-out evaluation by document completion, on the device (lda_heldout_loglik
 * / lda_doc_completion of lda_mi355x.h; formulas and error bound there and in
 * DESIGN 9c).  Both calls run on shard 0: every shard holds the same global
 * counts, and the inference draws are keyed by a token's index in the batch,
 * so spreading the documents over shards would change theta.  The results do
 * not depend on the number of shards, bit for bit.
 *
 * ldatm_heldout_loglik: theta[Dh*K] and the scored tokens are given (word ids
 * must lie in [0, V)); doc_ll[Dh], and total (may be NULL) = their sum added
 * in document order.  Errors as lda_heldout_loglik. */
lda_status ldatm_heldout_loglik(ldatm* m, int64_t Dh, const double* theta, const int64_t* doc_off,
                                const int32_t* words, double* doc_ll, double* total);
/* ldatm_evaluate: whole held-out documents are given.  Tokens outside [0, V)
 * are dropped, as ldatm_infer drops them, and are not counted; then the
 * first floor(L/2) tokens of each document are observed (ldatm_infer's
 * arguments apply to them) and the rest are scored.  doc_ll[Dh]; total,
 * tokens_scored (the number of scored tokens: perplexity =
 * exp(-total / tokens_scored)) and theta_out[Dh*K] may be NULL. */
lda_status ldatm_evaluate(ldatm* m, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                          int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed,
                          double* doc_ll, double* total, int64_t* tokens_scored, double* theta_out);
/* ldatm_left_to_right: Mallet's MarginalProbEstimator.evaluateLeftToRight
 * (ParallelTopicModel.getProbEstimator()) over whole held-out documents, on
 * the device (lda_left_to_right of lda_mi355x.h; the estimator, its draw and
 * its random stream there and in DESIGN 9f).  Tokens outside [0, V) are
 * dropped first, as ldatm_evaluate drops them, and are not counted; a draw's
 * token index g counts the kept tokens.  Runs on shard 0 for the reason above
 * (the draws are keyed by a token's index in the call), so the results do not
 * depend on the number of shards, bit for bit; the model's state is required
 * and left as ldatm_evaluate requires and leaves it.  doc_ll[Dh]; total
 * (their sum in document order) and tokens_scored (perplexity = exp(-total /
 * tokens_scored)) may be NULL.  Errors as lda_left_to_right: num_particles <
 * 1 INVALID_ARG; more than LDA_LTR_MAX_PARTICLES particles or a document of
 * more than LDA_LTR_MAX_DOC_TOKENS kept tokens UNSUPPORTED. */
lda_status ldatm_left_to_right(ldatm* m, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                               int32_t num_particles, int32_t resampling, uint64_t seed, double* doc_ll,
                               double* total, int64_t* tokens_scored);
/* The split ldatm_evaluate makes (host-only): obs_off / sc_off [Dh+1];
 * obs_words / sc_words (may be NULL to get the offsets only) need room for
 * the document's tokens. */
lda_status ldatm_completion_split(int32_t num_types, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                                  int64_t* obs_off, int32_t* obs_words, int64_t* sc_off, int32_t* sc_words);
/* A held-out set that ldatm_estimate evaluates (as ldatm_evaluate, with these
 * arguments) after every sweep `it` with it % interval == 0, after that
 * sweep's alpha / beta optimisation: it logs "<it> held-out LL/token: x" and
 * appends (it, total / tokens_scored) to the trace, which ldatm_estimate
 * clears when it starts.  interval = 0 turns it off.  The evaluation reads the
 * counts and writes only its own scratch: z, alpha and beta after
 * ldatm_estimate are the same bits with it on or off.  The documents are
 * copied.  The held-out set is not written by ldatm_save (the checkpoint
 * format is unchanged): set it again after ldatm_load. */
lda_status ldatm_set_held_out(ldatm* m, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                              int32_t interval, int32_t num_iterations, int32_t thinning, int32_t burn_in,
                              uint64_t seed);
/* shaped like ldatm_get_ll_trace */
lda_status ldatm_get_held_out_trace(ldatm* m, int32_t* iterations, double* ll, int32_t cap, int32_t* n);

/* The number renderings of Mallet's text outputs (host-only): style 0 =
 * Double.toString (printDocumentTopics weights), 1 = NumberFormat with at
 * most 5 fraction digits (printTopWords alpha, LL/token log). */
lda_status ldatm_format_double(double x, int32_t style, char* buf, size_t cap);

const char* ldatm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* LDA_TOPIC_MODEL_H */
