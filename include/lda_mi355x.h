/*
 * lda_mi355x.h — C ABI of the MI355X-native collapsed-Gibbs LDA sampler.
 *
 * This is the drop-in boundary for the reference's only hot path: the
 * per-token z-resampling loop that qianjinding/LDAGibbsSampling delegates to
 * Mallet 2.0.7 (pom.xml:107-111) through
 *     ParallelTopicModel.estimate()            src/cmu_ron/TrainAndPredict.java:166
 *                                              src/cmu/TrainAndPredict.java:265
 * and from there WorkerRunnable.sampleTopicsForOneDoc (Mallet, not vendored).
 * The reference has no FFI of its own; the seam is Mallet's public class API
 * as called from trainNewModel (src/cmu_ron/TrainAndPredict.java:159-171,
 * src/cmu/TrainAndPredict.java:258-269).  Each entry point below names the
 * Mallet call it replaces; INTEGRATION.md shows the JNI binding a Java
 * maintainer adds (GpuParallelTopicModel extends ParallelTopicModel).
 *
 * Conventions
 *  - Plain pointers and sizes only.  The caller owns every host buffer;
 *    lda_create copies its inputs into device memory and no pointer is kept
 *    after a call returns (except lda_delta_buffer's device pointer, which is
 *    owned by the context).
 *  - Every call returns an lda_status (0 = OK, < 0 = error class);
 *    lda_last_error() gives a thread-local message.  No C++ exception crosses
 *    the ABI.
 *  - One context = one GPU = one caller thread (not re-entrant per context).
 *    Multi-GPU: one process (or thread) per GPU, each with a context over its
 *    own document shard, exchanging the nw/nwsum delta buffer with an
 *    all-reduce between lda_sample() and lda_apply() (AD-LDA).
 *  - Counts are int32 (exact).  Sampling weights are fp32, evaluated in the
 *    fixed order documented in DESIGN.md so that z/nw/nwsum/nd are bit-exact
 *    against the CPU oracle and independent of GPU count and scheduling.
 */
#ifndef LDA_MI355X_H
#define LDA_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t lda_status;
#define LDA_OK 0
#define LDA_ERR_INVALID_ARG (-1)
#define LDA_ERR_DEVICE (-2)       /* HIP runtime / kernel launch failure */
#define LDA_ERR_OUT_OF_MEMORY (-3)
#define LDA_ERR_STATE (-4)        /* call out of order (e.g. sample with a pending delta) */
#define LDA_ERR_UNSUPPORTED (-5)  /* e.g. K above the compiled maximum */
#define LDA_ERR_INTERNAL (-6)     /* an unexpected C++ exception, caught at the ABI */

#define LDA_MAX_TOPICS 4096       /* K <= 4096 (LDA_SAMPLER_SPARSE above 1024)       */
#define LDA_MAX_TOPICS_DENSE 1024 /* the dense sampler's register-resident rows      */
/* With K > 1024 (Kp > 1024) a document's topic counts live in LDS as 16-bit
 * pairs: documents are limited to 65535 tokens there (LDA_ERR_UNSUPPORTED). */
#define LDA_MAX_DOC_TOKENS_BIGK 65535

/* Draw kernels.  Both are exact against the CPU oracle.
 *  DENSE   reads the word's whole row from a 16-bit copy of nw (2K bytes per
 *          token; the int32 row for words with a count > 65535);
 *  SPARSE  reads only the row's nonzero (count, topic) entries (4 bytes each),
 *          SparseLDA-style split into a word part and a dense doc part
 *          (a different fp32 summation with its own oracle restatement). */
/* The dense sampler needs num_types * Kp < 2^32 (V < 4.19M words at K = 1024). */
#define LDA_SAMPLER_DENSE 0
#define LDA_SAMPLER_SPARSE 1

typedef struct lda_ctx lda_ctx;

typedef struct lda_config {
  int32_t num_topics;     /* K      (ParallelTopicModel(numberOfTopics, ...)) */
  int32_t num_types;      /* V      (alphabet size; word ids are 0..V-1)       */
  int64_t num_docs;       /* D      documents in THIS shard                    */
  const double* alpha;    /* [K] per-topic alpha (alphaSum/K when symmetric)   */
  double beta;            /* beta   (ParallelTopicModel(.., .., beta))         */
  uint64_t seed;          /* Philox key (ParallelTopicModel.setRandomSeed)     */
  int32_t device;         /* HIP device ordinal                                */
  int32_t sampler;        /* LDA_SAMPLER_DENSE (0) or LDA_SAMPLER_SPARSE (1)   */
  int64_t token_base;     /* global index of this shard's first token          */
  int64_t tokens_per_range; /* work-queue granule (0 = default)                */
} lda_config;

/* Create a sampler over one shard.  doc_off[D+1] (int64, doc_off[0] may be
 * non-zero: offsets are rebased), words[N] (int32 word ids), z_init[N] or NULL
 * (NULL = Philox initialisation, the GPU analogue of addInstances' random
 * topics).  The shard's own counts are left as the PENDING delta: call
 * lda_apply (after an all-reduce of lda_delta_buffer when sharded) before the
 * first lda_sample.  Replaces ParallelTopicModel(K, alphaSum, beta) +
 * addInstances(InstanceList)  [src/cmu_ron/TrainAndPredict.java:160-162]. */
lda_status lda_create(lda_ctx** out, const lda_config* cfg, const int64_t* doc_off,
                      const int32_t* words, const int32_t* z_init);
void lda_destroy(lda_ctx* ctx);

/* Run n full sweeps on a single (unsharded) context: apply any pending delta,
 * then n x (sample + apply).  Replaces ParallelTopicModel.estimate() with
 * setNumIterations(n) and optimizeInterval 0 [src/cmu_ron/TrainAndPredict.java:165-166].
 * Plain dense sweeps (one part, not warm-start or recount sweeps) are
 * launched as hipGraphs of up to 16 sweeps, captured once per length on the
 * context's stream; the results are those of n lda_sample + lda_apply calls
 * (the sweep counter and beta are read from device memory).  No event timing
 * is recorded for them (lda_sample_times covers lda_sample launches).  The
 * environment variable LDA_GRAPHS=0 at lda_create turns the graphs off. */
lda_status lda_sweep(lda_ctx* ctx, int32_t n);

/* One sampling pass over the shard against the current nw/nwsum snapshot
 * (one sweep of WorkerRunnable.run()); its result goes to the exchange
 * buffer below.  Asynchronous on the context's stream, except that the
 * large-K sampler (K > 1024) times its two ring depths from the ninth sweep
 * on, every 19 sweeps: the sweep after such a probe waits on the host for
 * the probe's last launch (LDA_SB_RB=short or default at
 * lda_create fixes the ring and never waits).  Either ring gives the same
 * draws. */
lda_status lda_sample(lda_ctx* ctx);
/* Device pointer to the pending exchange buffer: int32[V*Kp + Kp] (an nw part
 * row-major with padded row length Kp = lda_padded_topics(), then an nwsum
 * part).  Sum it across ranks in place (the sumTypeTopicCounts analogue)
 * before lda_apply.  What it holds depends on the count-update mode
 * (lda_count_update_mode): the dense samplers RECOUNT -- the sampler writes
 * only z and the buffer receives this shard's own (word, topic) counts, which
 * lda_apply's sum replaces nw / nwsum with -- the sparse samplers keep a
 * DELTA of the shard's changes, which lda_apply adds.  Either way the caller
 * only sums it, and lda_apply leaves it zero. */
lda_status lda_delta_buffer(lda_ctx* ctx, void** dev_ptr, size_t* count);
/* recount = 1 when the pending buffer holds counts (or, with nothing
 * pending, when the next sweep will recount), 0 for a delta. */
lda_status lda_count_update_mode(lda_ctx* ctx, int32_t* recount);
/* Which sweeps recount (dense samplers; the sparse ones always keep a delta).
 *  LDA_COUNT_AUTO     the first recount_sweeps sweeps after the counts are
 *                     (re)seeded by lda_create / lda_set_z recount, later
 *                     ones keep a delta (near init nearly every token
 *                     changes, and the delta's device atomics cost more than
 *                     the recount; later they cost less).  The default is
 *                     LDA_RECOUNT_SWEEPS_DEFAULT when K <= 128 and the
 *                     shard holds 2^20 <= N tokens with z fitting the
 *                     Infinity Cache (4 N <= 256 MiB), else 0 (measured
 *                     crossover: DESIGN.md §4).
 *                     recount_sweeps < 0 keeps the current value.
 *                     Sequential sweeps -- warm-start sweeps
 *                     (lda_set_warm_start) and the steady ones of
 *                     lda_set_sequential_sweeps -- never recount under AUTO
 *                     but do count toward the window: with the native
 *                     ParallelTopicModel's default 4 x 50 warm start the
 *                     window has passed before the first plain sweep, which
 *                     is right, since after ~20 sweeps the delta is the
 *                     faster update; and its default Mallet-
 *                     staleness schedule makes every later sweep sequential
 *                     as well.  AUTO recount therefore acts only on plain
 *                     snapshot sweeps (lda_sweep without either schedule,
 *                     bench.py).
 *  LDA_COUNT_RECOUNT  every sweep, sequential ones included (after each part
 *                     the whole shard is recounted into buffer 0, the parts
 *                     sampled so far with their new topics);
 *  LDA_COUNT_DELTA    none.
 * Shards exchanging buffers must agree on it sweep by sweep: a distributed
 * driver sets the same mode and count on every rank (ADLDATrainer: the
 * minimum over ranks).  Results are identical in every mode.  On recount
 * sweeps the K <= 128 default sampler also keeps a copy of z in the
 * recount's word order (N int32 + N uint32 of device memory, allocated at
 * the first recount sweep) so that the recount streams it instead of
 * gathering z; LDA_ZW=0 at lda_create turns the copy off. */
#define LDA_COUNT_AUTO 0
#define LDA_COUNT_RECOUNT 1
#define LDA_COUNT_DELTA 2
#define LDA_RECOUNT_SWEEPS_DEFAULT 20
lda_status lda_set_count_update(lda_ctx* ctx, int32_t mode, int32_t recount_sweeps);
lda_status lda_get_count_update(lda_ctx* ctx, int32_t* mode, int32_t* recount_sweeps);
/* nw/nwsum := buffer (recount) or += buffer (delta), buffer = 0, refresh the
 * per-topic tables. */
lda_status lda_apply(lda_ctx* ctx);

/* Split sweep: the exchange overlapped with sampling.
 * Mallet sums its workers' counts only after every worker has finished the
 * sweep (ParallelTopicModel.sumTypeTopicCounts, [M]); here the shard's work
 * ranges are cut into `parts` token-balanced parts (1..LDA_MAX_EXCHANGE_PARTS),
 * each with its own delta buffer.  lda_sample_part(ctx, i) samples part i
 * against the unchanged snapshot; after it, buffer i is final for the sweep,
 * so its all-reduce can run (on another stream) while part i+1 samples.
 * Parts are sampled in order 0..parts-1 and all use the same sweep counter;
 * lda_apply folds every buffer.  Results are identical for any `parts`
 * (integer sums; draws keyed by the global token index).  lda_sample runs
 * every part.  reserve_cus: CUs' worth of sampler blocks left free in a split
 * sweep for the collective's kernels (0 = none, < 0 = the default: 1/32 of
 * the device's CUs, 8 on MI355X).  Sequential sweeps (warm start, steady
 * schedule) ignore the split: their parts are the schedule's, each summed and
 * applied before the next part samples (an exchange per part, nothing to
 * overlap), so under the native ParallelTopicModel's default staleness
 * schedule a multi-GPU sweep exchanges 2-4 times. */
#define LDA_MAX_EXCHANGE_PARTS 4
lda_status lda_set_exchange_parts(lda_ctx* ctx, int32_t parts, int32_t reserve_cus);
lda_status lda_get_exchange_parts(lda_ctx* ctx, int32_t* parts);
lda_status lda_sample_part(lda_ctx* ctx, int32_t part);
lda_status lda_delta_buffer_part(lda_ctx* ctx, int32_t part, void** dev_ptr, size_t* count);

/* Compact exchange.  The buffer of lda_delta_buffer_part
 * holds int32 cells [V*Kp | Kp]; summed across `world` ranks as they are,
 * that is 4 (V Kp + Kp) bytes per sweep (C5: 4.3 GB).  Instead a driver may
 * exchange it packed, two cells per int32 word:
 *   lda_exchange_sizes: packed_count int32 words [V*Kp/2 | Kp] and
 *     escape_count int32 of one rank's escape list, for `world` ranks whose
 *     largest shard holds max_shard_tokens tokens (the same on every rank);
 *   lda_exchange_pack(part): packs the part's buffer on the context's stream
 *     and returns the context-owned device arrays to exchange;
 *   the driver: SUM all-reduce (int32) of `packed` in place, and an
 *     all-gather of every rank's `escapes` into one device array
 *     [world x escape_count] in rank order;
 *   lda_exchange_unpack(part, escapes_all): the part's buffer = the unpacked
 *     sum plus every rank's escapes (then lda_apply as usual).
 * Cell 2i packs as d + 2^15/world (bits 0..15), cell 2i+1 as d + 2^14/world
 * (bits 16..30): the sum over the ranks cannot carry between the halves or
 * overflow int32.  Cells outside that range travel in the escape list
 * (count, then (cell lo, cell hi, value) triples); each rank has at most
 * 2 max_shard_tokens / (2^14/world) of them, since a rank's |cells| sum to
 * at most twice its tokens.  The result is the int32 sum, bit for bit. */
lda_status lda_exchange_sizes(lda_ctx* ctx, int32_t world, int64_t max_shard_tokens, size_t* packed_count,
                              size_t* escape_count);
lda_status lda_exchange_pack(lda_ctx* ctx, int32_t part, int32_t world, int64_t max_shard_tokens, void** packed,
                             void** escapes);
lda_status lda_exchange_unpack(lda_ctx* ctx, int32_t part, int32_t world, int64_t max_shard_tokens,
                               const void* escapes_all);
/* The escape lists sent at their used length (ldagibbssampling_amd/
 * distributed.py): escapes[0] after lda_exchange_pack is the rank's escape
 * count n (n > escape capacity cannot happen when every rank's shard holds at
 * most max_shard_tokens tokens; a driver that reads n > capacity must stop).
 * A driver that MAX-all-reduces n into m (identical on every rank) may
 * all-gather only the first 1 + 3 m int32 of each rank's list into
 * [world x (1 + 3 m)] and unpack with list_cap = m; m = 0 needs no all-gather
 * (escapes_all may be NULL).  list_cap in [0, capacity]; lda_exchange_unpack
 * is list_cap = capacity. */
lda_status lda_exchange_unpack_lists(lda_ctx* ctx, int32_t part, int32_t world, int64_t max_shard_tokens,
                                     const void* escapes_all, int32_t list_cap);
/* Cells per packed word (round 6): 2 (the default, above) or 4 -- cells
 * 4i..4i+2 as d + 2^7/world in bits 0..7, 8..15, 16..23 and cell 4i+3 as
 * d + 2^6/world in bits 24..30 (world <= 64), half the packed bytes of the
 * default (C5 at 8 ranks: 1.07 GB instead of 2.15 GB per exchange) at the
 * price of more escapes (a cell escapes beyond [-16, 16) at 8 ranks instead
 * of [-2048, 2048)); the escape capacity of lda_exchange_sizes follows the
 * smaller bias.  Every rank of a group must use the same value.  The result
 * is the same int32 sum, bit for bit. */
lda_status lda_set_exchange_cells(lda_ctx* ctx, int32_t cells_per_word);
lda_status lda_get_exchange_cells(lda_ctx* ctx, int32_t* cells_per_word);
/* Replica check (bench.py's multi-GPU line): a hash of the applied counts,
 * the sum mod 2^64 over the nonzero cells of nw (V x K) and nwsum (K) of
 * splitmix64's finaliser applied to (index << 32 | (uint32)value), index =
 * w K + k in nw and V K + k in nwsum (oracle.counts_checksum).  Every rank of
 * an AD-LDA group holds the same replica, so MIN == MAX over the ranks.
 * LDA_ERR_STATE with a pending delta.  Synchronises the context's stream. */
lda_status lda_counts_checksum(lda_ctx* ctx, uint64_t* checksum);

/* Warm start.  The GPU sweep samples every document against one snapshot
 * (AD-LDA), while Mallet's setNumThreads(4) workers each see their own
 * changes live: from a random start the snapshot sweep falls into a local
 * optimum more often (held-out perplexity over 96 seeds at
 * K = 20).  With lda_set_warm_start(ctx, parts, sweeps) the sweeps whose
 * sweep counter (lda_get_sweep: carried across estimate() calls and
 * checkpoints) is below `sweeps` run in `parts` token-balanced parts in
 * SEQUENTIAL order: part i samples against
 * the snapshot with parts 0..i-1 of this sweep applied.  Such a sweep keeps
 * its changes in buffer 0 (lda_delta_buffer_part returns it for every part)
 * and is never a recount sweep.  lda_sample / lda_sweep do it by themselves;
 * a sharding driver asks lda_sweep_parts and, when sequential, runs for
 * each part: lda_sample_part(i), sum buffer 0 across ranks, lda_apply.
 * parts in [1, LDA_MAX_EXCHANGE_PARTS] (1 = off).  The parts are cut in
 * the whole corpus, global token indices [corpus_first_token,
 * corpus_first_token + corpus_tokens) (corpus_tokens <= 0: this shard is the
 * whole corpus), into S = parts * LDA_WARM_BLOCKS token-balanced segments:
 * cut j is the first document starting at or after token
 * first + tokens * j / S, and segment j belongs to part j % parts.  A shard
 * samples its own documents of global part i in step i, so the result is the
 * same for any sharding and identical to cpu_exact's same schedule, and every
 * shard of a token-balanced sharding into <= LDA_WARM_BLOCKS shards has work
 * in every step. */
#define LDA_WARM_BLOCKS 64
/* Sequential parts are cut at cumulative fractions of each block in units of
 * 1 / LDA_SEQ_FRACTION_UNIT (lcm(1..16): equal parts are exact). */
#define LDA_SEQ_FRACTION_UNIT 720720
/* Host-only (no device call): the tokens a shard (documents doc_off[0..D],
 * global token base + doc_off[d] - doc_off[0]) samples in each warm-start
 * part of the corpus [corpus_first_token, + corpus_tokens), as
 * lda_set_warm_start cuts them; tokens_out[parts]. */
lda_status lda_warm_part_tokens(const int64_t* doc_off, int64_t num_docs, int32_t parts, int64_t token_base,
                                int64_t corpus_first_token, int64_t corpus_tokens, int64_t* tokens_out);
lda_status lda_set_warm_start(lda_ctx* ctx, int32_t parts, int32_t sweeps, int64_t corpus_first_token,
                              int64_t corpus_tokens);
lda_status lda_get_warm_start(lda_ctx* ctx, int32_t* parts, int32_t* sweeps);
/* Steady sequential sweeps: Mallet's staleness.  The snapshot sweep shows
 * every token none of the sweep's other changes; Mallet's setNumThreads(T)
 * workers each see their own changes live, so a token sees on average
 * 1/(2T) of them.  That difference is measurable at the reference's own
 * training settings: with hyperparameter optimisation the snapshot sweep
 * learns beta ~9% higher and alphaSum ~4% lower than Mallet's 4 threads and,
 * at K = 500, traps more chains.
 * lda_set_sequential_sweeps(ctx, parts, fractions, first, tokens): every
 * sweep that is not a warm-start sweep runs in `parts` sequential parts (as
 * the warm start's, each applied before the next samples, all through buffer
 * 0), part i taking the fraction fractions[i] of each of the
 * LDA_WARM_BLOCKS blocks of the corpus (fractions NULL: equal parts); parts
 * = 1 turns it off (the default: lda_sweep's plain snapshot sweeps).  The
 * corpus arguments are lda_set_warm_start's.  lda_staleness_schedule(T)
 * gives the schedule with Mallet's mean live fraction for T threads: two
 * parts, the first f = (1 - sqrt(1 - 2/T)) / 2 of every block (T = 4: f =
 * 0.146), so that f (1 - f) = 1/(2T); T = 1 gives LDA_MAX_EXCHANGE_PARTS
 * equal parts (mean 3/8, the nearest to sequential Mallet's 1/2).
 * lda_get_sequential_sweeps: the parts and the cumulative cut fractions
 * cum_units[parts + 1] in units of 1 / LDA_SEQ_FRACTION_UNIT. */
lda_status lda_set_sequential_sweeps(lda_ctx* ctx, int32_t parts, const double* fractions,
                                     int64_t corpus_first_token, int64_t corpus_tokens);
lda_status lda_get_sequential_sweeps(lda_ctx* ctx, int32_t* parts, int64_t* cum_units);
lda_status lda_staleness_schedule(int32_t threads, int32_t* parts, double* fractions);
/* The parts of the sweep in progress (or of the next one) and whether they
 * are sequential (a warm-start sweep) or exchange-overlapped. */
lda_status lda_sweep_parts(lda_ctx* ctx, int32_t* parts, int32_t* sequential);

/* The HIP stream every call of this context is ordered on (hipStream_t;
 * NULL = the context's own stream).  Work already queued on the previous
 * stream is ordered before the new stream's (an event, no host wait). */
lda_status lda_set_stream(lda_ctx* ctx, void* hip_stream);
lda_status lda_get_stream(lda_ctx* ctx, void** hip_stream);
lda_status lda_synchronize(lda_ctx* ctx);

/* Sweep counter (the Philox counter word that keys a sampling pass). */
lda_status lda_get_sweep(lda_ctx* ctx, uint32_t* sweep);
lda_status lda_set_sweep(lda_ctx* ctx, uint32_t sweep);

/* Kp = 64 * C, C the next power of two >= ceil(K/64) (1..64); lane l of a
 * wavefront owns topics [l*C, (l+1)*C). */
int32_t lda_padded_topics(int32_t num_topics);
lda_status lda_get_shape(lda_ctx* ctx, int32_t* K, int32_t* Kp, int32_t* V, int64_t* D,
                         int64_t* N);

/* Copy state out (caller-allocated host buffers; NULL skips an output).
 * z[N]; nw[V*K] row-major (unpadded); nwsum[K]; nd[D*K]; ndsum[D]. */
lda_status lda_get_z(lda_ctx* ctx, int32_t* z);
lda_status lda_set_z(lda_ctx* ctx, const int32_t* z); /* re-seeds counts as pending delta */
lda_status lda_get_counts(lda_ctx* ctx, int32_t* nw, int32_t* nwsum, int32_t* nd,
                          int32_t* ndsum);

/* Replace alpha[K] / beta (host-side hyperparameter optimisation,
 * ParallelTopicModel.optimizeAlpha/optimizeBeta). */
lda_status lda_set_alpha_beta(lda_ctx* ctx, const double* alpha, double beta);

/* ParallelTopicModel.modelLogLikelihood() over this shard's documents:
 * doc_part = sum_d [sum_k logG(a_k+n_dk)-logG(a_k)] - logG(A+n_d) + logG(A)
 * (fp64, Dirichlet.logGammaStirling); word_part = the nw/nwsum terms (global,
 * identical on every rank).  Total = sum over ranks of doc_part + word_part. */
lda_status lda_log_likelihood_parts(lda_ctx* ctx, double* doc_part, double* word_part);
lda_status lda_log_likelihood(lda_ctx* ctx, double* out); /* doc_part + word_part */
/* The same without waiting: the kernels and the copy of their partial sums
 * are enqueued on the context's stream, and the result is collected later
 * (ParallelTopicModel.estimate()'s "LL/token" every 10 sweeps no longer
 * stops the sweeps).  At most 16 results in flight: a 17th enqueue waits
 * for the oldest, whose ticket then no longer collects (LDA_ERR_STATE).  The
 * blocking calls above take no ticket and push none out of flight. */
lda_status lda_log_likelihood_enqueue(lda_ctx* ctx, int64_t* ticket);
lda_status lda_log_likelihood_collect(lda_ctx* ctx, int64_t ticket, double* doc_part, double* word_part);

/* TopicInferencer.getSampledDistribution(instance, numIterations, thinning,
 * burnIn) [src/cmu_ron/TrainAndPredict.java:144, src/cmu/TrainAndPredict.java:114]
 * batched over Dh held-out documents against the frozen model; the arguments
 * are in Mallet's order.  Word ids must be < V (out-of-vocabulary tokens are
 * removed by the caller); tokens whose type has no training tokens (an empty
 * typeTopicCounts row) are skipped, as Mallet's inferencer skips them.
 * theta[Dh*K] (fp64, rows sum to 1). */
lda_status lda_infer(lda_ctx* ctx, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                     int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed,
                     double* theta);

/* The reference's prediction step [src/cmu_ron/TrainAndPredict.java
 * Predictor.predict + Metrics.cosineSimilarity; src/cmu/TrainAndPredict.java
 * scoresForChangelistOnTests], batched: the similarity of Q topic
 * distributions theta[Q*K] (rows of lda_infer, or any non-negative rows; they
 * need not sum to 1) to the topic distribution of documents of THIS shard,
 *     p_d[k] = (n_dk + alpha_k) / (n_d + sum alpha),
 * what ParallelTopicModel.getTopicProbabilities returns, from the shard's
 * current z on the device.
 *  LDA_SCORE_COSINE  p_d . theta_q / (|p_d| |theta_q|)
 *  LDA_SCORE_MSE     sum_k (p_d[k] - theta_q[k])^2 / K
 * docs == NULL: documents [doc_begin, doc_begin + M); else docs[M] shard-local
 * ids in any order, duplicates allowed (doc_begin must be 0).  scores[Q*M]
 * row-major (scores[q*M + j] for the j-th document), fp64.  An empty document
 * scores as p_d = alpha / sum alpha.  Every sum is a fixed-order fp64
 * reduction: a call repeats bit for bit, and a document's scores do not
 * depend on M, docs or the shard's other documents.
 * Errors: LDA_ERR_STATE with a pending delta (call lda_apply first);
 * LDA_ERR_INVALID_ARG for an unknown metric, a document id or range outside
 * [0, D), a theta row with a negative or non-finite entry, or a theta row
 * that sums to zero.  Q = 0 or M = 0 succeeds and touches nothing.
 * Device scratch is grow-only and kept by the context.  The work is cut into
 * chunks of at most 1024 queries x 2^22 / min(Q, 1024) documents, so the
 * scratch never exceeds 32 MiB of scores + 32 MiB of document ids (docs
 * given) + 1024 (K + 2) doubles of queries (<= 32.1 MiB), whatever Q and M
 * are.  Waits for the context's stream. */
#define LDA_SCORE_COSINE 0
#define LDA_SCORE_MSE 1
lda_status lda_score_docs(lda_ctx* ctx, int32_t metric, int64_t Q, const double* theta,
                          int64_t doc_begin, int64_t M, const int64_t* docs, double* scores);

/* Held-out log likelihood by document completion, on the device against the
 * global counts this shard holds (the int32 nw rows and nwsum): for held-out
 * document d with topic distribution theta_d (a row of theta[Dh*K]; any
 * non-negative row, it need not sum to 1) and scored tokens
 * words[doc_off[d] - doc_off[0] .. doc_off[d+1] - doc_off[0]),
 *     doc_ll[d] = sum_i log sum_k theta_d[k] (nw[w_i,k] + beta) / (nwsum[k] + V beta)
 * in fp64.  Every token is scored, also one whose type has no training
 * tokens (its term is beta sum_k theta_d[k] / (nwsum[k] + V beta) > 0).  An
 * empty document gives 0.0.  total (may be NULL) receives doc_ll[0] + ... +
 * doc_ll[Dh-1] added in that order on the host, so it equals the caller's own
 * sum exactly.  The sums are fixed-order reductions without floating-point
 * atomics: a call repeats bit for bit, and doc_ll[d] depends on document d's
 * theta row and tokens alone, not on Dh, the other documents or the chunks.
 * Errors: LDA_ERR_STATE with a pending delta (call lda_apply first);
 * LDA_ERR_INVALID_ARG for a NULL ctx, theta, doc_off or doc_ll (words may be
 * NULL only without tokens), Dh < 0, a doc_off that is not monotone, a word id
 * outside [0, V), a theta entry that is negative or not finite, or a theta
 * row that sums to zero.  Dh = 0 succeeds and touches nothing.
 * Device scratch is grow-only and kept by the context.  The documents are cut
 * into chunks of at most max(1, 2^22 / K) documents (1024 at K = 4096) and at
 * most 2^23 tokens (a single longer document is a chunk of its own), so the
 * scratch never exceeds 32 MiB of theta + 32 MiB of word ids (or 4 bytes per
 * token of the longest document, if that is more) + 16 bytes per document of
 * a chunk for offsets and results (<= 64 MiB at K = 1) + 8 Kp bytes, whatever
 * Dh is.  Waits for the context's stream. */
lda_status lda_heldout_loglik(lda_ctx* ctx, int64_t Dh, const double* theta, const int64_t* doc_off,
                              const int32_t* words, double* doc_ll, double* total);
/* Document completion in one call: lda_infer on the observed halves
 * (obs_off, obs_words and the four sampling arguments exactly as lda_infer
 * takes them), then lda_heldout_loglik of the inferred distributions on the
 * scored halves (sc_off, sc_words).  theta_out[Dh*K] (may be NULL) receives
 * what lda_infer returns for the same arguments, bit for bit.  Errors as the
 * two calls; the scored halves are checked before the inference runs. */
lda_status lda_doc_completion(lda_ctx* ctx, int64_t Dh, const int64_t* obs_off, const int32_t* obs_words,
                              const int64_t* sc_off, const int32_t* sc_words, int32_t num_iterations,
                              int32_t thinning, int32_t burn_in, uint64_t seed, double* doc_ll,
                              double* total, double* theta_out);

/* Left-to-right held-out log likelihood: Mallet's MarginalProbEstimator
 * .evaluateLeftToRight (ParallelTopicModel.getProbEstimator(); Wallach et al.'s
 * particle estimator of log p(w | model)), on the device against the global
 * counts this shard holds.  With phi_wk = (nw_wk + beta) *
 * inv_k, inv_k = 1 / (nwsum_k + V beta), each particle r < num_particles of a
 * document w_0 .. w_{L-1} starts with nd = 0 and for each limit i = 0 .. L-1
 *  - if resampling != 0, visits j = 0 .. i-1 in order: takes z_j out of nd,
 *    draws z_j with weights (nd_k + alpha_k) phi_{w_j,k}, puts it back;
 *  - takes W = sum_k (nd_k + alpha_k) phi_{w_i,k}, p_r[i] = W / (sum alpha +
 *    the tokens scored so far), draws z_i with the same weights and adds it.
 * phat[i] = (p_0[i] + ... + p_{R-1}[i]) / R added in that order, and
 * doc_ll[d] = sum_i log phat[i].  A token whose type has no training tokens
 * (lda_infer's empty-row test) is skipped everywhere: no draw, no probability,
 * no count, not in tokens_scored; an empty or all-skipped document gives 0.0.
 * All arithmetic is fp64.  A draw with uniform u picks the smallest topic, in
 * ascending order, whose inclusive prefix of the weights exceeds u W, or the
 * last topic with a positive weight if none does; u = ((x0 << 21) | (x1 >>
 * 11)) 2^-53 from Philox4x32-10 with key seed and counter {g lo, g hi, i,
 * 3 | (r << 8)}, g = the drawn token's index within the call (doc_off[d] -
 * doc_off[0] + j), i the current limit, stream 3.  No floating-point atomics:
 * a call repeats bit for bit, and a document's results depend on its tokens,
 * their indices g and the arguments alone, not on Dh, the other documents,
 * the chunks or the grid; the first R particles of a call with more are the
 * particles of a call with R.
 * total (may be NULL) = doc_ll[0] + ... + doc_ll[Dh-1] added in that order on
 * the host; tokens_scored (may be NULL) = the tokens not skipped;
 * token_prob[N] (may be NULL) = phat per token, 0 for a skipped one;
 * z_out[num_particles * N] (may be NULL), particle-major, = each particle's
 * topics after its last pass, -1 for a skipped token (N = doc_off[Dh] -
 * doc_off[0]).
 * Cost: with resampling a document of L tokens takes L (L + 1) / 2 draws per
 * particle (L without), each a pass over the word's K counts; hence the
 * limits below.  Beyond either: LDA_ERR_UNSUPPORTED.
 * Errors, all checked on the host before any launch: LDA_ERR_INVALID_ARG for
 * a NULL ctx, doc_off or doc_ll (words may be NULL only without tokens),
 * Dh < 0, num_particles < 1, a doc_off that is not monotone, or a word id
 * outside [0, V); LDA_ERR_STATE with a pending delta (call lda_apply first).
 * Dh = 0 succeeds and touches nothing.
 * Device scratch is grow-only and kept by the context.  The documents are cut
 * into chunks of at most 2^20 documents and 2^22 (particle, token) cells (a
 * single document always fits: 1024 x 4096 = 2^22), so the scratch never
 * exceeds 16 MiB of topics + 32 MiB of probabilities + 12 bytes per token of
 * a chunk (ids and phat, <= 48 MiB) + 16 bytes per document of a chunk
 * (<= 16 MiB) + 8 Kp bytes: 112 MiB + 32 KiB, whatever Dh is.  Waits for the
 * context's stream. */
#define LDA_LTR_MAX_PARTICLES 1024
#define LDA_LTR_MAX_DOC_TOKENS 4096
lda_status lda_left_to_right(lda_ctx* ctx, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                             int32_t num_particles, int32_t resampling, uint64_t seed, double* doc_ll,
                             double* total, int64_t* tokens_scored, double* token_prob, int32_t* z_out);
/* Test hook: lda_left_to_right cuts its chunks at `cells` (particle, token)
 * cells instead of 2^22 (0 = the default; a document alone always fits). */
void lda_debug_ltr_chunk_cells(int64_t cells);

/* The readouts of a trained model, selected on the device.
 *
 * lda_top_words: ParallelTopicModel.printTopWords / displayTopWords' selection
 * [src/cmu_ron/TrainAndPredict.java:170] without the V x K table leaving the
 * device.  For each topic k < K (padded topics are never reported): the words
 * with nw[w,k] > 0 ordered by count descending, equal counts by ascending word
 * id (Mallet's IDSorter over an array in id order); the first n of them in
 * word_ids[k*n + i] and counts[k*n + i], i = 0 .. n-1.  Slots past the topic's
 * last nonzero word hold id -1 and count 0.  It reads the global counts this
 * shard holds (the int32 nw rows, V x Kp, kept for every sampler kind).
 * Integer compares only, no atomics: (count << 32) | (0xFFFFFFFF - w) is a
 * unique key per topic, so a topic's best n are one set however V is cut into
 * slabs, and a call repeats bit for bit.
 * Errors: LDA_ERR_INVALID_ARG for a NULL ctx or output, or n outside
 * [1, LDA_TOP_WORDS_MAX]; LDA_ERR_STATE with a pending delta (call lda_apply
 * first).
 * Device scratch is grow-only and kept by the context: the slab lists, at
 * most 1024 (slab, 64-topic group) waves x 64 topics x n keys of 8 bytes
 * (512 KiB x n: 32 MiB at n = 64; Kp x n x 8 bytes when V <= 256), and the
 * 8 K n bytes of the result, which is all that is copied to the host.  Waits
 * for the context's stream. */
#define LDA_TOP_WORDS_MAX 64
lda_status lda_top_words(lda_ctx* ctx, int32_t n, int32_t* word_ids /*[K*n]*/, int32_t* counts /*[K*n]*/);

/* lda_doc_top_topics: the m heaviest topics of documents of THIS shard,
 * printDocumentTopics' selection [src/cmu_ron/TrainAndPredict.java:232], from
 * the shard's current z on the device.  docs == NULL: documents
 * [doc_begin, doc_begin + M); else docs[M] shard-local ids in any order,
 * duplicates allowed (doc_begin must be 0), as lda_score_docs takes them.
 * For the j-th document the topics are ordered by the weight
 *     (alpha_k + n_dk) / (n_d + alphaSum)
 * descending, in fp64 with exactly that expression ((double) n_dk and
 * (double) n_d; alphaSum = alpha[0] + ... + alpha[K-1] added in that order in
 * fp64), equal weights by ascending topic id; topics[j*m + i] and the topic's
 * count n_dk in counts[j*m + i], i = 0 .. m-1.  With m > K the slots past K
 * hold topic -1 and count 0.  An empty document ranks by alpha alone.  The
 * device's quotient is IEEE-754 fp64 division (the library is built without
 * fast-math and with -ffp-contract=off), so the order is the one the same
 * expression gives on the host.  A document's row depends on that document
 * alone, not on M, docs or the chunks, and a call repeats bit for bit.
 * Errors: LDA_ERR_INVALID_ARG for a NULL ctx, m outside
 * [1, LDA_TOP_TOPICS_MAX], M < 0, a document id or range outside [0, D), a
 * list given with doc_begin != 0, or a NULL output with M > 0; LDA_ERR_STATE
 * with a pending delta.  M = 0 succeeds and touches nothing.
 * Device scratch is grow-only and kept by the context.  The documents are cut
 * into chunks of at most min(2^20, 2^23 / (2 m)) documents, so the scratch
 * never exceeds 32 MiB of results + 8 MiB of document ids (docs given),
 * whatever M is.  Waits for the context's stream. */
#define LDA_TOP_TOPICS_MAX 64
lda_status lda_doc_top_topics(lda_ctx* ctx, int32_t m, int64_t doc_begin, int64_t M, const int64_t* docs,
                              int32_t* topics /*[M*m]*/, int32_t* counts /*[M*m]*/);

/* lda_doc_counts: the dense topic counts of documents of THIS shard,
 * nd[j*K + k] = tokens of the j-th listed document with topic k (int32), from
 * the shard's current z on the device -- lda_get_counts' nd rows for a list of
 * documents.  doc_begin, M and docs as lda_doc_top_topics takes them (any
 * order, duplicates allowed).  Integer counts: a row depends on its document
 * alone and repeats bit for bit.
 * Errors: LDA_ERR_INVALID_ARG for a NULL ctx, M < 0, a document id or range
 * outside [0, D), a list given with doc_begin != 0, or a NULL nd with M > 0;
 * LDA_ERR_STATE with a pending delta.  M = 0 succeeds and touches nothing.
 * Device scratch is grow-only and kept by the context (shared with
 * lda_doc_top_topics).  The documents are cut into chunks of at most
 * min(2^20, max(1, 2^23 / K)) documents, so the scratch never exceeds 32 MiB
 * of rows + 8 MiB of document ids (docs given), whatever M is.  Waits for the
 * context's stream. */
lda_status lda_doc_counts(lda_ctx* ctx, int64_t doc_begin, int64_t M, const int64_t* docs, int32_t* nd /*[M*K]*/);

/* lda_topic_top_docs: the documents of THIS shard in which a topic is
 * heaviest -- the question Mallet's printTopicDocuments answers -- selected on
 * the device from the shard's current z.  For each topic
 * k < K (padded topics are never reported) the candidates are the documents d
 * with at least one token of the topic (n_dk > 0) and a length L_d >=
 * min_tokens.  They are ordered by the weight
 *     w(d,k) = ((double) n_dk + smoothing) / ((double) L_d + Ks)
 * descending, Ks = (double) K * smoothing formed once on the host, one
 * rounding per operation (IEEE fp64 division; the library is built without
 * fast-math and with -ffp-contract=off), equal weights by ascending document
 * id.  The first n candidates go to doc_ids[k*n + i] (shard-local id),
 * counts[k*n + i] = n_dk and lengths[k*n + i] = L_d, i = 0 .. n-1; slots past
 * the last candidate hold -1 / 0 / 0, so a topic without tokens is all -1.
 * 0 < w <= 1 always, so the weight's bit pattern orders as a uint64, and the
 * pair (weight bits descending, id ascending) is unique per topic: a topic's
 * best n are one set however the documents are cut into chunks and slabs, and
 * a call repeats bit for bit.  Integer and fp64 compares only, no atomics on
 * global memory.
 * This is this library's definition, not Mallet's: Mallet's sorted sets also
 * hold the documents with no token of the topic, ranked by the smoothing
 * alone; here a document that never shows a topic is not one of its top
 * documents, and a padded slot stays distinguishable.  With smoothing = 0
 * every one-topic document, one-token ones included, has weight 1.0;
 * min_tokens drops the short ones.
 * Errors, all checked on the host before any device work:
 * LDA_ERR_INVALID_ARG for a NULL ctx or output, n outside
 * [1, LDA_TOPIC_DOCS_MAX], smoothing negative or not finite, or
 * min_tokens < 1; LDA_ERR_STATE with a pending delta (call lda_apply first).
 * D = 0 succeeds with -1 / 0 / 0 everywhere.
 * Device scratch is grow-only and kept by the context, and its bound depends
 * on neither D nor N: the documents go through in chunks of at most
 * max(1, 2^23 / Kp) documents, whose dense rows take at most 32 MiB; the
 * (slab, topic) lists, at most 1024 (slab, 64-topic group) waves x 64 topics x
 * n entries of 20 bytes (1.25 MiB x n: 12.5 MiB at n = 10, 160 MiB at
 * n = 128), carried from chunk to chunk; and the 16 K n bytes of the result,
 * which is all that is copied to the host.  Waits once for the context's
 * stream. */
#define LDA_TOPIC_DOCS_MAX 128
lda_status lda_topic_top_docs(lda_ctx* ctx, int32_t n, double smoothing, int32_t min_tokens,
                              int64_t* doc_ids /*[K*n]*/, int32_t* counts /*[K*n]*/, int32_t* lengths /*[K*n]*/);
/* Test hook: lda_topic_top_docs cuts the documents into chunks of `docs`
 * documents instead of 2^23 / Kp (0 = the default). */
void lda_debug_topic_docs_chunk_docs(int64_t docs);

/* lda_topic_cooccurrence: which topics are used together in the same
 * documents of THIS shard, counted on the device from the shard's current z
 * (DESIGN.md §9l).  n_dk is document d's count of topic k, L_d its length.
 *   A document is USED when L_d >= min_tokens (min_tokens >= 1).
 *   Topic k is PRESENT in d when n_dk >= min_count and
 *       (double) n_dk >= min_prop * (double) L_d
 *   (min_count >= 1, 0 <= min_prop <= 1; one fp64 product and one compare).
 * Over the used documents:
 *   *docs_used  = their number
 *   tokens[k]   = N_k  = sum over d of n_dk
 *   present[k]  = C_k  = documents in which k is present
 *   codocs[k*K + l]  = C_kl = documents in which k and l are both present;
 *                      the diagonal is C_k
 *   overlap[k*K + l] = M_kl = sum over d of min(n_dk, n_dl); the diagonal is N_k
 *   product[k*K + l] = S_kl = sum over d of n_dk * n_dl; the diagonal is the
 *                      sum of n_dk^2
 * The three tables are full symmetric K x K, row-major; each is requested by
 * a non-NULL pointer, and only the requested ones are allocated and
 * accumulated.  overlap and product run over every nonzero topic of a used
 * document: the two presence thresholds apply to present and codocs only.
 * One wave per document; 64-bit integer adds only, so the result is a
 * function of z and does not depend on the grid or the order of arrival.  Up
 * to K = LDA_TOPIC_COOC_LDS_TOPICS a block accumulates the triangles in LDS
 * and adds its nonzero cells once; above, every pair is a global atomic.
 * Errors, checked on the host in this order before any device work:
 * LDA_ERR_INVALID_ARG for a NULL ctx, a NULL docs_used / tokens / present,
 * min_tokens < 1, min_count < 1, min_prop outside [0, 1] or NaN;
 * LDA_ERR_STATE with a pending delta (call lda_apply first);
 * LDA_ERR_UNSUPPORTED when product is requested and N * L_max >= 2^63 (N the
 * shard's tokens, L_max of lda_max_doc_length: the bound of a product cell).
 * D = 0 succeeds with zeros.  Changes no state of the context.
 * Device scratch is grow-only and kept by the context: 8 (1 + 2 K) bytes and
 * 8 K K bytes per requested table (128 MiB each at K = 4096), all of which is
 * copied to the host.  Waits once for the context's stream. */
#define LDA_TOPIC_COOC_LDS_TOPICS 64
lda_status lda_topic_cooccurrence(lda_ctx* ctx, int64_t min_tokens, int32_t min_count, double min_prop,
                                  int64_t* docs_used, int64_t* tokens /*[K]*/, int64_t* present /*[K]*/,
                                  int64_t* codocs /*[K*K] or NULL*/, int64_t* overlap /*[K*K] or NULL*/,
                                  int64_t* product /*[K*K] or NULL*/);
/* Test and measurement hook: on != 0 makes lda_topic_cooccurrence use global
 * atomics at every K (0 = the default, LDS up to LDA_TOPIC_COOC_LDS_TOPICS). */
void lda_debug_topic_cooccurrence_global(int32_t on);

/* lda_group_topics: how much of each group of documents is each topic, counted
 * on the device from the shard's current z.  doc_group[d], a
 * host array over THIS shard's documents, is document d's group in [-1, G);
 * -1 leaves the document out.  n_dk is document d's count of topic k, L_d its
 * length.  Used and present are lda_topic_cooccurrence's:
 *   A document is USED when its group is >= 0 and L_d >= min_tokens
 *   (min_tokens >= 1).
 *   Topic k is PRESENT in d when n_dk >= min_count and
 *       (double) n_dk >= min_prop * (double) L_d
 *   (min_count >= 1, 0 <= min_prop <= 1; one fp64 product and one compare).
 * Over the used documents of group g:
 *   group_docs[g]    = their number
 *   group_tokens[g]  = sum of L_d
 *   tokens[g*K + k]  = sum of n_dk
 *   present[g*K + k] = documents in which k is present
 *   shares[g*K + k]  = sum over d of floor(n_dk * 2^32 / L_d), one unsigned
 *                      64-bit integer division per nonzero (document, topic)
 * shares / (2^32 group_docs) is the document-weighted mean proportion of the
 * topic in the group, short by less than 2^-32 per document; it is kept in
 * fixed point so that every output is a function of z alone: 64-bit integer
 * adds only, whatever the grid and the order of arrival.  present and shares
 * are each requested by a non-NULL pointer, and only the requested tables are
 * allocated and accumulated.  One wave per document.  When group_docs,
 * group_tokens, the requested tables and the block's four wave histograms and
 * lists (24 Kp bytes) fit 64 KiB of LDS, a block accumulates them there and
 * adds its nonzero cells to global memory once; otherwise every add is a
 * global atomic (lda_group_topics_path says which).
 * Errors, checked on the host in this order before any device work:
 * LDA_ERR_INVALID_ARG for a NULL ctx, G < 1, a NULL group_docs / group_tokens
 * / tokens, min_tokens < 1, min_count < 1, min_prop outside [0, 1] or NaN, a
 * NULL doc_group with D > 0, a group id outside [-1, G) (the message names the
 * first such document); LDA_ERR_STATE with a pending delta (call lda_apply
 * first); LDA_ERR_UNSUPPORTED when G * K > LDA_GROUP_TOPICS_MAX_CELLS (2 GiB
 * per table) or when shares is requested with D >= 2^31 (a cell holds fewer
 * than 2^31 shares of at most 2^32).  D = 0 succeeds with zeros.  Changes no
 * state of the context.  Device scratch is grow-only and kept by the context:
 * 4 D bytes and 8 (2 G + tables G K) bytes, all of the latter copied to the
 * host.  Waits once for the context's stream. */
#define LDA_GROUP_TOPICS_MAX_CELLS (1 << 28)
lda_status lda_group_topics(lda_ctx* ctx, const int32_t* doc_group /*[D]*/, int32_t G, int64_t min_tokens,
                            int32_t min_count, double min_prop, int64_t* group_docs /*[G]*/,
                            int64_t* group_tokens /*[G]*/, int64_t* tokens /*[G*K]*/,
                            int64_t* present /*[G*K] or NULL*/, uint64_t* shares /*[G*K] or NULL*/);
/* Host only: the path lda_group_topics takes for G groups, K topics and
 * `tables` G x K tables (tokens and each requested one of present and shares:
 * 1 to 3): 1 = LDS accumulation, 0 = global atomics, -1 = a bad argument
 * (G < 1, K outside [1, LDA_MAX_TOPICS], tables outside [1, 3]).  *lds (may be
 * NULL) gets the dynamic LDS bytes of a block on that path. */
int32_t lda_group_topics_path(int32_t G, int32_t K, int32_t tables, int32_t* lds);
/* Test and measurement hook: on != 0 makes lda_group_topics use global atomics
 * at every shape (0 = the default, LDS where lda_group_topics_path says 1). */
void lda_debug_group_topics_global(int32_t on);

/* Sub-corpus topic words: each topic's top words inside a chosen set of
 * documents only.  A
 * context gets an optional sub-corpus table sub[V x Kp] of int32, allocated by
 * the first lda_subcorpus_count, kept until lda_subcorpus_release (or
 * lda_destroy) and never touched by sampling.  The table is a SNAPSHOT of z at
 * the time of the count: later sweeps neither update nor invalidate it.
 * lda_subcorpus_count: sub[w, k] becomes the number of tokens of word w with
 * topic k in the documents of THIS shard whose byte of doc_mask (a host array
 * [D]) is nonzero; accumulate = 0 zeroes the table first, accumulate != 0 adds
 * to what it holds (a table allocated by this call starts from zero either
 * way).  One wave per document; a masked-out document costs one load.  A cell
 * is bounded by the model's global count of (w, k), so int32 holds it.
 * LDA_ERR_INVALID_ARG for a NULL ctx or a NULL doc_mask with D > 0,
 * LDA_ERR_STATE with a pending delta; a failed allocation is
 * LDA_ERR_OUT_OF_MEMORY and leaves no table.  The table is complete when the
 * call returns.
 * lda_subcorpus_merge: sub(ctx) += sub(from), cell by cell; from is unchanged.
 * This is how the shards of one model add up exactly: the top n of a sum is
 * not a merge of the shards' top n, so the tables are added before selecting.
 * LDA_ERR_INVALID_ARG for a NULL ctx or from, from == ctx, or contexts that
 * differ in V or K; LDA_ERR_STATE with a pending delta on either or a missing
 * table on either.  The shards of one model cannot overflow a cell; a sum
 * above int32 between unrelated contexts wraps and is the caller's concern.
 * On one device it is one elementwise add; between devices from's table comes
 * over in chunks of a 64 MiB staging buffer by peer copies.
 * lda_subcorpus_top_words: lda_top_words' definition, ordering and padding
 * (count descending, equal counts by ascending word id, zero counts left out,
 * -1 / 0 past the last) applied to sub by the same kernels; totals[k] is the
 * sum of column k of sub (int64).  LDA_ERR_INVALID_ARG for a NULL ctx, n
 * outside [1, LDA_TOP_WORDS_MAX] or a NULL output; LDA_ERR_STATE with a
 * pending delta or without a table.
 * lda_subcorpus_release: frees the table (no table: nothing to do).
 * Each call waits once for the context's stream and changes nothing else. */
lda_status lda_subcorpus_count(lda_ctx* ctx, const uint8_t* doc_mask /*[D]*/, int32_t accumulate);
lda_status lda_subcorpus_merge(lda_ctx* ctx, lda_ctx* from);
lda_status lda_subcorpus_top_words(lda_ctx* ctx, int32_t n, int32_t* word_ids /*[K*n]*/, int32_t* counts /*[K*n]*/,
                                   int64_t* totals /*[K]*/);
lda_status lda_subcorpus_release(lda_ctx* ctx);

/* Relevance-ranked topic words, salient terms and word rows: what an LDAvis
 * view of a trained model shows, selected on the device from the global counts
 * this shard holds (the int32 nw rows, V x Kp, and nwsum), without the V x K
 * table leaving the device.  All fp64, one rounding per
 * operation (the library is built without fast-math and with
 * -ffp-contract=off):
 *     tw[w]        = sum over k < K of nw[w,k]                    (int64)
 *     N            = sum over k < K of nwsum[k]                   (int64)
 *     logprob(w,k) = log(((double) nw[w,k] + beta) / ((double) nwsum[k] + Vbeta)),
 *                    Vbeta = (double) V * beta
 *     logtp(w)     = log((double) tw[w] / (double) N)
 *     loglift(w,k) = logprob(w,k) - logtp(w)
 *     key(w,k,l)   = logprob(w,k) - m * logtp(w),  m = 1.0 - lambda_l
 * key is Sievert & Shirley's relevance lambda logprob + (1 - lambda) loglift
 * written with one product; at lambda = 1 it is logprob exactly.  log is the
 * device's fp64 log, which is not bit for bit the host libm's.
 *
 * lda_relevant_words: for each of L lambdas and each topic k < K (padded
 * topics are never reported) the candidates are the words with nw[w,k] > 0
 * (lda_top_words' candidates; tw > 0 follows), ordered by key descending,
 * equal keys by ascending word id.  The first n of them go to plane l, row k:
 * word_ids / counts (nw[w,k]) / totals (tw[w]) / logprob / loglift
 * [(l * K + k) * n + i], i = 0 .. n-1; slots past the last candidate hold
 * -1 / 0 / 0 / 0.0 / 0.0.  The same lambda may be passed more than once.
 * The key's bits are mapped to a uint64 of the same order (every bit of a
 * negative value flipped, else the sign bit set), and (key, word id) is unique
 * per topic, so a topic's best n are one set however V is cut into slabs.  A
 * lambda's plane is a function of that lambda, the table and (beta, V) alone:
 * not of L, of the lambda's position, of how many lambdas a pass handles (8 up
 * to n = 10, 4 up to n = 21, 2 up to n = 42, else 1: what 64 KiB of LDS hold
 * at 12 bytes x 64 topics x n per list) or of the slabs; a call repeats bit
 * for bit.  fp64 and integer compares only, no atomics.
 * Errors, checked on the host in this order before any device work:
 * LDA_ERR_INVALID_ARG for a NULL ctx, n outside [1, LDA_TOP_WORDS_MAX], L
 * outside [1, LDA_RELEVANCE_LAMBDAS_MAX], a NULL lambdas, a lambda that is not
 * finite or outside [0, 1], a NULL output; LDA_ERR_STATE with a pending delta
 * (call lda_apply first).  V = 0 succeeds with -1 / 0 / 0 / 0.0 / 0.0
 * everywhere.
 * Cost: ceil(L / lambdas per pass) passes over nw; a cell with nw > 0 costs
 * one division and one log per pass, a lambda a product, a difference and a
 * compare more.
 * Device scratch is grow-only and kept by the context.  tw and logtp take
 * 16 V bytes (1/(4 Kp) of the nw table); everything else has a bound that
 * depends on neither V nor N: the slab lists, at most 1024 (slab, 64-topic
 * group) waves x 64 KiB (64 MiB), and a pass's planes, 32 bytes x K x n x
 * lambdas per pass (at most 11 MiB), copied to the host pass by pass.  Waits
 * once for the context's stream.
 *
 * lda_salient_words: the n most salient words (Chuang et al. 2012).  For a
 * word with tw > 0
 *     distinctiveness(w) = sum over k < K with nw[w,k] > 0 of q log(q / p_k),
 *         q = (double) nw[w,k] / (double) tw[w],  p_k = (double) nwsum[k] / (double) N
 *     saliency(w)        = ((double) tw[w] / (double) N) * distinctiveness(w)
 * The sum is added in a fixed order that depends on the row alone: one wave
 * per word, lane l adds the terms of k = l, l + 64, ... in ascending order
 * from 0.0, then the 64 lane sums combine in the xor butterfly 32, 16, 8, 4,
 * 2, 1 (lda_topic_word_stats' order).  The candidates, the words with tw > 0,
 * are ordered by the saliency as computed, descending (a value a few ulp
 * below 0 orders as the number it is; -0.0 as 0.0), equal values by ascending
 * word id; the first n go to word_ids / totals (tw) / saliency /
 * distinctiveness [i], slots past the last candidate hold -1 / 0 / 0.0 / 0.0.
 * A call repeats bit for bit; no atomics.
 * Errors, in this order before any device work: LDA_ERR_INVALID_ARG for a
 * NULL ctx, n outside [1, LDA_SALIENT_WORDS_MAX], a NULL output;
 * LDA_ERR_STATE with a pending delta.  V = 0 succeeds with the empty slots.
 * Device scratch (shared with lda_relevant_words): tw, logtp and the
 * distinctiveness, 24 V bytes; the slabs' lists, at most 1024 slabs x n
 * entries of 12 bytes (3 MiB at n = 256), and the 24 n bytes of the result,
 * whatever V and N are.  Waits once for the context's stream.
 *
 * lda_word_rows: the unpadded nw rows and totals of M listed words,
 * rows[j*K + k] = nw[word_ids[j], k] (k < K) and totals[j] = tw[word_ids[j]];
 * the list in any order, duplicates allowed.
 * Errors, in this order before any device work: LDA_ERR_INVALID_ARG for a
 * NULL ctx, M < 0, a NULL list with M > 0, an id outside [0, V), a NULL output
 * with M > 0; LDA_ERR_STATE with a pending delta.  M = 0 then succeeds and
 * touches nothing.
 * The list goes through in chunks of at most max(1, 2^23 / K) rows, so the
 * scratch never exceeds 32 MiB of rows + 12 bytes per row of the chunk (ids
 * and totals), whatever M is.  Waits once for the context's stream. */
#define LDA_RELEVANCE_LAMBDAS_MAX 128
#define LDA_SALIENT_WORDS_MAX 256
lda_status lda_relevant_words(lda_ctx* ctx, int32_t n, int32_t L, const double* lambdas /*[L]*/,
                              int32_t* word_ids /*[L*K*n]*/, int32_t* counts /*[L*K*n]*/,
                              int64_t* totals /*[L*K*n]*/, double* logprob /*[L*K*n]*/,
                              double* loglift /*[L*K*n]*/);
lda_status lda_salient_words(lda_ctx* ctx, int32_t n, int32_t* word_ids /*[n]*/, int64_t* totals /*[n]*/,
                             double* saliency /*[n]*/, double* distinctiveness /*[n]*/);
lda_status lda_word_rows(lda_ctx* ctx, int64_t M, const int32_t* word_ids /*[M]*/, int32_t* rows /*[M*K]*/,
                         int64_t* totals /*[M]*/);
/* Test hook: lda_relevant_words cuts V into slabs of `rows` rows (more rows
 * where that would make more than 1024 slabs) instead of lda_top_words' cut,
 * and lda_salient_words takes its slabs through LDS in chunks of
 * min(rows, 1024) rows, four chunks to a slab, instead of one chunk of 1024
 * (0 = the defaults). */
void lda_debug_relevance_slab_rows(int64_t rows);

/* lda_topic_phrases: the most frequent same-topic token runs of every topic of
 * THIS shard -- the question Mallet's --xml-topic-phrase-report
 * (topicPhraseXMLReport) answers -- counted on the device from the shard's
 * words and current z.
 * A RUN is a maximal range of consecutive tokens [s, e) inside one document
 * with z[s] = ... = z[e-1] = k: it extends neither left nor right and never
 * crosses a document's end.  Its PHRASE is (k, words[s..e)).  A run qualifies
 * if min_len <= e - s <= max_len, 2 <= min_len <= max_len <=
 * LDA_PHRASE_LEN_MAX.  A run longer than max_len is not cut into pieces: it
 * counts toward *skipped_long and nothing else; a run shorter than min_len
 * counts toward nothing.  count(k, phrase) is the number of qualifying runs
 * with that topic and exactly that word sequence.
 * Per topic the phrases are ordered by count descending, equal counts by word
 * id sequence lexicographically ascending, a proper prefix before its
 * extension: a strict total order on content alone, so a topic's best n are
 * one set however the work is cut into passes, and a call repeats bit for bit.
 * For each topic k < K the first n phrases with count >= min_count go to
 * phrase_words[(k*n + i) * max_len + j] (-1 past the phrase's length),
 * lengths[k*n + i], counts[k*n + i] and first[k*n + i], the smallest
 * shard-local token index at which a qualifying run of the phrase starts;
 * empty slots hold words -1, length 0, count 0, first -1.  topic_runs[k] is
 * the topic's qualifying runs, topic_distinct[k] its distinct phrases before
 * min_count.
 * This is this library's definition, not Mallet's.  As recalled (Mallet is
 * not vendored; nothing is tested against it), Mallet 2.0.7's loop never
 * counts a run that reaches a document's last token and does not let the token
 * that closes a phrase start the next one; both are accidents of its state
 * machine and neither holds here.
 * The counts live in a device hash table (open addressing, linear probing,
 * one 64-bit key topic:12 | length-1:5 | start:47 and one 32-bit count per
 * slot; the key refers to the read-only words, so an insert is one
 * compare-and-swap, one add and one minimum, without a lock or a wait; every
 * probe sequence ends after `slots` steps).  The table has the smallest power
 * of two of slots >= 2 * (N / min_len), at most 2^28 (3 GiB, plus 1 GiB for
 * the selection); beyond that the runs are cut by their hash into passes, each
 * filling at most half the table from a count made beforehand, each followed
 * by a selection whose per-topic list carries over to the next; a phrase
 * lives in exactly one pass, so this is exact.
 * lda_phrase_counts: the exact count of each of Q given (topic, word
 * sequence) under the same definition, sequence q being
 * phrase_words[phrase_off[q] .. phrase_off[q+1]); a sequence never seen or of
 * a length outside [min_len, max_len] counts 0.  It builds the table the same
 * way, in the same passes, and keeps nothing from an earlier call.
 * lda_phrase_lookup is lda_phrase_counts that also returns, in first[q]
 * (NULL: not wanted), the smallest shard-local start of the phrase, -1 where
 * the count is 0: what a merge over shards needs.
 * Errors, all checked on the host before any device work:
 * LDA_ERR_INVALID_ARG for a NULL ctx or output, n outside
 * [1, LDA_PHRASES_MAX], limits outside 2 <= min_len <= max_len <=
 * LDA_PHRASE_LEN_MAX, min_count < 1, Q < 0, a query topic outside [0, K), a
 * word id outside [0, V), phrase_off[0] != 0 or a decreasing phrase_off;
 * LDA_ERR_STATE with a pending delta (call lda_apply first);
 * LDA_ERR_UNSUPPORTED for a shard of 2^32 or more tokens (the counts are 32
 * bits).  D = 0 or N = 0 succeeds with empty lists (all counts 0).
 * LDA_ERR_INTERNAL if a pass filled its table, which the pass cut rules out
 * unless one part alone holds more distinct phrases than half the slots.
 * Device scratch is grow-only and kept by the context.  Waits once for the
 * context's stream, and once more, for the per-part run counts, only when
 * N / min_len exceeds half the largest table (or the test hook is set). */
#define LDA_PHRASE_LEN_MAX 32
#define LDA_PHRASES_MAX 128
lda_status lda_topic_phrases(lda_ctx* ctx, int32_t n, int32_t min_len, int32_t max_len, int32_t min_count,
                             int32_t* phrase_words /*[K*n*max_len], -1 padded*/, int32_t* lengths /*[K*n]*/,
                             int64_t* counts /*[K*n]*/, int64_t* first /*[K*n]*/, int64_t* topic_runs /*[K]*/,
                             int64_t* topic_distinct /*[K]*/, int64_t* skipped_long);
lda_status lda_phrase_counts(lda_ctx* ctx, int32_t min_len, int32_t max_len, int64_t Q,
                             const int32_t* topics /*[Q]*/, const int64_t* phrase_off /*[Q+1]*/,
                             const int32_t* phrase_words, int64_t* counts /*[Q]*/);
lda_status lda_phrase_lookup(lda_ctx* ctx, int32_t min_len, int32_t max_len, int64_t Q,
                             const int32_t* topics /*[Q]*/, const int64_t* phrase_off /*[Q+1]*/,
                             const int32_t* phrase_words, int64_t* counts /*[Q]*/, int64_t* first /*[Q] or NULL*/);
/* Test hook: the phrase table has exactly `slots` slots (a power of two >= 2;
 * 0 or anything else = the default), so that small inputs take many passes. */
void lda_debug_phrase_table_slots(int64_t slots);

/* Topic diagnostics: the integer statistics behind per-topic coherence,
 * document entropy, rank-1 documents, allocation ratio / count, exclusivity
 * and the distances from the uniform and corpus distributions, counted on the
 * device.  The definitions follow Mallet's
 * TopicModelDiagnostics as this header states them; they are not pinned
 * against Mallet itself.
 *
 * Both calls take K word lists from the caller, word_ids[k*n + i], i < n,
 * 1 <= n <= LDA_DIAG_WORDS_MAX; a slot holding -1 is empty (anywhere in a
 * list).  lda_top_words' output is such a list, and so is any other.
 * Errors of both, all checked on the host before any device work:
 * LDA_ERR_INVALID_ARG for a NULL ctx, word_ids or output, n out of range, a
 * word id outside [-1, V), or the same id twice in one topic's list (a word
 * may stand in several topics' lists); LDA_ERR_STATE with a pending delta.
 * Device scratch is grow-only and kept by the context: the lists (4 K n
 * bytes), the lookup table (at most 4 MiB), the results (4 K n (n + 1) / 2 +
 * 8 K (2 + P) bytes: 34 MiB at K = 4096, n = 64; 28 K n + 8 K bytes for the
 * word statistics).  Each call waits once for the context's stream and
 * repeats bit for bit.
 *
 * lda_topic_codocuments: counted from THIS shard's documents and current z.
 * codoc: each topic's packed lower triangle, K * n (n + 1) / 2 int32; cell
 * (i, j), j <= i, of topic k at codoc[k * n (n + 1) / 2 + i (i + 1) / 2 + j]
 * = documents holding at least one token of word_ids[k, i] ASSIGNED TO TOPIC
 * k and at least one of word_ids[k, j] assigned to topic k.  The diagonal is
 * the word's document frequency under topic k; cells of an empty slot are 0.
 * doc_stats[k * (2 + P) + c], int64, per topic:
 *   c = 0: documents with n_dk > 0;
 *   c = 1: documents whose largest topic count is topic k's (equal counts go
 *          to the smallest topic id; an empty document counts for no topic);
 *   c = 2 + i: documents with n_dk > 0 and
 *          (alpha_k + (double) n_dk) / ((double) n_d + alphaSum) >= props[i],
 *          lda_doc_top_topics' fp64 expression and alphaSum (alpha added in
 *          topic order); the division is IEEE, so a weight equal to a
 *          threshold counts.
 * 0 <= P <= LDA_DIAG_PROPS_MAX; props strictly ascending in (0, 1], else
 * LDA_ERR_INVALID_ARG (props may be NULL when P = 0).  A shard of 2^31 or
 * more documents: LDA_ERR_UNSUPPORTED.  Everything is an integer count, so
 * the results are exact, independent of any order, and shards' results add.
 *
 * lda_topic_word_stats: from the global int32 nw rows and nwsum (the same on
 * every shard).  counts[k*n + i] = nw[w, k]; totals = sum over k' of
 * nw[w, k'] (int64); share_sums = sum over k' < K of
 * (beta + nw[w, k']) / (V beta + nwsum[k']) in fp64, V beta = (double) V *
 * beta, added in a fixed order: lane l = 0 .. 63 adds k' = l, l + 64, ...
 * ascending, then the 64 partial sums combine in a butterfly, x[l] += x[l ^ o]
 * for o = 32, 16, 8, 4, 2, 1.  sumsq[k] = sum over w of nw[w, k]^2 (uint64,
 * exact: it is at most nwsum[k]^2 < 2^63).  Empty slots give 0. */
#define LDA_DIAG_WORDS_MAX 64
#define LDA_DIAG_PROPS_MAX 8
lda_status lda_topic_codocuments(lda_ctx* ctx, int32_t n, const int32_t* word_ids /*[K*n]*/, int32_t P,
                                 const double* props /*[P]*/, int32_t* codoc /*[K*n(n+1)/2]*/,
                                 int64_t* doc_stats /*[K*(2+P)]*/);
lda_status lda_topic_word_stats(lda_ctx* ctx, int32_t n, const int32_t* word_ids /*[K*n]*/,
                                int32_t* counts /*[K*n]*/, int64_t* totals /*[K*n]*/,
                                double* share_sums /*[K*n]*/, uint64_t* sumsq /*[K]*/);

/* lda_word_cooccurrences: the counts behind reference-corpus topic coherence
 * (UMass, UCI / PMI, NPMI), by plain co-occurrence in a corpus, whatever the
 * tokens' topics.  word_ids are K lists as
 * lda_topic_codocuments takes them (1 <= n <= LDA_DIAG_WORDS_MAX, -1 = an
 * empty slot, no id twice in one list; a word may stand in any number of
 * topics' lists, at different slots).
 * The corpus: doc_off == NULL is THIS shard's own training documents, already
 * on the device (Dh and words are ignored); otherwise Dh documents in host
 * memory, document d's tokens words[doc_off[d] - doc_off[0] ..
 * doc_off[d + 1] - doc_off[0]), ids in [-1, V): -1 is a token outside the
 * alphabet, which keeps its position in a window and matches nothing.
 * The units: window == 0, every document with at least one token is one
 * unit; window == W >= 1, a document of L >= 1 tokens gives max(1, L - W + 1)
 * units, the token ranges [s, s + W) clipped to the document.  A document
 * without tokens is no unit.
 * cooc: one packed lower triangle per topic, int64, in lda_topic_codocuments'
 * layout: cell (i, j), j <= i, of topic k at cooc[k * n (n + 1) / 2 +
 * i (i + 1) / 2 + j] = units that hold a token of word_ids[k, i] and a token
 * of word_ids[k, j]; the diagonal is the units holding that one word; cells
 * of an empty slot are 0.  *units = the number of units.  Integer counts:
 * exact, independent of the grid, of the chunks and of Dh's other documents,
 * two corpora's results add, and a call repeats bit for bit.  The block
 * counters are 32-bit and moved to the 64-bit result before they can reach
 * 2^29, whatever the corpus.
 * The call reads neither z nor the counts: a pending delta is NOT an error,
 * and the call leaves all model state untouched.
 * Errors, all checked on the host before any device work:
 * LDA_ERR_INVALID_ARG for a NULL ctx, word_ids, cooc or units, n or the
 * lists as above, window outside [0, LDA_COOC_WINDOW_MAX], and with a host
 * corpus Dh < 0, a non-monotone doc_off, NULL words when there are tokens, or
 * an id outside [-1, V); LDA_ERR_UNSUPPORTED for K >= 2^25.  Dh = 0 succeeds
 * with zeros.
 * Device scratch is grow-only and kept by the context: the words' membership
 * rows (4 (V + 1) + 4 K n bytes), the result (8 K n (n + 1) / 2 bytes: 68 MiB
 * at K = 4096, n = 64), and for a host corpus one chunk of whole documents:
 * at most 2^23 tokens (32 MiB of ids; a single longer document goes alone and
 * takes 4 bytes per token) and 2^20 documents (8 MiB of offsets).  Waits for
 * the context's stream. */
#define LDA_COOC_WINDOW_MAX 256
lda_status lda_word_cooccurrences(lda_ctx* ctx, int32_t n, const int32_t* word_ids /*[K*n]*/, int32_t window,
                                  int64_t Dh, const int64_t* doc_off, const int32_t* words,
                                  int64_t* cooc /*[K*n(n+1)/2]*/, int64_t* units);
/* Test hook: lda_word_cooccurrences cuts a host corpus into chunks of at most
 * `tokens` tokens instead of 2^23 (0 = the default; a longer document goes
 * alone). */
void lda_debug_cooc_chunk_tokens(int64_t tokens);

/* Topic distances and nearest topics, within one model or between two, on the
 * device from the global int32 nw rows and nwsum.  other ==
 * NULL or other == ctx is SELF mode (K2 = K); else CROSS mode: topic a of ctx
 * against topic b of other, which must hold the same V (word ids must mean the
 * same words: aligning vocabularies is the caller's job) on the same device.
 * Each side's smoothed topic uses its own beta and nwsum,
 *     phi_k(w) = (nw[w,k] + beta) / (nwsum[k] + V beta),   V beta = (double) V * beta,
 * an IEEE fp64 division.  With p = phi_a of ctx and q = phi_b of other, sums
 * over the words w, natural logarithms, everything in fp64:
 *  LDA_TOPIC_COSINE     sum p q / sqrt(sum p^2 * sum q^2)       (a similarity)
 *  LDA_TOPIC_HELLINGER  sqrt(min(1, (1/2) sum (sqrt p - sqrt q)^2))
 *                       = sqrt(1 - sum sqrt p sqrt q), in [0, 1]
 *  LDA_TOPIC_JS         max(0, (1/2) [sum p ln p + sum q ln q
 *                                     - sum (p + q) ln((p + q) / 2)]),
 *                       Jensen-Shannon in nats, in [0, ln 2]
 *  LDA_TOPIC_KL         sum p ln p - sum p ln q = KL(p || q); row = p
 * (the Hellinger and Jensen-Shannon forms are chosen so that equal columns
 * give exactly 0, below).  out[a * K2 + b], a < K, b < K2; padded topics are
 * never reported.
 * Determinism.  The word rows are cut into slabs that are a function of
 * (V, K, K2) alone -- lda_topic_distance_slabs; never of the device: s =
 * max(1, min(ceil(V / 256), floor(LDA_TOPIC_SCRATCH_CAP_MIB MiB / (8 K K2)),
 * 64)), slab_rows = ceil(V / s), slabs = ceil(V / slab_rows).  Every sum (the
 * pair sums and the per-topic sums alike) adds a slab's rows in ascending
 * order from 0.0 and then the slabs in slab order; no floating-point atomics.
 * So a pair's value is a function of the two columns, the two (beta, nwsum)
 * and V alone, not of where the pair sits in the matrix: two topics with
 * identical columns (and equal nwsum) have bit-identical distances to every
 * third topic and distance exactly 0 (cosine exactly 1) to each other, and a
 * call repeats bit for bit.
 * Self mode: cosine, Hellinger and Jensen-Shannon are bit-symmetric by
 * construction (only pairs a < b are computed; (b, a) is a copy) and the
 * diagonal is set, not computed: 1 for cosine, 0 for the others, also for
 * Kullback-Leibler, whose other cells are as computed.
 * Cross mode: the kernels run on ctx's stream and read other's nw / nwsum
 * after waiting for other's stream; nothing of other is written.
 * Errors, checked in this order before any device work: LDA_ERR_INVALID_ARG
 * for a NULL ctx, a metric outside [0, 3], (nearest) n outside
 * [1, LDA_TOPIC_NEAREST_MAX], a NULL output, V differing between the two
 * contexts; LDA_ERR_UNSUPPORTED for contexts on different devices;
 * LDA_ERR_STATE with a pending delta on either side (call lda_apply first) or
 * V = 0.
 * Cost: V K K2 terms (half in self mode for the symmetric metrics), dense on
 * purpose.  Device scratch is grow-only and kept by ctx: the slabs' pair sums,
 * at most LDA_TOPIC_SCRATCH_CAP_MIB MiB (one 8 K K2-byte plane if that is
 * more: 128 MiB at K = K2 = 4096), the matrix (8 K K2 bytes) and the per-topic
 * sums (at most 65 x 16 (Kp + Kp2) bytes).  Waits for ctx's stream.
 *
 * lda_topic_nearest: the same matrix, kept on the device, and per row a the n
 * nearest topics b of the other side: value ascending (cosine: descending),
 * equal values by ascending topic id (-0.0 counts as 0.0); topics[a * n + i],
 * values[a * n + i] (the matrix's own bits).  In self mode topic a is not a
 * candidate of its own row.  With fewer than n candidates the tail holds id
 * -1 and value NaN.  Only the K n ids and values are copied to the host. */
#define LDA_TOPIC_COSINE 0
#define LDA_TOPIC_HELLINGER 1
#define LDA_TOPIC_JS 2
#define LDA_TOPIC_KL 3
#define LDA_TOPIC_NEAREST_MAX 64
#define LDA_TOPIC_SCRATCH_CAP_MIB 256
lda_status lda_topic_distances(lda_ctx* ctx, lda_ctx* other /* NULL = ctx itself */, int32_t metric,
                               double* out /* [K * K2], row a = topic a of ctx */);
lda_status lda_topic_nearest(lda_ctx* ctx, lda_ctx* other /* NULL = ctx itself */, int32_t metric, int32_t n,
                             int32_t* topics /* [K * n] */, double* values /* [K * n] */);
/* Host-only: the slabs lda_topic_distances cuts V word rows into for a K x K2
 * matrix (slab s holds rows [s * slab_rows, min(V, (s + 1) * slab_rows))). */
lda_status lda_topic_distance_slabs(int32_t V, int32_t K, int32_t K2, int32_t* slabs, int32_t* slab_rows);

/* ---- nearest documents --------------------------------------
 * Distances between topic distributions of documents, and per query the n
 * nearest documents of the shard, selected on the device: the document-side
 * sibling of lda_topic_distances / lda_topic_nearest, and lda_score_docs'
 * generalisation to more metrics.
 *
 * Candidate row.  Document d of ctx has the row
 *     p_d[k] = ((double) n_dk + alpha_k) / ((double) L_d + A),
 * n_dk from the shard's current z on the device, L_d its tokens, A = alpha[0]
 * + ... + alpha[K-1] added in that order (lda_doc_top_topics' A).
 * Query row.  Exactly one of theta / counts is given.
 *   theta:  fp64 rows [Q * K], checked as lda_score_docs checks them (finite,
 *           not negative, positive sum) and used as given; Hellinger and
 *           Jensen-Shannon are then the stated expressions of that row
 *           (distances when it sums to 1).
 *   counts: int32 rows c [Q * K], not negative, turned on the device into
 *           ((double) c_k + alpha_k) / ((double) sum c + A) with ctx's alpha:
 *           the candidate's expression, so a query with the counts of a
 *           candidate document is bit-identical to that candidate's row.
 * Metrics (the LDA_TOPIC_* numbers 0..2; Kullback-Leibler is not offered).
 * Everything is fp64, every sum over k runs in ascending k from 0.0, natural
 * logarithms, x ln x = 0 at x = 0, no fused multiply-add (-ffp-contract=off),
 * no floating-point atomics:
 *   cosine (0)          S = sum p q, P2 = sum p^2, Q2 = sum q^2
 *                       S / sqrt(P2 * Q2)                    larger is nearer
 *   Hellinger (1)       S = sum (sqrt p - sqrt q)^2
 *                       sqrt(min(1, S / 2))                  smaller is nearer
 *   Jensen-Shannon (2)  S = sum (p + q) ln((p + q) / 2), Hp = sum p ln p,
 *                       Hq = sum q ln q
 *                       max(0, ((Hp + Hq) - S) / 2)          smaller is nearer
 * Two bit-identical rows give exactly 0 (Hellinger, Jensen-Shannon) and
 * exactly 1 (cosine).  Every reported value gets + 0.0: no -0.0 appears.
 * Determinism.  A pair's value is a function of the two rows, K and the
 * metric alone: not of where the pair sits in a tile, of the chunks, of M or
 * Q, of the list order, of the shard's other documents or of the number of
 * shards.  A call repeats bit for bit.
 * Selection order.  Candidates are ordered by (value by the metric's order,
 * document id ascending); the fp64 bit pattern is made monotone as
 * lda_topic_nearest makes it.  Slots past the last candidate hold id -1 and
 * value NaN.
 *
 * lda_doc_distances: out[q * M + j] = the value between query q and document
 * docs[j] (or doc_begin + j), the documents addressed as lda_score_docs
 * addresses them (a range, or a list in any order, duplicates allowed, with
 * doc_begin = 0).
 * lda_doc_nearest: per query the n nearest of all the shard's documents with
 * L_d >= min_tokens, leaving out document skip[q] (-1: none; skip NULL: none):
 * doc_ids[q * n + i] (shard-local), values[q * n + i].  Only the Q n ids and
 * values come back.
 * lda_doc_neighbors: the queries are the shard's own documents docs[j] (or
 * doc_begin + j), their rows built on the device from z, each query's own id
 * left out.  Bit-identical to lda_doc_counts followed by
 * lda_doc_nearest(counts, skip = own id).
 * Errors, checked in this order before any device work: LDA_ERR_INVALID_ARG
 * for a NULL ctx ("null ctx"), a metric outside [0, 2] ("metric"), n outside
 * [1, LDA_DOC_NEAREST_MAX] ("n"), both or neither of theta / counts
 * ("theta / counts"), a NULL output with work to do ("null output"), Q < 0 or
 * M < 0 ("bad sizes"), a document id or range outside [0, D) ("document"),
 * min_tokens < 1 ("min_tokens"), a skip id outside [-1, D) ("skip"), a bad
 * theta row ("theta"), a negative count ("counts"); LDA_ERR_STATE with a
 * pending delta.  Q = 0 or M = 0 succeeds and touches nothing.
 * Cost: Q D K pair terms, dense on purpose (with alpha > 0 no p is zero).
 * Device scratch is grow-only, kept by ctx and bounded whatever Q and D are:
 * the work goes in chunks of at most 1024 queries by at most
 * min(2^23 / queries, 2^22 / K) candidates, so at most 64 MiB of chunk values,
 * 32 MiB of candidate rows, 32 MiB of query rows (each padded to a multiple
 * of 64 columns: at most 2 MiB more), 32 MiB of a query chunk's uploaded rows,
 * and under 2 MiB of sums, lengths, ids and lists.  Waits for ctx's stream. */
#define LDA_DOC_NEAREST_MAX 64
lda_status lda_doc_distances(lda_ctx* ctx, int32_t metric, int64_t Q, const double* theta /* [Q*K] or NULL */,
                             const int32_t* counts /* [Q*K] or NULL */, int64_t doc_begin, int64_t M,
                             const int64_t* docs /* [M] or NULL */, double* out /* [Q*M] */);
lda_status lda_doc_nearest(lda_ctx* ctx, int32_t metric, int32_t n, int64_t Q, const double* theta,
                           const int32_t* counts, const int64_t* skip /* [Q] or NULL */, int32_t min_tokens,
                           int64_t* doc_ids /* [Q*n] */, double* values /* [Q*n] */);
lda_status lda_doc_neighbors(lda_ctx* ctx, int32_t metric, int32_t n, int64_t doc_begin, int64_t M,
                             const int64_t* docs /* [M] or NULL */, int32_t min_tokens, int64_t* doc_ids /* [M*n] */,
                             double* values /* [M*n] */);
/* Test hook: at most `docs` candidates and `queries` queries per chunk (0 =
 * the default of each), so that small tests run the second trip of every
 * chunk loop and the merge of the running lists. */
void lda_debug_doc_nearest_chunk(int64_t docs, int64_t queries);

/* Mallet-layout adapter: typeTopicCounts as packed (count << topic_bits) |
 * topic rows sorted descending, rows[row_off[w] .. row_off[w+1]) with
 * row_off[V+1]; row length = min(K, typeTotal[w]) exactly as Mallet allocates
 * it, trailing cells 0.  Pass rows = NULL to get row_off / total / topic_bits
 * only. */
lda_status lda_to_mallet_packed(lda_ctx* ctx, int32_t* rows, int64_t* row_off,
                                int32_t* topic_bits);

/* ---- hyperparameter optimisation ----------------------
 * Mallet 2.0.7 ParallelTopicModel.optimizeAlpha / optimizeBeta, enabled by
 * setOptimizeInterval(20) [src/cmu_ron/TrainAndPredict.java:163,
 * src/cmu/TrainAndPredict.java:261].  The GPU builds the integer statistics;
 * the fp64 fixed-point updates run on the host. */

/* Longest document of this shard (sizes the histograms below). */
lda_status lda_max_doc_length(lda_ctx* ctx, int32_t* max_len);
/* WorkerRunnable's alpha statistics from the current z of this shard, ADDED
 * into caller buffers (accumulate over the sampled sweeps, sum across ranks):
 * doc_len_counts[max_len+1]: documents of each length (docLengthCounts);
 * topic_doc_counts[K*(max_len+1)], row k: documents in which topic k has
 * each count > 0 (topicDocCounts).  max_len >= lda_max_doc_length. */
lda_status lda_doc_topic_histograms(lda_ctx* ctx, int32_t max_len, int32_t* doc_len_counts,
                                    int32_t* topic_doc_counts);
/* The same statistics summed on the device over several sweeps without a
 * host round trip: _accumulate adds the current z's histograms into the
 * context's own buffer, _take ADDS the sum into the caller's buffers and
 * zeroes it, _clear zeroes it.  max_len must stay the same between takes. */
lda_status lda_doc_topic_histograms_accumulate(lda_ctx* ctx, int32_t max_len);
lda_status lda_doc_topic_histograms_take(lda_ctx* ctx, int32_t max_len, int32_t* doc_len_counts,
                                         int32_t* topic_doc_counts);
lda_status lda_doc_topic_histograms_clear(lda_ctx* ctx);
/* optimizeBeta's countHistogram, ADDED into count_hist[max_count+1]: cells
 * (w, k) of the global nw holding each count c > 0 (identical on every rank:
 * do not sum it across ranks).  LDA_ERR_INVALID_ARG if a cell exceeds
 * max_count (the largest word total bounds every cell). */
lda_status lda_count_histogram(lda_ctx* ctx, int64_t max_count, int32_t* count_hist);
/* One optimisation step's statistics with a single wait on the stream (the
 * three calls above and lda_get_counts' nwsum each wait on their own): the
 * accumulated document histograms ADDED and zeroed as _take (when
 * doc_len_counts / topic_doc_counts are non-null), the count histogram ADDED
 * (count_hist non-null), nwsum[K] copied (non-null).  Each output is optional.
 * Replaces the per-statistic round trips of ParallelTopicModel.estimate()'s
 * optimizeAlpha / optimizeBeta (ParallelTopicModel.java 2.0.7). */
lda_status lda_hyper_statistics(lda_ctx* ctx, int32_t max_len, int32_t* doc_len_counts,
                                int32_t* topic_doc_counts, int64_t max_count, int32_t* count_hist,
                                int32_t* nwsum);

/* Dirichlet.learnParameters(params, observations, observationLengths, shape,
 * scale, iterations): Minka's fixed point with a Gamma(shape, scale) prior;
 * params[K] updated in place, params_sum = their new sum.  Host-only. */
lda_status lda_learn_parameters(double* params, int32_t K, const int32_t* observations,
                                const int32_t* observation_lengths, int32_t max_len, double shape,
                                double scale, int32_t iterations, double* params_sum);
/* Dirichlet.learnSymmetricConcentration(countHistogram, observationLengths,
 * numDimensions, currentValue): 200 fixed-point steps for a symmetric
 * Dirichlet's total concentration.  count_hist[max_count+1]; the observation
 * length histogram is given sparsely as ascending (lengths[j], length_counts[j])
 * pairs (topic sizes reach ~1e9 at C4).  Host-only. */
lda_status lda_learn_symmetric_concentration(const int32_t* count_hist, int64_t max_count,
                                             const int64_t* lengths, const int32_t* length_counts,
                                             int64_t n_lengths, int32_t num_dims, double current,
                                             double* out);
/* Dirichlet.digamma (the series the estimators use).  Host-only. */
double lda_digamma(double z);

/* Token-weighted mean number of nonzero topics in a token's word row of the
 * current (global) snapshot: sum_w n_w * nnz(nw[w]) / sum_w n_w.  The sparse
 * samplers read 4 bytes per such entry (SURVEY.md §8d's B_sparse). */
lda_status lda_row_stats(lda_ctx* ctx, double* mean_row_nnz);

/* Kernel-level timing of the last lda_sample (ms, HIP events on the
 * context's stream). */
lda_status lda_last_sample_ms(lda_ctx* ctx, float* ms);
/* Kernel durations (ms, oldest first) of the last n = min(max, launches, 256)
 * lda_sample calls: bench.py reads the launches of its timed region. */
lda_status lda_sample_times(lda_ctx* ctx, int32_t max, float* ms, int32_t* n);
/* The same for the recount kernel that follows each sampler launch in the
 * recount mode (0 ms in the delta mode). */
lda_status lda_recount_times(lda_ctx* ctx, int32_t max, float* ms, int32_t* n);

/* Diagnostics: the sampler's own uniform draws on the current device.
 * out[i] = word 0 of Philox4x32-10 with counter {gtok[i] lo, gtok[i] hi, c2,
 * c3} and key {seed lo, seed hi} -- the x0 every kernel draws (c2 = sweep,
 * c3 = stream: 0 sample, 1 init, 2 inference).  Used to pin the device RNG
 * against rocRAND's philox4x32_10 (tests/native/philox_vs_rocrand.hip). */
lda_status lda_philox_draws(uint64_t seed, uint32_t c2, uint32_t c3, const int64_t* gtok, int64_t n,
                            uint32_t* out);

const char* lda_last_error(void);
/* Test hook: the nth host allocation of a caller-sized buffer on this thread
 * (counted from this call; 0 = off) fails with std::bad_alloc, which the
 * entry point reports as LDA_ERR_OUT_OF_MEMORY (tests/test_abi_guard*.py). */
void lda_debug_fail_host_alloc(int32_t nth);
/* "lda_mi355x <version> (gfx950; ABI <n>)".  ABI history: 2 -- lda_infer's
 * last three ints became (num_iterations, thinning, burn_in), Mallet's
 * getSampledDistribution order (was (n_iter, burn_in, thin)); 3 -- the dense
 * samplers' exchange buffer holds recounted counts (lda_count_update_mode),
 * lda_recount_times, lda_set_exchange_parts' reserve_cus < 0 = default; 4 --
 * lda_hyper_statistics, lda_set_alpha_beta returns without waiting for the
 * stream (its upload is asynchronous); 5 -- warm-start parts are interleaved
 * segments of the corpus (LDA_WARM_BLOCKS), lda_warm_part_tokens; 6 -- the
 * large-K sampler's draw (C >= 32: exact fixed-point doc part, own-entry
 * accept / re-draw), sequential sweeps recount under LDA_COUNT_RECOUNT,
 * lda_exchange_unpack_lists, lda_counts_checksum; 7 -- lda_set_exchange_cells
 * (four 8-bit cells per packed word); 8 -- lda_score_docs.
 * lda_heldout_loglik and lda_doc_completion, then lda_top_words,
 * lda_doc_top_topics and lda_doc_counts, then lda_topic_codocuments and
 * lda_topic_word_stats, then lda_left_to_right (with its test hook
 * lda_debug_ltr_chunk_cells), then lda_topic_distances, lda_topic_nearest
 * and lda_topic_distance_slabs, then lda_word_cooccurrences (with its test
 * hook lda_debug_cooc_chunk_tokens), then lda_topic_top_docs (with its test
 * hook lda_debug_topic_docs_chunk_docs), then lda_topic_phrases,
 * lda_phrase_counts and lda_phrase_lookup (with their test hook
 * lda_debug_phrase_table_slots), then lda_relevant_words, lda_salient_words
 * and lda_word_rows (with their test hook lda_debug_relevance_slab_rows), then
 * lda_topic_cooccurrence (with its test hook
 * lda_debug_topic_cooccurrence_global), then lda_group_topics (with
 * lda_group_topics_path and its test hook lda_debug_group_topics_global) and
 * lda_subcorpus_count, lda_subcorpus_merge, lda_subcorpus_top_words and
 * lda_subcorpus_release, then lda_doc_distances, lda_doc_nearest and
 * lda_doc_neighbors (with their test hook lda_debug_doc_nearest_chunk) came
 * later and only add symbols, so the version stays 8. */
#define LDA_ABI_VERSION 8
const char* lda_version(void);
int32_t lda_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LDA_MI355X_H */
