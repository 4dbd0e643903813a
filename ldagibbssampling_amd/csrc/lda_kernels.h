// lda_kernels.h — internal interface between the C-ABI runtime
// (lda_capi.cpp) and the gfx950 kernels (lda_kernels.hip).  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lda {

// Philox counter word 3: which stream a draw belongs to.
constexpr uint32_t STREAM_SAMPLE = 0u;
constexpr uint32_t STREAM_INIT = 1u;
constexpr uint32_t STREAM_INFER = 2u;
constexpr uint32_t STREAM_LTR = 3u;     // lda_left_to_right; the particle sits in bits 8 and up

// Row-prefetch depth of the sampler per C = Kp/64 (tokens in flight per wave;
// C = 8: P = 3 is +1% over 2 on C4 once the pipeline waits vmcnt(P-1), P = 4
// spills; C = 16: 3 is within noise of 2).
#ifndef SAMPLE_P1
#define SAMPLE_P1 4
#endif
#ifndef SAMPLE_P2
#define SAMPLE_P2 4
#endif
#ifndef SAMPLE_P4
#define SAMPLE_P4 4
#endif
#ifndef SAMPLE_P8
#define SAMPLE_P8 3
#endif
#ifndef SAMPLE_P16
#define SAMPLE_P16 2
#endif
// half-wave dense sampler (K <= 128, two documents per wave): tokens in flight
#ifndef SAMPLE_PH
#define SAMPLE_PH 4
#endif
#ifndef SAMPLE_PQ
#define SAMPLE_PQ 4
#endif
// sparse sampler: tokens in flight, 64-entry rounds prefetched per token
#ifndef SPARSE_P
#define SPARSE_P 4
#endif
#ifndef SPARSE_R0
#define SPARSE_R0 2
#endif

// Per-sweep tables of the large-K sampler (k_big_tables, oracle
// exact_big_tables): the fixed-point exponent S, sum_k G_k, beta 2^-S, 2^S / beta.
struct BigScal {
  int32_t S;
  float bsig;               // beta 2^-S
  uint64_t S0;
  float bsig_hi;            // beta 2^(32-S)
  int32_t pad;
  double isig;              // 2^S / beta
};
struct BigTables {
  float2* tab;              // [Kp] {inv, ainv = alpha * inv}
  float4* tab_m1;           // [Kp] {inv_m1, alpha * inv_m1, bits of big_fix(inv_m1), bits of
                            //  big_fix(alpha inv_m1) - big_fix(alpha inv)} (0 for a topic with no tokens)
  uint32_t* F;              // [Kp] big_fix(inv)
  uint64_t* pfx;            // [Kp] inclusive prefix of big_fix(ainv)
  BigScal* scal;
};

struct SampleParams {
  const int32_t* words;     // [N] token stream (doc-contiguous)
  int32_t* z;               // [N] topic of each token (read old, write new)
  const int64_t* doc_off;   // [D+1]
  const int64_t* range_doc; // [R] work range r starts at document range_doc[r]
  const int64_t* range_end; // [R] ... and ends before range_end[r] (range_doc + 1: contiguous ranges)
  int64_t num_ranges;
  int32_t* queue;           // range counter, zeroed before each launch
  const int32_t* nw;        // [V*Kp] snapshot
  int32_t* delta;           // [V*Kp] pending nw delta
  int32_t* dsum;            // [Kp]   pending nwsum delta
  const float* alpha;       // [Kp]
  const float* inv;         // [Kp]   1/(nwsum + V*beta)
  const float* inv_m1;      // [Kp]   1/(nwsum - 1 + V*beta)
  float beta;
  int32_t K;
  int64_t token_base;       // Philox counter offset (global token index)
  uint32_t k0, k1;          // Philox key (seed)
  uint32_t c2, c3;          // Philox counter words 2 (sweep) and 3 (stream)
  // sparse rows of the snapshot (k_sample_sparse only)
  const uint32_t* ent;      // packed (count << 12) | topic, count saturated at 0xFFFFF
  const int64_t* row_off;   // [V+1] capacity offsets (min(Kp, word total) per row)
  const int32_t* row_nnz;   // [V] live entries per row; sign bit: the row has a saturated count
  const uint32_t* row_rnd;  // [V] row_off / 64 (rows start on whole 64-entry rounds)
  float* trace;             // debug only: 8 floats per token when non-null
  // 16-bit copy of the snapshot rows (k_sample)
  const uint16_t* nw16;     // [V*Kp] counts, clamped at 65535
  const uint8_t* wide;      // [V] 1 when the row holds a count > 65535 (read nw)
  // graph-launched sweeps (lda_sweep), dense kernels: [0] the sweep counter
  // (Philox word 2), which each sweep's apply advances, [1] beta's fp32 bits,
  // read from device memory in place of c2 / beta
  const uint32_t* state_dev;
  // recount sweeps of the quarter-wave sampler: the word-ordered copy of z
  // (zw[zpos[i]] = z[i], the recount index's order) kept current by the
  // sampler, so the recount streams it instead of gathering z through perm
  int32_t* zw;
  const uint32_t* zpos;
  // the large-K sampler's per-sweep tables (k_sample_big)
  BigTables big;
};

// Tokens [tok[i], tok[i+1]) of a shard belong to exchange part i.
struct PartSpans {
  int64_t tok[5];
  int32_t parts;
};
// Recount work item size: a word with more tokens in a part is split over
// several items (its row then takes device atomics).
constexpr int32_t RECOUNT_ITEM_TOKENS = 1024;

// Sparse-row packing: 12 topic bits (K <= 4096), 20 count bits; a saturated
// count field means "read the exact count from the dense nw row".
constexpr uint32_t ENT_TOPIC_BITS = 12;
constexpr uint32_t ENT_TOPIC_MASK = (1u << ENT_TOPIC_BITS) - 1;
constexpr uint32_t ENT_COUNT_SAT = (1u << (32 - ENT_TOPIC_BITS)) - 1;

// half: 1 = the half-wave variant k_sample_half, 2 = the quarter-wave
// k_sample_quarter (C <= 2 only; lda_capi.cpp: LDA_DENSE_HALF), 0 = k_sample<C>
hipError_t launch_sample(int C, bool frozen, const SampleParams& p, int blocks, hipStream_t st,
                         int half = 0);
int sample_blocks_per_cu(int C, bool frozen, int K, int half = 0);
int half_topics_per_lane(int K);
int quarter_topics_per_lane(int K);
// rb: the large-K sampler's ring (C >= 32): 0 the default depth, nonzero
// the short one for short rows (SB_RB_SHORT_ROUNDS below)
hipError_t launch_sample_sparse(int C, bool frozen, const SampleParams& p, int blocks,
                                hipStream_t st, int rb = 0);
constexpr int SB_RB_SHORT_ROUNDS = 6;   // the short ring's register rounds
int sample_sparse_blocks_per_cu(int C, bool frozen);
// row totals of nw (saturating at Kp) -> host prefix -> capacity offsets
hipError_t launch_row_caps(const int32_t* nw, int64_t V, int32_t Kp, int32_t* caps, hipStream_t st);
hipError_t launch_build_sparse(const int32_t* nw, int64_t V, int32_t Kp, const int64_t* row_off,
                               uint32_t* ent, int32_t* row_nnz, hipStream_t st);
// the sparse samplers' apply + row build in one pass (rows already sized:
// build_row_capacity): nw += delta, delta = 0, dsum += the delta's column
// sums, the sparse entries and row_nnz of every row
hipError_t launch_apply_build(int32_t* nw, int32_t* delta, int64_t V, int32_t Kp, const int64_t* row_off,
                              uint32_t* ent, int32_t* row_nnz, int32_t* dsum, hipStream_t st);
// the large-K sampler's tables from the topic tables (after every k_prepare_topics)
hipError_t launch_big_tables(const int32_t* nwsum, const float* alpha_f, const float* inv, const float* inv_m1,
                             int32_t K, int32_t Kp, float beta, const BigTables& t, hipStream_t st);
hipError_t launch_build_packed(const int32_t* nw, int64_t V, int32_t Kp, uint16_t* nw16,
                               uint8_t* wide, hipStream_t st);
// per-topic state refreshed by an apply (k_prepare_topics' arguments)
struct TopicTables {
  int32_t* nwsum;           // [Kp]
  const double* alpha;      // [K]
  float* alpha_f;           // [Kp]
  float* inv;               // [Kp]
  float* inv_m1;            // [Kp]
  float vbeta;              // (float)(V * beta)
  int32_t K;
  int32_t* queue;           // work-queue counter zeroed for the next sample (nullable)
  int32_t absolute;         // 1: the buffer holds recounted counts that replace nw / nwsum
  uint32_t* state_dev;      // graph-launched sweeps: [0] advanced by one, [2] vbeta's fp32 bits read in place of vbeta
  int32_t advance;          // with state_dev: 1 = this apply ends a sweep (advance [0]); 0 = a part's apply inside one
};
// dense sampler's apply: nw += delta, delta = 0, 16-bit rows + wide flags,
// nwsum/tables (k_apply + k_build_packed + k_prepare_topics in one launch)
hipError_t launch_apply_packed(int32_t* nw, int32_t* delta, int64_t V, int32_t Kp, uint16_t* nw16,
                               uint8_t* wide, const TopicTables& t, hipStream_t st);
// the recount (see k_recount): index build and the per-sweep recount
hipError_t launch_word_hist(const int32_t* words, int64_t n, const PartSpans& ps, int64_t V,
                            uint32_t* cnt, hipStream_t st);
hipError_t launch_word_scatter(const int32_t* words, int64_t n, const PartSpans& ps, int64_t V,
                               uint32_t* cursor, uint32_t* perm, hipStream_t st);
// zpos[perm[j]] = j; zw[j] = z[perm[j]] (the word-ordered copy of z)
hipError_t launch_zw_build(const uint32_t* perm, int64_t n, const int32_t* z, uint32_t* zpos, int32_t* zw,
                           hipStream_t st);
// zw non-null: the topics are read from zw[perm index] (streamed) instead of z[perm[.]]
hipError_t launch_recount(int32_t Kp, const uint32_t* perm, const int32_t* zw, const int32_t* items, int32_t n_items,
                          const int32_t* z, int32_t* buf, int32_t* bufsum, int blocks, hipStream_t st);
hipError_t launch_philox_draws(const int64_t* gtok, int64_t n, uint32_t c2, uint32_t c3, uint64_t seed,
                               uint32_t* out, hipStream_t st);
hipError_t launch_init_z(int32_t* z, int64_t n, int32_t K, int64_t token_base, uint32_t k0,
                         uint32_t k1, hipStream_t st);
hipError_t launch_count(const int32_t* words, const int32_t* z, int64_t n, int32_t Kp,
                        int32_t* delta, int32_t* dsum, hipStream_t st);
hipError_t launch_apply(int32_t* nw, int32_t* delta, int64_t n, hipStream_t st);
// dst += src; src = 0 over n int32 (n a multiple of 4): a split sweep's parts
// sparse samplers' apply: nw += delta, delta = 0, dsum += the delta's column
// sums (dsum must hold only what is to be added: the caller zeroes it)
hipError_t launch_apply_cols(int32_t* nw, int32_t* delta, int64_t V, int32_t Kp, int32_t* dsum,
                             hipStream_t st);
// compact exchange (lda_exchange_pack / _unpack): 2 cells per int32 word,
// biases b0 = 2^15 / world (bits 0..15) and b1 = 2^14 / world (bits 16..30)
inline int32_t exch_bias0(int32_t world) { return 32768 / world; }
inline int32_t exch_bias1(int32_t world) { return 16384 / world; }
// ... or 4 cells per word (lda_set_exchange_cells 4, round 6): cells 4i..4i+2
// biased by 2^7 / world in bits 0..7, 8..15, 16..23, cell 4i+3 by 2^6 / world
// in bits 24..30 (world <= 64)
inline int32_t exch_bias4(int32_t world) { return 128 / world; }
inline int32_t exch_bias4_top(int32_t world) { return 64 / world; }
// cells: a multiple of 4; packed: cells / per_word words; esc: [1 + 3 cap] with esc[0] zeroed
hipError_t launch_exch_pack(const int32_t* buf, int64_t cells, int32_t* packed, int32_t world,
                            int32_t* esc, int32_t cap, hipStream_t st, int32_t per_word = 2);
// buf[cells] = the unpacked sum, then + every rank's escapes (esc_all: world x
// [1 + 3 cap]; nullptr: none)
hipError_t launch_exch_unpack(const int32_t* packed, int64_t cells, int32_t* buf, int32_t world,
                              const int32_t* esc_all, int32_t cap, hipStream_t st, int32_t per_word = 2);
// one uint64 partial per block of the nw / nwsum hash (lda_counts_checksum)
hipError_t launch_counts_checksum(const int32_t* nw, const int32_t* nwsum, int32_t K, int32_t Kp, int64_t V,
                                  uint64_t* partial, int blocks, hipStream_t st);
hipError_t launch_fold_delta(int32_t* dst, int32_t* src, int64_t n, hipStream_t st);
hipError_t launch_prepare_topics(int32_t* nwsum, int32_t* dsum, const double* alpha, double beta,
                                 double vbeta, int32_t K, int32_t Kp, float* alpha_f, float* inv,
                                 float* inv_m1, hipStream_t st);
hipError_t launch_doc_topics(const int32_t* z, const int64_t* doc_off, int64_t D, int32_t K,
                             int32_t Kp, int32_t* out, int accumulate, hipStream_t st);
hipError_t launch_ll_docs(const int32_t* z, const int64_t* doc_off, int64_t D, const double* alpha,
                          double alpha_sum, int32_t K, int32_t Kp, double* partial, int blocks,
                          hipStream_t st);
hipError_t launch_ll_words(const int32_t* nw, int64_t V, int32_t K, int32_t Kp, double beta,
                           double* partial, unsigned long long* nonzero, int blocks,
                           hipStream_t st);
// lda_score_docs (k_doc_scores): one register tile of nq <= DOC_SCORE_TILE
// queries against M documents
constexpr int DOC_SCORE_TILE = 16;
constexpr int DOC_SCORE_TILE_SMALL = 4;   // the tile for nq <= 4
struct DocScoreArgs {
  const int32_t* z;
  const int64_t* doc_off;
  const int64_t* docs;      // [M] shard-local document ids, or null: doc_begin + j
  int64_t doc_begin, M;
  const double* alpha;      // [K]
  const double* theta;      // [K * T] transposed tile, theta[k * T + t] (T the tile's width,
                            // rows t >= nq zero), 16-byte aligned
  const double* qconst;     // [2 nq]: alpha . theta_q, |theta_q|^2 per query of the tile
  int32_t nq, K, Kp, metric;
  double a2, A;             // sum alpha^2, sum alpha
  double* out;              // out[t * ldo + j], t < nq, j < M
  int64_t ldo;
};
hipError_t launch_doc_scores(const DocScoreArgs& a, int blocks, hipStream_t st);
// lda_top_words: stage 1 (k_top_words_slab) keeps, per (slab of rows, topic),
// the slab's best n keys (count << 32 | 0xFFFFFFFF - word) as a descending
// list, lists[((slab * G + group) * n + i) * 64 + lane] (G = Kp / 64, empty
// slots 0); stage 2 (k_top_words_merge) merges a topic's slab lists into
// ids / counts [K * n].  slabs <= TOP_WORDS_MAX_SLABS.
constexpr int TOP_WORDS_MAX_SLABS = 1024;
struct TopWordsArgs {
  const int32_t* nw;             // [V * Kp]
  int32_t V, K, Kp, n;
  int32_t slabs, slab_rows;      // slab s holds rows [s * slab_rows, min(V, (s + 1) * slab_rows))
  unsigned long long* lists;     // [slabs * Kp * n]
  int32_t* ids;                  // [K * n]
  int32_t* counts;               // [K * n]
};
hipError_t launch_top_words(const TopWordsArgs& a, hipStream_t st);
// lda_doc_counts (k_doc_counts) and lda_doc_top_topics (k_doc_top_topics): M
// listed documents of the shard, one wave per document
struct DocReadoutArgs {
  const int32_t* z;
  const int64_t* doc_off;
  const int64_t* docs;      // [M] shard-local document ids, or null: doc_begin + j
  int64_t doc_begin, M;
  const double* alpha;      // [K]
  double A;                 // alpha[0] + ... + alpha[K-1], added in that order
  int32_t K, Kp, m;
  int32_t* topics;          // k_doc_top_topics: [M * m]; k_doc_counts: the rows [M * K]
  int32_t* counts;          // k_doc_top_topics: [M * m]
};
hipError_t launch_doc_counts(const DocReadoutArgs& a, int blocks, hipStream_t st);
hipError_t launch_doc_top_topics(const DocReadoutArgs& a, int blocks, hipStream_t st);
// lda_topic_top_docs: the shard's documents go through in chunks.  Per chunk,
// k_topic_docs_count writes the chunk's dense rows [M * Kp] and
// k_topic_docs_slab folds them into the (slab, topic) lists: the descending
// best n of every topic among the documents slab s has seen so far, as
// weight bits / ids / counts at [((slab * G + group) * n + i) * 64 + lane]
// (G = Kp / 64; bits 0 = an empty slot).  Slab s of a chunk is its documents
// [s * slab_docs, min(M, (s + 1) * slab_docs)); slabs and slab_docs are those
// of the first chunk (first != 0: the lists start empty), a shorter last
// chunk leaves its trailing slabs untouched.  k_topic_docs_merge then merges
// a topic's slab lists into out_* [K * n].  slabs <= TOPIC_DOCS_MAX_SLABS.
constexpr int TOPIC_DOCS_MAX = 128;
constexpr int TOPIC_DOCS_MAX_SLABS = 1024;
struct TopicDocsArgs {
  const int32_t* z;
  const int64_t* doc_off;
  int64_t doc_begin, M;          // the chunk: documents [doc_begin, doc_begin + M) of the shard
  int64_t slab_docs;
  int32_t K, Kp, n, min_tokens;
  int32_t slabs, first;
  double smoothing, Ks;          // Ks = (double) K * smoothing
  int32_t* rows;                 // [M * Kp]
  unsigned long long* bits;      // [slabs * Kp * n]
  int64_t* ids;                  // [slabs * Kp * n]
  int32_t* cnts;                 // [slabs * Kp * n]
  int64_t* out_ids;              // [K * n]
  int32_t* out_counts;           // [K * n]
  int32_t* out_lengths;          // [K * n]
};
hipError_t launch_topic_docs_chunk(const TopicDocsArgs& a, int blocks, hipStream_t st);
hipError_t launch_topic_docs_merge(const TopicDocsArgs& a, hipStream_t st);
// lda_topic_codocuments, the co-document count (k_codoc): grid (document
// slabs, topic groups); a block keeps the packed triangles of its
// group_topics topics in LDS, a wave takes a document, marks the listed words
// it holds under each topic of the group in a 64-bit mask per topic and adds
// the masks' pairs into the triangles; the block adds its nonzero cells to
// codoc (zeroed by the caller) once at the end.  (word, topic) -> slot goes
// through an open-addressing table keyed w * Kp + k: entry
// ((key + 1) << 6) | slot, 0 = empty, linear probing from
// codoc_hash(key) & table_mask; at most half full, so a probe ends.
constexpr int DIAG_WORDS_MAX = 64;
constexpr int DIAG_PROPS_MAX = 8;
constexpr size_t CODOC_LDS_BYTES = 64 * 1024;
// topics per group of a block of `waves` waves: a mask per wave (8 bytes
// each) and a triangle per topic
constexpr int codoc_group_topics(int K, int n, int waves) {
  const int per = 8 * waves + 4 * (n * (n + 1) / 2), g = (int)(CODOC_LDS_BYTES / per);
  return g < K ? g : K;
}
constexpr uint64_t codoc_hash(uint64_t key) { return (key * 0x9E3779B97F4A7C15ull) >> 32; }
struct CodocArgs {
  const int32_t* words;
  const int32_t* z;
  const int64_t* doc_off;
  int64_t D;
  const unsigned long long* table;   // [table_mask + 1]
  uint32_t table_mask;
  int32_t K, Kp, n, group_topics;
  int32_t* codoc;                    // [K * n (n + 1) / 2], zeroed
};
hipError_t launch_codoc(const CodocArgs& a, int slabs, int waves, hipStream_t st);
// lda_topic_codocuments' document statistics (k_doc_diag): one wave per
// document, the counts in the per-wave LDS histogram, read back through the
// document's own tokens.  stats[k * (2 + P) + c] (zeroed by the caller); the
// increments go through per-block LDS counters when lds_counters is set (the
// launcher sets it when 16 Kp + 4 K (2 + P) bytes fit 64 KiB), else straight
// to stats.
struct DocDiagArgs {
  const int32_t* z;
  const int64_t* doc_off;
  int64_t D;
  const double* alpha;      // [K]
  double A;                 // alpha[0] + ... + alpha[K-1], added in that order
  double props[DIAG_PROPS_MAX];   // ascending; props[i >= P] unused
  int32_t K, Kp, P, lds_counters;
  unsigned long long* stats;
};
hipError_t launch_doc_diag(DocDiagArgs a, int blocks, hipStream_t st);
// lda_topic_word_stats: k_word_stats, one wave per listed word (cell of
// ids[K * n]); k_sumsq, the column sums of nw squared (sumsq zeroed by the
// caller, slabs x Kp / 64 one-wave blocks adding one integer per column).
struct WordStatsArgs {
  const int32_t* nw;        // [V * Kp]
  const int32_t* nwsum;     // [Kp]
  const int32_t* ids;       // [K * n], -1 = empty
  int32_t V, K, Kp, n;
  double beta, vbeta;
  int32_t slabs, slab_rows;
  int32_t* counts;                 // [K * n]
  long long* totals;               // [K * n]
  double* share_sums;              // [K * n]
  unsigned long long* sumsq;       // [K], zeroed
};
hipError_t launch_word_stats(const WordStatsArgs& a, hipStream_t st);
// lda_word_cooccurrences (k_cooc): units of a corpus that hold
// two listed words, whatever their topics.  A word's memberships are a CSR
// row: mem[moff[w] .. moff[w + 1]) = (topic << 6) | slot, ascending (so by
// topic).  Grid (slabs, topic groups), `waves` waves per block; a wave takes a
// tile of up to 64 units -- 64 consecutive documents (window == 0) or 64
// consecutive window starts of one document -- and keeps, per (topic of the
// group, slot), the 64-bit mask of the tile's units that hold the word: a
// token of document j sets bit j; a token at position q of a window tile sets
// the starts [q - window + 1, q].  Cell (i, j) then grows by
// popcount(mask i & mask j).  LDS: per wave a slot mask per topic and the unit
// masks [Gt (n + 1)] of 8 bytes, and the block's int32 triangles [Gt][T].
constexpr size_t COOC_LDS_BYTES = 64 * 1024;
constexpr int COOC_WAVES = 4;
// a wave moves the block's triangles to the result whenever it has counted
// this many units since it last did: a cell then holds less than COOC_WAVES x
// (COOC_FLUSH_UNITS + 64) = 2^28 + 256 at any time, whatever the corpus
constexpr int32_t COOC_FLUSH_UNITS = 1 << 26;
constexpr int cooc_group_topics(int K, int n, int waves) {
  const int per = 8 * waves * (n + 1) + 4 * (n * (n + 1) / 2), g = (int)(COOC_LDS_BYTES / per);
  return g < K ? g : K;
}
struct CoocArgs {
  const int32_t* words;              // ids in [-1, V); -1 matches nothing
  const int64_t* doc_off;            // [D + 1] into words
  int64_t D;
  const int32_t* moff;               // [V + 1]
  const int32_t* mem;                // [moff[V]]
  int32_t K, n, window, group_topics;
  unsigned long long* out;           // [K * n (n + 1) / 2], zeroed by the caller before the first launch
};
hipError_t launch_cooc(const CoocArgs& a, int slabs, hipStream_t st);
// lda_heldout_loglik (k_doc_completion): the scored tokens of Dh held-out
// documents against the int32 nw rows.  A wave takes a document's tokens in
// batches of doc_completion_batch(C): 64 up to C = 8, 16 above (the batch's
// fp64 partial sums are registers beside the lane's C values of u_d).
constexpr int doc_completion_batch(int C) { return C <= 8 ? 64 : 16; }
struct DocCompletionArgs {
  const int32_t* nw;        // [V * Kp]
  const double* inv;        // [Kp]: 1 / (nwsum[k] + V beta), 0 past K (launch_heldout_inv)
  const double* theta;      // [Dh * K]
  const int64_t* doc_off;   // [Dh + 1] into words
  const int32_t* words;     // every id in [0, V)
  double* out;              // [Dh]
  int64_t Dh;
  int32_t K, Kp;
  double beta;
};
hipError_t launch_heldout_inv(const int32_t* nwsum, double vbeta, int32_t K, int32_t Kp, double* inv,
                              hipStream_t st);
hipError_t launch_doc_completion(const DocCompletionArgs& a, int blocks, hipStream_t st);
// lda_left_to_right: k_left_to_right, one wave per (document,
// particle) of a chunk, job = d * R + r, writes the particle's topics z[r * N +
// t] and probabilities p[r * N + t]; k_ltr_reduce, one wave per document,
// averages them into phat[N] and sums the logs into ll[D].  words holds -1 for
// a skipped token (a type without training tokens): no draw, z = -1, p = 0.
// The uniform of a draw is Philox counter {g lo, g hi, limit, STREAM_LTR |
// (r << 8)} with g = g0 + the token's index in the chunk.
struct LeftToRightArgs {
  const int32_t* nw;        // [V * Kp]
  const double* inv;        // [Kp] (launch_heldout_inv)
  const double* alpha;      // [K]
  const int64_t* doc_off;   // [D + 1] into words
  const int32_t* words;     // [N], -1 = skipped
  int32_t* z;               // [R * N]
  double* p;                // [R * N]
  double* phat;             // [N]
  double* ll;               // [D]
  int64_t D, N, g0;
  int32_t R, resampling, K, Kp;
  double beta, A;           // A = alpha[0] + ... + alpha[K-1], added in that order
  uint32_t k0, k1;          // Philox key (seed)
};
hipError_t launch_left_to_right(const LeftToRightArgs& a, hipStream_t st);
hipError_t launch_ltr_reduce(const LeftToRightArgs& a, hipStream_t st);
// lda_topic_distances / lda_topic_nearest.  Side A is the
// calling context (topic a = row of the result), side B the other one (the
// same arrays in self mode).  phi = (nw + beta) / (nwsum + vbeta), an IEEE
// division, in every kernel that forms it.  The rows are cut into `slabs`
// slabs of slab_rows rows, the same cut for the per-topic sums and the pairs;
// within a slab every sum adds its rows in ascending order from 0.0, and the
// slabs are added in slab order, so a sum over the same values is the same
// bits wherever it is computed.
//  k_topic_sums          grid (slabs, Kp / 64), lane per topic: the slab's
//                        sum of phi^2 and of phi ln phi,
//                        sums[(slab * 2 + which) * Kp + k]
//  k_topic_sums_reduce   tot[which * Kp + k] = the slabs added in order
//  k_topic_pairs<metric> grid (b tiles, a tiles, slabs), 256 threads: a 64 x
//                        64 tile of pairs over one slab, TOPIC_PAIR_ROWS rows
//                        at a time through LDS, a 4 x 4 fp64 register tile
//                        per thread (a = ty + 16 i, b = tx + 16 j); the
//                        slab's sums go to part[(slab * K + a) * K2 + b].
//                        With `upper` set (self mode, symmetric metric) the
//                        tiles below the diagonal are not computed.
//  k_topic_dist_final    one thread per cell: adds the slabs in order and
//                        closes the metric; with `upper` the cell (a, b),
//                        a > b, is computed from the sums of (b, a), and in
//                        self mode the diagonal is set (1 for cosine, else 0)
//  k_topic_nearest       one wave per row of the matrix: n rounds of a
//                        wave-wide minimum over (order key, topic id)
// The term summed over the words and the closing expression per metric:
//  cosine     p q                 S / sqrt(sum p^2 * sum q^2)
//  Hellinger  (sqrt p - sqrt q)^2 sqrt(min(1, S / 2))
//  JS         (p + q) ln((p+q)/2) max(0, (sum p ln p + sum q ln q - S) / 2)
//  KL         p ln q              sum p ln p - S
constexpr int TOPIC_COSINE = 0, TOPIC_HELLINGER = 1, TOPIC_JS = 2, TOPIC_KL = 3;
constexpr int TOPIC_PAIR_ROWS = 32;
constexpr int TOPIC_MAX_SLABS = 64;
struct TopicSumsArgs {
  const int32_t* nw;        // [V * Kp]
  const int32_t* nwsum;     // [Kp]
  int32_t V, Kp;
  double beta, vbeta;
  int32_t slabs, slab_rows;
  double* sums;             // [slabs * 2 * Kp]
  double* tot;              // [2 * Kp]
};
hipError_t launch_topic_sums(const TopicSumsArgs& a, hipStream_t st);
struct TopicPairArgs {
  const int32_t *nw_a, *nwsum_a, *nw_b, *nwsum_b;
  int32_t V, K, Kp, K2, Kp2, metric;
  double beta_a, vbeta_a, beta_b, vbeta_b;
  int32_t slabs, slab_rows;
  int32_t self, upper;      // self mode; only the tiles on and above the diagonal
  double* part;             // [slabs * K * K2]
  const double* tot_a;      // [2 * Kp]
  const double* tot_b;      // [2 * Kp2]
  double* out;              // [K * K2]
};
hipError_t launch_topic_pairs(const TopicPairArgs& a, hipStream_t st);
hipError_t launch_topic_dist_final(const TopicPairArgs& a, hipStream_t st);
struct TopicNearestArgs {
  const double* mat;        // [K * K2]
  int32_t K, K2, n, self, descending;
  int32_t* topics;          // [K * n]
  double* values;           // [K * n]
};
hipError_t launch_topic_nearest(const TopicNearestArgs& a, hipStream_t st);
// lda_doc_distances / lda_doc_nearest / lda_doc_neighbors:
// k_topic_pairs with the roles turned -- the topics are the summed axis, the
// documents the columns.  A side's rows live transposed in scratch,
// rows[k * ld + j] for column j < ld (ld a multiple of 64, the columns past M
// zero), holding p (sqrt p for Hellinger), so a tile's row segment is one
// coalesced load.  The metrics are TOPIC_COSINE / _HELLINGER / _JS above.
//  k_doc_rows        one wave per column.  source DOC_ROWS_Z: document
//                    docs[j] (or doc_begin + j) of the shard, its counts in
//                    the per-wave LDS histogram of k_doc_counts, p = ((double)
//                    n_dk + alpha_k) / ((double) L_d + A), and lens[j] = L_d
//                    when lens is given; DOC_ROWS_COUNTS: the same expression
//                    of a caller's int32 row (L = its integer sum);
//                    DOC_ROWS_THETA: a caller's fp64 row as given
//  k_doc_row_sums    one thread per column: sum of x^2 (cosine) or of x ln x
//                    (JS; 0 at x = 0) over k ascending from 0.0, sums[j]
//  k_doc_pairs<m>    grid (candidate tiles, query tiles), 256 threads: a 64 x
//                    64 tile of pairs, TOPIC_PAIR_ROWS topics at a time
//                    through LDS, a 4 x 4 fp64 register tile per thread, each
//                    pair's sum one chain over k ascending; closes the metric
//                    and writes out[q * ldo + j] (+ 0.0) for q < Q, j < M
//  k_doc_select      one wave per query: folds the chunk's values into the
//                    query's running best-n list.  Candidates are ordered by
//                    (monotone key of the value, document id); round i takes
//                    the smallest pair above round i - 1's among the chunk's
//                    columns that pass the filter (lens[j] >= min_tokens,
//                    id_begin + j != skip[q]) and the old list, and writes
//                    slot i of the new list (id -1, value NaN when exhausted)
constexpr int DOC_ROWS_Z = 0, DOC_ROWS_COUNTS = 1, DOC_ROWS_THETA = 2;
constexpr int DOC_NEAREST_MAX = 64;
struct DocRowsArgs {
  int32_t source, metric;
  const int32_t* z;         // DOC_ROWS_Z
  const int64_t* doc_off;
  const int64_t* docs;      // [M] shard-local ids, or null: doc_begin + j
  int64_t doc_begin;
  const int32_t* counts;    // DOC_ROWS_COUNTS: [M * K]
  const double* theta;      // DOC_ROWS_THETA: [M * K]
  const double* alpha;      // [K]
  double A;                 // alpha[0] + ... + alpha[K-1], added in that order
  int64_t M, ld;            // columns filled, columns of the buffer (M <= ld)
  int32_t K, Kp;
  double* rows;             // [K * ld]
  double* sums;             // [ld]
  int32_t* lens;            // [ld] or null
};
hipError_t launch_doc_rows(const DocRowsArgs& a, int blocks, hipStream_t st);
struct DocPairArgs {
  const double *qrows, *crows;   // [K * qld], [K * cld]
  const double *qsums, *csums;   // [qld], [cld]
  int64_t Q, M, qld, cld, ldo;
  int32_t K, metric;
  double* out;                   // [Q * ldo]
};
hipError_t launch_doc_pairs(const DocPairArgs& a, hipStream_t st);
struct DocSelectArgs {
  const double* vals;            // [Q * ldv]
  int64_t Q, M, ldv, id_begin;
  const int32_t* lens;           // [M]
  const int64_t* skip;           // [Q], -1 = none
  int32_t n, min_tokens, descending, first;   // first: the old list is empty
  const int64_t* in_ids;         // [Q * n]
  const double* in_vals;
  int64_t* out_ids;              // [Q * n]
  double* out_vals;
};
hipError_t launch_doc_select(const DocSelectArgs& a, hipStream_t st);
// range workers per block of the sampler kernel used for (C, sampler): 4
// waves, 16 for the large-K sparse kernel (C >= 32), 8 for the half-wave
// dense kernel (4 waves x 2 halves)
int sample_waves_per_block(int C, bool sparse, int half = 0);
hipError_t launch_row_stats(const int32_t* nw, int64_t V, int32_t K, int32_t Kp,
                            unsigned long long* out, hipStream_t st);
hipError_t launch_doc_hist(const int32_t* z, const int64_t* doc_off, int64_t D, int32_t K, int32_t Kp,
                           int32_t L, int32_t* len_hist, int32_t* topic_hist, hipStream_t st);
hipError_t launch_count_hist(const int32_t* nw, int64_t V, int32_t K, int32_t Kp, int64_t max_count,
                             int32_t* hist, int32_t* overflow, hipStream_t st);
hipError_t launch_infer_init(const int32_t* words, int32_t* z, int64_t n, const int32_t* nw,
                             int32_t K, int32_t Kp, hipStream_t st);

// lda_topic_phrases / lda_phrase_counts.  A run is a maximal
// range of consecutive tokens of one document with one topic; it qualifies
// with min_len <= length <= max_len.  Every pass over the runs recomputes
// them from z and doc_off: a wave takes a document, a lane a token, the lane
// of a run's first token walks at most max_len further tokens.  No pass keeps
// a list of runs.
//   launch_phrase_scan    counts per topic the qualifying runs, the runs
//                         longer than max_len, and per hash part (the top
//                         PHRASE_PART_BITS bits of a run's 64-bit hash) the
//                         qualifying runs, from which the host cuts the passes
//   launch_phrase_insert  inserts the qualifying runs whose part lies in
//                         [part_lo, part_hi) into the table: open addressing,
//                         linear probing, slots a power of two, a slot one
//                         64-bit key (topic : 12 | length - 1 : 5 | start :
//                         47; all ones = empty) and one 32-bit count.  An
//                         empty slot is claimed by one 64-bit compare-and-swap;
//                         an occupied one is compared by content through the
//                         read-only words at its start, so nothing waits for
//                         another lane.  A match adds 1 and takes the minimum
//                         key, that is the smallest start.  A probe sequence
//                         ends after `slots` steps and sets flag[0].
//   launch_phrase_select  the pass's selection: a per-topic histogram of
//                         min(count, PHRASE_HIST_CAP) and the topic's distinct
//                         phrases; per topic the largest threshold >= min_count
//                         with n phrases at or above it and the bucket offsets;
//                         the scatter of the slots at or above the threshold;
//                         then one wave per topic folds its bucket into the
//                         topic's carried best-n list (sel_key / sel_cnt /
//                         sel_len; first != 0: the lists start empty) by
//                         count descending, then word sequence ascending, a
//                         prefix before its extension.
//   launch_phrase_gather  the lists as words / lengths / counts / starts
//   launch_phrase_lookup  one probe sequence per query (topic, word sequence)
//                         whose part lies in the pass
constexpr int PHRASE_LEN_MAX = 32;
constexpr int PHRASES_MAX = 128;
constexpr int PHRASE_TOPIC_BITS = 12, PHRASE_LEN_BITS = 5, PHRASE_START_BITS = 47;
constexpr int PHRASE_PART_BITS = 12;
constexpr int PHRASE_PARTS = 1 << PHRASE_PART_BITS;
constexpr int PHRASE_HIST_CAP = 256;
constexpr unsigned long long PHRASE_EMPTY = ~0ull;
static_assert(PHRASE_TOPIC_BITS + PHRASE_LEN_BITS + PHRASE_START_BITS == 64, "the key is one 64-bit word");
static_assert((1 << PHRASE_LEN_BITS) >= PHRASE_LEN_MAX, "length - 1 fits its field");
struct PhraseArgs {
  const int32_t* words;
  const int32_t* z;
  const int64_t* doc_off;
  int64_t D;
  int32_t K, n, min_len, max_len, min_count;
  int32_t part_lo, part_hi, first;
  int64_t slots;                     // a power of two
  unsigned long long* keys;          // [slots]
  uint32_t* cnts;                    // [slots]
  uint32_t* cand;                    // [slots]: the slots scattered into per-topic buckets
  uint32_t* part_runs;               // [PHRASE_PARTS]
  unsigned long long* topic_runs;    // [K]
  unsigned long long* topic_distinct;// [K]
  unsigned long long* skipped_long;  // [1]
  uint32_t* flag;                    // [1]: a probe sequence found the table full
  uint32_t* hist;                    // [K * PHRASE_HIST_CAP]
  uint32_t* thr;                     // [K]
  uint32_t* bucket_off;              // [K]
  uint32_t* cursor;                  // [K]
  unsigned long long* sel_key;       // [K * n]
  uint32_t* sel_cnt;                 // [K * n]
  int32_t* sel_len;                  // [K]
  int32_t* out_words;                // [K * n * max_len]
  int32_t* out_lengths;              // [K * n]
  long long* out_counts;             // [K * n]
  long long* out_first;              // [K * n]
  // lookup
  int64_t Q;
  const int32_t* q_topics;           // [Q]
  const int64_t* q_off;              // [Q + 1]
  const int32_t* q_words;
  long long* q_counts;               // [Q], zeroed by the caller
  long long* q_first;                // [Q], -1 by the caller
};
hipError_t launch_phrase_scan(const PhraseArgs& a, int blocks, hipStream_t st);
hipError_t launch_phrase_insert(const PhraseArgs& a, int blocks, hipStream_t st);
hipError_t launch_phrase_select(const PhraseArgs& a, int blocks, hipStream_t st);
hipError_t launch_phrase_gather(const PhraseArgs& a, hipStream_t st);
hipError_t launch_phrase_lookup(const PhraseArgs& a, hipStream_t st);

// ---- lda_relevant_words / lda_salient_words / lda_word_rows
// k_word_totals: one wave per word row, tw[w] = the row's integer sum over
// k < K, logtp[w] = log((double) tw / (double) N) (0.0 where tw = 0) and, with
// dist non-null, the word's distinctiveness; N = nwsum[0] + ... + nwsum[K-1]
// comes from k_token_total (ntot[0]).
// lda_relevant_words: a pass handles `batch` (1, 2, 4 or 8) lambdas.  Stage 1
// (k_relevant_slab) keeps, per (slab of rows, topic, lambda of the pass), the
// slab's best n (key, word) as a descending list,
// keys / ids[((((slab * G + group) * batch + j) * n + i) * 64 + lane]
// (G = Kp / 64, key 0 = an empty slot); stage 2 (k_relevant_merge, grid
// (K, batch)) merges a topic's slab lists and writes plane j of the pass:
// out_*[(j * K + k) * n + i].  slabs <= RELEVANCE_MAX_SLABS.
constexpr int RELEVANCE_MAX_SLABS = 1024;
constexpr int RELEVANCE_BATCH_MAX = 8;
constexpr size_t RELEVANCE_LDS_BYTES = 64 * 1024;
constexpr int RELEVANCE_ENTRY_BYTES = 12;   // the key's 8 and the word id's 4
// the lambdas a wave keeps at once: the largest of 8, 4, 2, 1 whose lists
// (n x 64 entries each) fit RELEVANCE_LDS_BYTES -- 8 up to n = 10, 4 up to
// n = 21, 2 up to n = 42, else 1
constexpr int relevance_batch(int n) {
  int b = RELEVANCE_BATCH_MAX;
  while (b > 1 && (size_t)b * (size_t)n * 64 * RELEVANCE_ENTRY_BYTES > RELEVANCE_LDS_BYTES) b >>= 1;
  return b;
}
struct RelevanceArgs {
  const int32_t* nw;             // [V * Kp]
  const int32_t* nwsum;          // [Kp]
  int32_t V, K, Kp, n;
  int32_t slabs, slab_rows;      // slab s holds rows [s * slab_rows, min(V, (s + 1) * slab_rows))
  int32_t batch;
  double beta, vbeta;
  double m[RELEVANCE_BATCH_MAX]; // 1.0 - lambda of the pass's lists
  long long* ntot;               // [1]
  long long* tw;                 // [V]
  double* logtp;                 // [V]
  double* dist;                  // [V] or null
  unsigned long long* keys;      // [slabs * Kp * batch * n]
  int32_t* ids;                  // [slabs * Kp * batch * n]
  int32_t* out_ids;              // [batch * K * n]
  int32_t* out_counts;           // [batch * K * n]
  long long* out_totals;         // [batch * K * n]
  double* out_logprob;           // [batch * K * n]
  double* out_loglift;           // [batch * K * n]
};
hipError_t launch_word_totals(const RelevanceArgs& a, hipStream_t st);
hipError_t launch_relevant_pass(const RelevanceArgs& a, hipStream_t st);
// lda_salient_words: k_salient_slab, one wave per slab of rows, keeps the
// slab's best n (saliency key, word) in keys / ids[slab * n + i], descending;
// k_salient_merge (one wave) merges them into out_*[n].
// slabs <= SALIENT_MAX_SLABS, n <= SALIENT_MAX.
constexpr int SALIENT_MAX = 256;
constexpr int SALIENT_MAX_SLABS = 1024;
constexpr int SALIENT_CHUNK_ROWS = 1024;
struct SalientArgs {
  const long long* ntot;         // [1]
  const long long* tw;           // [V]
  const double* dist;            // [V]
  int32_t V, n, slabs, slab_rows;
  int32_t chunk_rows;            // rows per LDS chunk, 1 .. SALIENT_CHUNK_ROWS
  unsigned long long* keys;      // [slabs * n]
  int32_t* ids;                  // [slabs * n]
  int32_t* out_ids;              // [n]
  long long* out_totals;         // [n]
  double* out_saliency;          // [n]
  double* out_dist;              // [n]
};
hipError_t launch_salient(const SalientArgs& a, hipStream_t st);
// lda_word_rows: k_word_rows, one wave per listed word: its unpadded row and
// its total.
struct WordRowsArgs {
  const int32_t* nw;             // [V * Kp]
  const int32_t* ids;            // [M]
  int64_t M;
  int32_t K, Kp;
  int32_t* rows;                 // [M * K]
  long long* totals;             // [M]
};
hipError_t launch_word_rows(const WordRowsArgs& a, hipStream_t st);
// lda_topic_cooccurrence: k_topic_cooc, one wave per document
// of at least min_tokens tokens, builds the document's topic counts in its LDS
// histogram, compacts the distinct topics into a 16-bit LDS list of m entries
// and spreads the m (m + 1) / 2 pairs (i <= j) over its lanes.  Topic k is
// present when n_dk >= min_count and (double) n_dk >= min_prop * (double) L_d.
// head = docs_used, tokens[K], present[K]; each non-NULL table gets, at cell
// (min(k, l), max(k, l)) of its K x K rows, 1 when both are present (codocs),
// min(n_dk, n_dl) (overlap), n_dk * n_dl (product).  Only the upper triangle
// is written: k_topic_cooc_mirror copies it below the diagonal.  Everything
// must be zero before the launch.  With lds != 0 (K <= TOPIC_COOC_LDS_TOPICS)
// a block keeps the head and the packed triangles of the requested tables in
// LDS as 64-bit cells and adds its nonzero cells once at its end; otherwise
// every add is a global 64-bit integer atomic.
constexpr int TOPIC_COOC_LDS_TOPICS = 64;
struct TopicCoocArgs {
  const int32_t* z;
  const int64_t* doc_off;
  int64_t D, min_tokens;
  double min_prop;
  int32_t min_count, K, Kp;
  unsigned long long* head;      // [1 + 2 K]
  unsigned long long* codocs;    // [K * K] or NULL
  unsigned long long* overlap;   // [K * K] or NULL
  unsigned long long* product;   // [K * K] or NULL
};
hipError_t launch_topic_cooc(const TopicCoocArgs& a, int blocks, int lds, hipStream_t st);
// lda_group_topics: k_group_topics, one wave per document with a
// group id >= 0 and at least min_tokens tokens, builds the document's topic
// counts and the list of its distinct topics as k_topic_cooc does and adds, to
// row g of the tables, n_dk (tokens), 1 when the topic is present (present) and
// floor(n_dk 2^32 / L_d) (shares); 1 and L_d to group_docs[g], group_tokens[g].
// buf = group_docs [G], group_tokens [G], tokens [G K], then present [G K] and
// shares [G K] when requested; o_present / o_shares are their first cells (-1:
// not requested) and cells the length of buf, which must be zero before the
// launch.  With lds != 0 a block keeps a copy of buf in 64-bit LDS cells behind
// the four waves' histograms and lists (group_topics_wave_bytes) and adds its
// nonzero cells once; the whole must fit GROUP_TOPICS_LDS_BYTES, the default
// dynamic LDS limit.  Otherwise every add is a global 64-bit integer atomic.
constexpr size_t GROUP_TOPICS_LDS_BYTES = 65536;
inline size_t group_topics_wave_bytes(int32_t Kp) { return 4 * (size_t)Kp * (sizeof(uint32_t) + sizeof(uint16_t)); }
struct GroupTopicsArgs {
  const int32_t* z;
  const int64_t* doc_off;
  const int32_t* doc_group;      // [D], -1 = left out
  int64_t D, min_tokens;
  double min_prop;
  int32_t min_count, K, Kp, G;
  int64_t o_present, o_shares, cells;
  unsigned long long* buf;       // [cells]
};
hipError_t launch_group_topics(const GroupTopicsArgs& a, int blocks, int lds, hipStream_t st);
// lda_subcorpus_* (DESIGN.md 9m): k_subcorpus_count adds 1 to sub[word, topic]
// (V x Kp int32) for every token of the documents whose mask byte is nonzero,
// one wave per document; k_subcorpus_add is dst += src over cells;
// k_subcorpus_totals adds the column sums of sub to totals [K] (zero before).
hipError_t launch_subcorpus_count(const int32_t* z, const int32_t* words, const int64_t* doc_off,
                                  const uint8_t* mask, int64_t D, int32_t Kp, int32_t* sub, int blocks,
                                  hipStream_t st);
hipError_t launch_subcorpus_add(int32_t* dst, const int32_t* src, int64_t cells, hipStream_t st);
hipError_t launch_subcorpus_totals(const int32_t* sub, int32_t V, int32_t K, int32_t Kp, long long* totals,
                                   hipStream_t st);

}  // namespace lda
