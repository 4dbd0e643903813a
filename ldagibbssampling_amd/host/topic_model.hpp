// topic_model.hpp — native host mirror of Mallet 2.0.7's ParallelTopicModel
// (cc.mallet.topics, not vendored; pom.xml:107-111) over the sampler C ABI.
//
// What the reference calls (src/cmu_ron/TrainAndPredict.java:159-177,
// src/cmu/TrainAndPredict.java:258-274) keeps its name and meaning here; the
// per-token sampling inside estimate() is the GPU (lda_sample / lda_apply on
// one context per GPU shard, RCCL all-reduce of the int32 delta between them).
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/lda_mi355x.h"

namespace lda_host {

struct Error {
  lda_status status;
  std::string message;
};

class ShardGroup;  // GPU shards + their all-reduce (topic_model.cpp)

// GPU shards for setNumThreads(num_threads) over this corpus (ldatm_plan_shards)
int32_t plan_shards(int32_t num_threads, int32_t num_devices, int64_t num_tokens, int32_t num_types,
                    int32_t num_topics, int64_t num_docs);

// The eleven per-topic diagnostics from the integer statistics (host only,
// no device; ldatm_diagnostics_finish of lda_topic_model.h states the columns)
void diagnosticsFinish(int32_t K, int32_t V, int32_t n, double beta, const int32_t* nwsum, int32_t max_len,
                       const int64_t* topic_doc_counts, const int32_t* word_ids, const int32_t* counts,
                       const int64_t* totals, const double* share_sums, const uint64_t* sumsq, const int64_t* codoc,
                       const int64_t* doc_stats, double* out);

// Reference-corpus coherence from co-occurrence counts (host only, no device;
// ldatm_coherence_finish of lda_topic_model.h states the three expressions):
// sums [K] over the kept pairs and their number pairs [K]
void coherenceFinish(int32_t K, int32_t n, int32_t measure, double epsilon, const int64_t* cooc, int64_t units,
                     double* sums, int64_t* pairs);

// lda_topic_top_docs' weight, ((double) count + smoothing) / ((double) length
// + (double) K * smoothing), and printTopicDocuments' text from K x n lists
// (host only, no device; ldatm_topic_documents_format of lda_topic_model.h)
double topicDocWeight(int32_t K, double smoothing, int32_t count, int32_t length);
std::string topicDocumentsFormat(int32_t K, int32_t n, double smoothing, const int64_t* doc_ids, const int32_t* counts,
                                 const int32_t* lengths, const std::function<std::string(int64_t)>& name);
// printDocumentNeighbors' text from M x n arrays: "#doc neighbor name value",
// then "<doc> <neighbor> <name of the neighbor> <value>" per query document
// docs[j] (null: j) and rank, Java Double.toString values; a query's list
// ends at its first id < 0 (host only; ldatm_document_neighbors_format)
std::string documentNeighborsFormat(int64_t M, int32_t n, const int64_t* docs, const int64_t* doc_ids,
                                    const double* values, const std::function<std::string(int64_t)>& name);

// ldatm_relevant_words_format's relevance, logprob - (1 - lambda) (logprob -
// loglift), and its text from K x n lists (host only, no device)
double relevanceOf(double lambda, double logprob, double loglift);
std::string relevantWordsFormat(int32_t K, int32_t n, double lambda, const int32_t* word_ids, const int32_t* counts,
                                const int64_t* totals, const double* logprob, const double* loglift,
                                const std::function<std::string(int32_t)>& name);

// lda_topic_phrases over several shards: B_k, the sum over
// the shards of the count of the shard's last (LDA_PHRASES_MAX-th) listed
// phrase of topic k (0 where the list is not full), bounds the total of every
// phrase outside the united lists; proven[k] is the number of leading entries
// of totals[k*n ..] strictly above B_k, n where B_k = 0.
// shard_counts [G][K][LDA_PHRASES_MAX].  And printTopicPhrases' text from
// K x n lists (host only; ldatm_topic_phrases_format of lda_topic_model.h).
void topicPhrasesBound(int32_t K, int32_t n, int32_t G, const int64_t* shard_counts, const int64_t* totals,
                       int64_t* bound, int32_t* proven);
std::string topicPhrasesFormat(int32_t K, int32_t n, int32_t max_len, const int32_t* phrase_words,
                               const int32_t* lengths, const int64_t* counts,
                               const std::function<std::string(int32_t)>& name);

// Topic co-occurrence, host only: the table a measure needs
// (LDATM_COOC_*, -1 for an unknown measure), the K x K matrix of a measure
// from lda_topic_cooccurrence's integers, each topic's n strongest other
// topics from a matrix (value descending, then smaller id, non-finite values
// left out, -1 / NaN past the last), and the partners' text.
int32_t correlationTable(int32_t measure);
void topicCorrelationFinish(int32_t measure, int32_t K, int64_t docs_used, const int64_t* tokens,
                            const int64_t* present, int32_t table_kind, const int64_t* table, double* out);
void topicPartnersSelect(int32_t K, int32_t n, const double* matrix, int32_t* ids, double* values);
std::string topicCorrelationsFormat(int32_t K, int32_t n, const int32_t* ids, const double* values);

// Topics by document group, host only: the G x K matrix of a
// kind (LDATM_GROUP_*) from lda_group_topics' integers, each group's n largest
// finite values of a G x K matrix (value descending, then smaller topic id,
// -1 / NaN past the last), and that selection's text.
void groupPrevalenceFinish(int32_t kind, int32_t G, int32_t K, const int64_t* group_docs, const int64_t* group_tokens,
                           const int64_t* tokens, const int64_t* present, const uint64_t* shares, double* out);
void groupTopTopicsSelect(int32_t G, int32_t K, int32_t n, const double* matrix, int32_t* ids, double* values);
std::string groupTopicsFormat(int32_t G, int32_t n, const int32_t* ids, const double* values);

class ParallelTopicModel {
 public:
  ParallelTopicModel(int32_t num_topics, double alpha_sum, double beta);
  ~ParallelTopicModel();
  ParallelTopicModel(const ParallelTopicModel&) = delete;
  ParallelTopicModel& operator=(const ParallelTopicModel&) = delete;

  // ---- data (addInstances) -------------------------------------------
  void setAlphabet(std::vector<std::string> words, int32_t num_types);
  void addInstances(int64_t D, const int64_t* doc_off, const int32_t* words,
                    const char* const* sources);

  // ---- options -------------------------------------------------------
  void setNumIterations(int32_t n) { num_iterations_ = n; }
  void setOptimizeInterval(int32_t n) { optimize_interval_ = n; }
  void setBurninPeriod(int32_t n) { burnin_period_ = n; }
  void setSaveSampleInterval(int32_t n) { save_sample_interval_ = n; }
  void setSymmetricAlpha(bool on) { symmetric_alpha_ = on; }
  void setTopicDisplay(int32_t interval, int32_t n) {
    show_topics_interval_ = interval;
    words_per_topic_ = n;
  }
  void setRandomSeed(int64_t seed);
  void setNumThreads(int32_t n);
  void setSampler(int32_t sampler);
  // split sweeps across GPU shards: each shard's sweep in `parts` parts, part
  // i's all-reduce overlapping part i+1's sampling (1 = one exchange per sweep)
  void setExchangeParts(int32_t parts);
  // explicit shard placement: shard g on devices[g] (n shards; n = 0 returns
  // to setNumThreads' plan).  Shards that share one device exchange through a
  // device-side sum instead of RCCL (the multi-shard path on one GPU).
  void setDevices(const int32_t* devices, int32_t n);
  // warm start (lda_set_warm_start): sweeps 0..sweeps-1 in `parts` sequential
  // parts; the default 4 x 50 (held-out perplexity at K = 20)
  void setWarmStart(int32_t parts, int32_t sweeps);
  // sweeps past the warm start emulate the staleness of Mallet's T worker
  // threads (lda_staleness_schedule): T = 0 -> numThreads (the default),
  // T < 0 -> plain snapshot sweeps
  void setStalenessThreads(int32_t threads);
  int32_t numShards();
  // the shards' compact exchange: cells per packed word (0: not compact),
  // escape lists at their used length (1) or whole, the largest per-shard
  // escape count gathered and the count reads so far (ldatm_exchange_info)
  void exchangeInfo(int32_t* cells, int32_t* used_lists, int32_t* escapes_max, int64_t* list_exchanges);
  void setVerbosity(int32_t v) { verbosity_ = v; }
  // state a Java-side ParallelTopicModel already holds (GpuParallelTopicModel:
  // Mallet's own addInstances topics, alpha/beta optimised in an earlier
  // estimate(), the Philox sweep counter of the previous estimate())
  void setTopics(const int32_t* z, int64_t n);
  void setHyper(const double* alpha, double alpha_sum, double beta);
  uint32_t sweep();
  void setSweep(uint32_t s);
  void setPrintLogLikelihood(bool on) { print_log_likelihood_ = on; }

  // ---- training ------------------------------------------------------
  void estimate();
  const std::vector<std::pair<int32_t, double>>& llTrace() const { return ll_trace_; }
  double modelLogLikelihood();

  // ---- state ---------------------------------------------------------
  int32_t numTopics() const { return K_; }
  int32_t numTypes() const { return V_; }
  int64_t numDocs() const { return (int64_t)doc_off_.size() - 1; }
  int64_t numTokens() const { return doc_off_.back(); }
  const std::vector<double>& alpha() const { return alpha_; }
  double alphaSum() const { return alpha_sum_; }
  double beta() const { return beta_; }
  std::vector<int32_t> topics();                      // z of every token
  void counts(int32_t* nw, int32_t* nwsum);           // nw[V*K] (nullable), nwsum[K]
  std::vector<double> getTopicProbabilities(int64_t doc);

  // ---- readouts selected on the device -----------------
  // lda_top_words on shard 0 (every shard holds the same global counts):
  // word_ids / counts [K*n], count descending, ties by ascending word id,
  // -1 / 0 past a topic's last nonzero word
  void topWords(int32_t n, int32_t* word_ids, int32_t* counts);
  // the global document ids docs[M] (null: every document, M = numDocs())
  // mapped onto the shards as scoreTheta maps them; each shard answers for
  // its own documents (lda_doc_top_topics / lda_doc_counts) and the rows are
  // scattered back into the caller's order.  topics / counts [M*mtop]; nd [M*K]
  void docTopTopics(int32_t mtop, int64_t M, const int64_t* docs, int32_t* topics, int32_t* counts);
  void docCounts(int64_t M, const int64_t* docs, int32_t* nd);
  // lda_topic_top_docs on every shard, the local ids made
  // global, and the shards' lists merged per topic by (weight descending, id
  // ascending) with the weight recomputed from (count, length): doc_ids /
  // counts / lengths [K*n], -1 / 0 / 0 past a topic's last candidate.  The
  // arguments are checked before any shard is built.
  void topicTopDocs(int32_t n, double smoothing, int32_t min_tokens, int64_t* doc_ids, int32_t* counts,
                    int32_t* lengths);

  // lda_relevant_words / lda_salient_words / lda_word_rows on shard 0
  // (every shard holds the same global counts).  The arguments
  // are checked before any shard is built.  Planes [L*K*n]; lists [n]; rows
  // [M*K] and totals [M]
  void relevantWords(int32_t n, int32_t L, const double* lambdas, int32_t* word_ids, int32_t* counts,
                     int64_t* totals, double* logprob, double* loglift);
  void salientWords(int32_t n, int32_t* word_ids, int64_t* totals, double* saliency, double* distinctiveness);
  void wordRows(int64_t M, const int32_t* word_ids, int32_t* rows, int64_t* totals);
  // relevantWords(n, one lambda) as text: "topic rank word count total
  // relevance logprob loglift" per topic and rank
  std::string relevantWordsText(int32_t n, double lambda);

  // lda_topic_phrases.  One shard: passed through, proven[k]
  // = n.  Several: every shard's best LDA_PHRASES_MAX per topic united by
  // content, the exact totals and smallest global starts of the candidates
  // from lda_phrase_lookup on every shard, ordered as lda_topic_phrases
  // orders them; topic_runs and skipped_long are sums, topic_distinct is -1
  // (a phrase may live in several shards), proven as topicPhrasesBound.
  void topicPhrases(int32_t n, int32_t min_len, int32_t max_len, int32_t min_count, int32_t* phrase_words,
                    int32_t* lengths, int64_t* counts, int64_t* first, int64_t* topic_runs, int64_t* topic_distinct,
                    int64_t* skipped_long, int32_t* proven);
  // topicPhrases as text: "#topic rank count phrase", then "topic rank count w1 w2 ..."
  std::string topicPhrasesText(int32_t n, int32_t min_len, int32_t max_len, int32_t min_count);

  // lda_topic_cooccurrence on every shard, summed (integers: exact); the
  // matrix of one measure, counting only the table it needs; each topic's n
  // strongest partners by it; the partners as text.  The arguments are
  // checked before any shard is built.
  void topicCooccurrence(int64_t min_tokens, int32_t min_count, double min_prop, int64_t* docs_used,
                         int64_t* tokens, int64_t* present, int64_t* codocs, int64_t* overlap, int64_t* product);
  void topicCorrelations(int32_t measure, int64_t min_tokens, int32_t min_count, double min_prop, double* out);
  void topicPartners(int32_t measure, int64_t min_tokens, int32_t min_count, double min_prop, int32_t n,
                     int32_t* ids, double* values);
  std::string topicCorrelationsText(int32_t measure, int32_t n, int64_t min_tokens, int32_t min_count,
                                    double min_prop);

  // lda_group_topics on every shard with its slice of doc_group (global
  // document ids), summed (integers: exact); the matrix of one kind, counting
  // only the table it needs; each group's n largest topics by it as text; each
  // topic's top words inside the masked documents (every shard counts its
  // slice, the tables are added into shard 0's, which selects; the tables are
  // released).  The arguments are checked before any shard is built.
  void groupTopics(const int32_t* doc_group, int32_t G, int64_t min_tokens, int32_t min_count, double min_prop,
                   int64_t* group_docs, int64_t* group_tokens, int64_t* tokens, int64_t* present, uint64_t* shares);
  void groupPrevalence(const int32_t* doc_group, int32_t G, int32_t kind, int64_t min_tokens, int32_t min_count,
                       double min_prop, double* out);
  std::string groupTopicsText(const int32_t* doc_group, int32_t G, int32_t kind, int32_t n, int64_t min_tokens,
                              int32_t min_count, double min_prop);
  void subCorpusTopWords(const uint8_t* doc_mask, int32_t n, int32_t* word_ids, int32_t* counts, int64_t* totals);

  // ---- topic diagnostics --------------------------------
  // lda_topic_codocuments on every shard with the caller's lists, summed in
  // int64: codoc [K n(n+1)/2], doc_stats [K (2+P)]
  void topicCodocuments(int32_t n, const int32_t* word_ids, int32_t P, const double* props, int64_t* codoc,
                        int64_t* doc_stats);
  // topWords(n) and lda_topic_word_stats on shard 0, then topicCodocuments
  // with Mallet's seven proportions (doc_stats [K 9])
  void topicStatistics(int32_t n, int32_t* word_ids, int32_t* counts, int64_t* totals, double* share_sums,
                       uint64_t* sumsq, int64_t* codoc, int64_t* doc_stats);
  // topicStatistics, the shards' topicDocCounts of the current z and
  // diagnosticsFinish: out [K LDATM_DIAG_COLUMNS]; word_ids [K n] or null
  void topicDiagnostics(int32_t n, double* out, int32_t* word_ids);

  // ---- reference-corpus coherence ------------------------
  // lda_word_cooccurrences with the caller's lists: on the training corpus
  // (doc_off null) every shard counts its own documents and the results add;
  // a host corpus goes to shard 0 alone.  cooc [K n(n+1)/2], *units
  void wordCooccurrences(int32_t n, const int32_t* word_ids, int32_t window, int64_t Dh, const int64_t* doc_off,
                         const int32_t* words, int64_t* cooc, int64_t* units);
  // topWords(n), wordCooccurrences and coherenceFinish: values [K] (the mean
  // over the kept pairs, 0 without one) and pairs [K]; word_ids_out [K n] and
  // cooc_out [K n(n+1)/2] may be null; epsilon < 0: the measure's default
  void topicCoherence(int32_t measure, int32_t n, int32_t window, double epsilon, int64_t Dh, const int64_t* doc_off,
                      const int32_t* words, double* values, int64_t* pairs, int32_t* word_ids_out, int64_t* cooc_out,
                      int64_t* units);

  // ---- topic distances and nearest topics ----------------
  // lda_topic_distances / lda_topic_nearest on shard 0 of this model against
  // shard 0 of `other` (null: this model); every shard holds the same global
  // counts.  out [K * K2]; topics / values [K * n].  The arguments are checked
  // before any shard is built.
  void topicDistances(ParallelTopicModel* other, int32_t metric, double* out);
  void nearestTopics(ParallelTopicModel* other, int32_t metric, int32_t n, int32_t* topics, double* values);

  // ---- nearest documents ---------------------------------
  // lda_doc_distances routed to the shards as scoreTheta routes: queries
  // theta[Q*K] or counts[Q*K] (exactly one) against the global document ids
  // docs[M] (null: every document, M = numDocs()); out [Q*M]
  void documentDistances(int32_t metric, int64_t Q, const double* theta, const int32_t* counts, int64_t M,
                         const int64_t* docs, double* out);
  // lda_doc_nearest on every shard among its own documents (skip: global ids,
  // -1 or null = none), the local ids made global and the shards' Q x n lists
  // merged by (value, global id).  A shard's list holds each of its documents
  // that belongs to the global best n, so the result does not depend on the
  // number of shards, bit for bit.  doc_ids / values [Q*n], -1 / NaN past the
  // last candidate
  void nearestDocuments(int32_t metric, int32_t n, int64_t Q, const double* theta, const int32_t* counts,
                        const int64_t* skip, int32_t min_tokens, int64_t* doc_ids, double* values);
  // the queries are the model's own documents docs[M] (null: all).  One
  // shard: lda_doc_neighbors passed through.  Several: per chunk of queries
  // docCounts from the owning shards, then nearestDocuments(counts, skip = own
  // id); the same bits by lda_doc_neighbors' contract
  void documentNeighbors(int32_t metric, int32_t n, int64_t M, const int64_t* docs, int32_t min_tokens,
                         int64_t* doc_ids, double* values);
  // documentNeighbors of every document as text (documentNeighborsFormat)
  std::string documentNeighborsText(int32_t n, int32_t metric, int32_t min_tokens);

  // ---- outputs -------------------------------------------------------
  std::string documentTopics(double threshold, int32_t max);
  std::string displayTopWords(int32_t num_words, bool using_new_lines);
  // topicTopDocs(max) as text: "topic doc name weight" per topic and rank
  std::string topicDocuments(int32_t max, double smoothing, int32_t min_tokens);

  // ---- checkpoint / resume (the reference's save()/load(),
  //      src/cmu_ron/TrainAndPredict.java:179-200, as a native format) ----
  void save(const std::string& path);
  static std::unique_ptr<ParallelTopicModel> load(const std::string& path);

  // ---- inference (TopicInferencer.getSampledDistribution, batched) ---
  void infer(int64_t Dh, const int64_t* doc_off, const int32_t* words, int32_t num_iterations,
             int32_t thinning, int32_t burn_in, uint64_t seed, double* theta);

  // ---- prediction scoring (the reference's Predictor.predict /
  //      scoresForChangelistOnTests, batched on the device: lda_score_docs) ----
  // theta[Q*K] against the global document ids docs[M] (null: every document,
  // M = numDocs()); scores[Q*M].  Each shard scores its own documents.
  void scoreTheta(int32_t metric, int64_t Q, const double* theta, int64_t M, const int64_t* docs,
                  double* scores);
  // the n best documents per query, best first (cosine: largest; mse:
  // smallest), ties by ascending id; doc_ids / scores [Q*n], entries past
  // numDocs() are -1 / NaN
  void scoreTop(int32_t metric, int64_t Q, const double* theta, int32_t n, int64_t* doc_ids, double* scores);

  // ---- held-out evaluation by document completion (lda_heldout_loglik /
  //      lda_doc_completion on shard 0: every shard holds the same global
  //      counts, and the inference draws are keyed by a token's index in the
  //      batch, so spreading the documents over shards would change theta) ----
  // theta[Dh*K] and the scored tokens given; returns the total
  double heldOutLogLik(int64_t Dh, const double* theta, const int64_t* doc_off, const int32_t* words,
                       double* doc_ll);
  // whole held-out documents: tokens outside [0, V) are dropped, then each
  // document is split as completionSplit does; returns the total
  double evaluate(int64_t Dh, const int64_t* doc_off, const int32_t* words, int32_t num_iterations,
                  int32_t thinning, int32_t burn_in, uint64_t seed, double* doc_ll, int64_t* tokens_scored,
                  double* theta_out);
  // the first floor(L/2) kept tokens of each document are observed, the rest
  // scored (corpus.document_completion_split after the out-of-vocabulary drop)
  static void completionSplit(int32_t V, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                              std::vector<int64_t>& obs_off, std::vector<int32_t>& obs,
                              std::vector<int64_t>& sc_off, std::vector<int32_t>& sc);
  // Mallet's MarginalProbEstimator.evaluateLeftToRight (lda_left_to_right on
  // shard 0, for the same reason): tokens outside [0, V) are dropped and not
  // counted; doc_ll[Dh]; tokens_scored may be null; returns the total
  double leftToRight(int64_t Dh, const int64_t* doc_off, const int32_t* words, int32_t num_particles,
                     int32_t resampling, uint64_t seed, double* doc_ll, int64_t* tokens_scored);
  // a held-out set evaluated by estimate() after every interval-th sweep
  // (interval 0: off); not part of the checkpoint
  void setHeldOut(int64_t Dh, const int64_t* doc_off, const int32_t* words, int32_t interval,
                  int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed);
  const std::vector<std::pair<int32_t, double>>& heldOutTrace() const { return held_trace_; }

 private:
  void ensureShards();
  void markDirty();
  void optimizeAlpha();
  // count histogram (max_word_total_ + 1 cells) and nwsum, fetched with the
  // alpha statistics in one lda_hyper_statistics call
  void optimizeBeta(const std::vector<int32_t>& count_hist, const std::vector<int32_t>& nwsum);
  void log(const std::string& line) const;
  // docTopTopics (mtop >= 1) / docCounts (mtop == 0, width K) over the shards
  void docReadout(int32_t mtop, int64_t M, const int64_t* docs, int32_t* out0, int32_t* out1);

  int32_t K_;
  double alpha_sum_, beta_;
  std::vector<double> alpha_;
  int32_t V_ = 0;
  std::vector<std::string> alphabet_;
  std::vector<int64_t> doc_off_{0};
  std::vector<int32_t> words_;
  std::vector<std::string> sources_;
  std::vector<uint8_t> has_source_;
  std::vector<int32_t> z_cache_;  // z of the shards, valid when !z_dirty_
  bool z_dirty_ = true;

  int32_t num_iterations_ = 1000, optimize_interval_ = 0, burnin_period_ = 200;
  int32_t save_sample_interval_ = 10, show_topics_interval_ = 50, words_per_topic_ = 7;
  bool symmetric_alpha_ = false, print_log_likelihood_ = true;
  uint64_t seed_ = 0;
  int32_t num_threads_ = 1, sampler_ = LDA_SAMPLER_DENSE, verbosity_ = 0, exchange_parts_ = 1;
  // shards on distinct GPUs exchange packed words (lda_exchange_pack);
  // LDA_EXCHANGE_INT32=1 in the environment sends the int32 buffers (A/B)
  bool compact_exchange_ = true;
  int32_t warm_parts_ = 4, warm_sweeps_ = 50;
  int32_t staleness_threads_ = 0;
  void applySweepSchedule();

  std::vector<int32_t> devices_;  // setDevices (empty: plan_shards)
  std::unique_ptr<ShardGroup> shards_;
  bool shards_dirty_ = true;
  int32_t max_doc_len_ = -1;
  int64_t max_word_total_ = 0;  // largest word frequency (countHistogram bound), set with the shards
  uint32_t sweep_ = 0;  // Philox sweep counter carried across re-sharding
  std::vector<int32_t> doc_len_counts_, topic_doc_counts_;  // alpha statistics
  std::vector<std::pair<int32_t, double>> ll_trace_;
  // setHeldOut: the documents and the inference settings, and estimate()'s trace
  std::vector<int64_t> held_off_{0};
  std::vector<int32_t> held_words_;
  int32_t held_interval_ = 0, held_iterations_ = 100, held_thinning_ = 10, held_burn_in_ = 10;
  uint64_t held_seed_ = 0;
  std::vector<std::pair<int32_t, double>> held_trace_;
};

}  // namespace lda_host
