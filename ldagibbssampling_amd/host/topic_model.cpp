// topic_model.cpp — ParallelTopicModel host mirror (see topic_model.hpp) and
// the C ABI of include/lda_topic_model.h.
//
// Mallet 2.0.7 behaviour restated here (cc.mallet.topics.ParallelTopicModel,
// not vendored; call sites src/cmu_ron/TrainAndPredict.java:159-177):
//  * addInstances: new documents get random topics, earlier ones keep theirs;
//    counts are rebuilt from every document.
//  * estimate(): for iteration = 1..numIterations: topic display every
//    showTopicsInterval; one parallel sweep (AD-LDA: every shard samples
//    against the same nw snapshot, then the deltas are summed); alpha
//    statistics on sweeps with iteration > burninPeriod and
//    iteration % saveSampleInterval == 0; optimizeAlpha + optimizeBeta when
//    iteration > burninPeriod and iteration % optimizeInterval == 0;
//    "<iteration> LL/token: x" every 10 iterations.  Not Mallet's: with
//    setHeldOut, "<iteration> held-out LL/token: x" every interval-th
//    iteration (document completion on the device; training is unchanged).
//  * optimizeAlpha: Dirichlet.learnParameters(alpha, topicDocCounts,
//    docLengthCounts, 1.001, 1.0, 1), or learnSymmetricConcentration over the
//    pooled histogram when usingSymmetricAlpha; histograms then cleared.
//  * optimizeBeta: learnSymmetricConcentration(countHistogram,
//    topicSizeHistogram, numTypes, betaSum); beta = betaSum / numTypes.
#include "topic_model.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <numeric>
#include <sstream>

#include "../../include/lda_topic_model.h"
#include "java_format.hpp"

namespace lda_host {

namespace {

[[noreturn]] void raise(lda_status s, const std::string& msg) { throw Error{s, msg}; }

void check(lda_status s, const char* where) {
  if (s != LDA_OK) {
    const char* m = lda_last_error();
    raise(s, std::string(where) + ": " + (m ? m : ""));
  }
}

// dst[i] += src[i]: the in-process sum of shard buffers that share one device
// (ShardGroup's local exchange; RCCL refuses two ranks on one GPU)
__global__ void k_sum_into(int4* __restrict__ dst, const int4* __restrict__ src, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int4 b = src[i];
    if (b.x | b.y | b.z | b.w) {
      int4 a = dst[i];
      a.x += b.x;
      a.y += b.y;
      a.z += b.z;
      a.w += b.w;
      dst[i] = a;
    }
  }
}

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) raise(e == hipErrorOutOfMemory ? LDA_ERR_OUT_OF_MEMORY : LDA_ERR_DEVICE,
                             std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

// How many GPU shards setNumThreads(n) becomes (ldatm_plan_shards): at most
// n, the visible devices and the documents, and one when splitting the
// sweep saves less than the exchange costs.  Per sweep, the sampler moves
// ~(2 Kp + 16) bytes per token (the 16-bit row + stream; the sparse kernels
// read fewer bytes at a lower rate) at ~5 TB/s, the exchange is a ring
// all-reduce of 4 (V Kp + Kp) bytes at ~100 GB/s per link plus ~100 us of
// latency; G shards save (1 - 1/G) of the sweep.  The reference's own corpus
// (C1: ~16k tokens, K = 500, V ~ 5000) with setNumThreads(4) gets one GPU: its
// ~40 us sweep is far below a 10 MB all-reduce.
int32_t plan_shards(int32_t num_threads, int32_t num_devices, int64_t num_tokens, int32_t num_types,
                    int32_t num_topics, int64_t num_docs) {
  const int64_t g = std::max<int64_t>(1, std::min<int64_t>({(int64_t)num_threads, (int64_t)num_devices,
                                                            std::max<int64_t>(num_docs, 1)}));
  if (g < 2) return 1;
  const double kp = (double)lda_padded_topics(num_topics);
  const double sweep_s = (double)num_tokens * (2.0 * kp + 16.0) / 5e12;
  const double exch_s = 2.0 * 4.0 * ((double)num_types * kp + kp) / 1e11 + 1e-4;
  for (int64_t k = g; k >= 2; --k)
    if (sweep_s * (1.0 - 1.0 / (double)k) > exch_s) return (int32_t)k;
  return 1;
}

// ----------------------------------------------------------------- shards
// One lda_ctx per GPU over a contiguous, token-balanced document range; the
// delta buffers are summed in place with one RCCL all-reduce per sweep
// (ncclCommInitAll over the shards' devices, grouped calls from this thread).
//
// Split sweeps (setExchangeParts, lda_set_exchange_parts): every shard samples
// its documents in P parts with one delta buffer each; part i's all-reduce is
// issued on a per-shard collective stream that waits only for part i, so it
// runs while part i+1 samples, and the shards' streams wait for the last sum
// before the apply.  Same sweep bit for bit (integer sums, fixed snapshot).
//
// Shards on distinct devices exchange through RCCL.  Shards that share one
// device (ParallelTopicModel::setDevices, e.g. {0, 0, 0}: the multi-shard
// path exercised on a one-GPU box) exchange through a device-side sum
// instead -- shard 0's stream adds every other buffer into its own and copies
// the sum back -- with the same events, streams and apply ordering.
class ShardGroup {
 public:
  std::vector<lda_ctx*> ctx;
  std::vector<int> dev;            // shard g runs on device dev[g]
  std::vector<int64_t> doc_begin;  // shard g owns documents [doc_begin[g], doc_begin[g+1])
  bool local_sum = false;          // every shard on one device: no RCCL
  std::vector<ncclComm_t> comms;
  std::vector<hipStream_t> comm_streams;  // per shard, split sweeps only
  std::vector<hipEvent_t> events;
  std::vector<hipEvent_t> sum_events;     // local_sum: per shard "sampled" / shard 0 "summed"
  int parts = 1;
  // RCCL exchange in the compact form (lda_exchange_pack): the largest
  // shard's tokens (sizes the escape lists), the packed words and escape
  // list of every shard per part, and per shard and part the gathered lists
  // of all shards [G x escape_count]
  int64_t max_tokens = 0;
  bool compact = true;
  // shards on one device exchange the compact form through device-side
  // stand-ins for the collectives (sum of the packed words, copies of the
  // escape lists): the pack / unpack ordering of the multi-GPU path, run on a
  // one-GPU box (LDA_LOCAL_COMPACT=1; tests/test_topic_model_gpu.py)
  bool local_compact = false;
  size_t packed_count = 0, escape_count = 0;
  std::vector<std::vector<void*>> packed, escapes;        // [part][shard]
  std::vector<std::vector<int32_t*>> escapes_all;         // [part][shard], device buffers
  // escape lists at their used length (round 6, the torch path's default
  // since round 5): every shard's count is copied to pinned host memory right
  // behind its pack, the packed words' all-reduce is issued, and only then
  // does the host read the counts (the copies, not the sum: the read overlaps
  // that collective) and all-gather 1 + 3 m int32 per shard, m the largest
  // count; nothing when m = 0.  false: the whole fixed-capacity lists, no
  // read (LDA_ESCAPE_LISTS=capacity).
  bool used_lists = true;
  int32_t cells = 2;                                      // lda_set_exchange_cells
  int32_t* host_counts = nullptr;                         // pinned [LDA_MAX_EXCHANGE_PARTS][G]
  std::vector<std::vector<hipEvent_t>> count_events;      // [part][shard]: count copied
  std::vector<size_t> gathered_cap;                       // [part]: escapes_all holds G x this
  std::vector<int32_t> part_m;                            // [part]: the m of the pending exchange
  int32_t m_max = 0;                                      // largest m gathered (ldatm_exchange_info)
  int64_t list_exchanges = 0;                             // count reads so far

  ~ShardGroup() {
    for (auto c : comms) ncclCommDestroy(c);
    for (size_t g = 0; g < comm_streams.size(); ++g) {
      (void)hipSetDevice(dev[g]);
      (void)hipEventDestroy(events[g]);
      (void)hipStreamDestroy(comm_streams[g]);
    }
    for (size_t g = 0; g < sum_events.size(); ++g) {
      (void)hipSetDevice(dev[g]);
      (void)hipEventDestroy(sum_events[g]);
    }
    for (auto& v : escapes_all)
      for (size_t g = 0; g < v.size(); ++g)
        if (v[g]) {
          (void)hipSetDevice(dev[g]);
          (void)hipFree(v[g]);
        }
    for (auto& v : count_events)
      for (size_t g = 0; g < v.size(); ++g) {
        (void)hipSetDevice(dev[g]);
        (void)hipEventDestroy(v[g]);
      }
    if (host_counts) (void)hipHostFree(host_counts);
    for (auto c : ctx) lda_destroy(c);
  }

  void init_exchange() {
    const size_t G = ctx.size();
    if (G < 2) return;
    local_sum = std::all_of(dev.begin(), dev.end(), [&](int d) { return d == dev[0]; });
    if (local_sum) {
      sum_events.resize(G);
      hip_check(hipSetDevice(dev[0]), "hipSetDevice");
      for (size_t g = 0; g < G; ++g)
        hip_check(hipEventCreateWithFlags(&sum_events[g], hipEventDisableTiming), "hipEventCreate");
      return;
    }
    std::vector<int> sorted = dev;
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      raise(LDA_ERR_UNSUPPORTED, "shards share a device with others on different devices: place all on "
                                 "one device or each on its own");
    comms.resize(G);
    const ncclResult_t r = ncclCommInitAll(comms.data(), (int)G, dev.data());
    if (r != ncclSuccess) {
      comms.clear();
      raise(LDA_ERR_DEVICE, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
    }
  }

  // local_sum: buffer 0 += buffer g, then every buffer = buffer 0, on
  // streams[0] once every shard's streams[g] has reached this point; the
  // other streams then wait for the sum
  void local_reduce(const std::vector<void*>& ptr, size_t count, const std::vector<hipStream_t>& streams) {
    const size_t G = ctx.size();
    hip_check(hipSetDevice(dev[0]), "hipSetDevice");
    for (size_t g = 1; g < G; ++g) {
      hip_check(hipEventRecord(sum_events[g], streams[g]), "hipEventRecord");
      hip_check(hipStreamWaitEvent(streams[0], sum_events[g], 0), "hipStreamWaitEvent");
    }
    const int64_t n4 = (int64_t)count / 4;   // V*Kp + Kp: a multiple of 4 (Kp % 64 == 0)
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n4 + 255) / 256, 4096));
    for (size_t g = 1; g < G; ++g) {
      hipLaunchKernelGGL(k_sum_into, dim3(blocks), dim3(256), 0, streams[0], static_cast<int4*>(ptr[0]),
                         static_cast<const int4*>(ptr[g]), n4);
      hip_check(hipGetLastError(), "k_sum_into");
    }
    for (size_t g = 1; g < G; ++g)
      hip_check(hipMemcpyAsync(ptr[g], ptr[0], count * sizeof(int32_t), hipMemcpyDeviceToDevice, streams[0]),
                "hipMemcpyAsync");
    hip_check(hipEventRecord(sum_events[0], streams[0]), "hipEventRecord");
    for (size_t g = 1; g < G; ++g) hip_check(hipStreamWaitEvent(streams[g], sum_events[0], 0), "hipStreamWaitEvent");
  }

  hipStream_t stream(size_t g) {
    void* s = nullptr;
    check(lda_get_stream(ctx[g], &s), "lda_get_stream");
    return static_cast<hipStream_t>(s);
  }

  bool use_compact() const { return compact && (!local_sum || local_compact) && ctx.size() > 1; }

  // local_sum + use_compact(): every shard's first n int32 of its escape
  // list copied into every shard's escapes_all [G x n] in shard order (what
  // ncclAllGather leaves on distinct devices)
  void local_gather(int part, size_t n, const std::vector<hipStream_t>& streams) {
    const size_t G = ctx.size();
    for (size_t g = 0; g < G; ++g)
      for (size_t r = 0; r < G; ++r)
        hip_check(hipMemcpyAsync(escapes_all[(size_t)part][g] + r * n, escapes[(size_t)part][r],
                                 sizeof(int32_t) * n, hipMemcpyDeviceToDevice, streams[g]),
                  "hipMemcpyAsync");
  }

  // the compact exchange's cells per packed word and list mode, once the
  // shards exist: four 8-bit cells for the large-K sampler's tables (Kp >=
  // 2048, at most 64 shards) when the lists travel at their used length --
  // C5 at 8 GPUs: 1.07 GB instead of 2.15 GB per exchange, ~1e5 escapes per
  // shard per sweep -- else two (C4: the narrower fields
  // escape about as many bytes as they save).  LDA_ESCAPE_LISTS=capacity
  // and LDA_EXCHANGE_CELLS=2|4 override (A/B and tests).
  void init_cells(int32_t kp) {
    const char* el = std::getenv("LDA_ESCAPE_LISTS");
    used_lists = !(el && std::strcmp(el, "capacity") == 0);
    cells = (used_lists && ctx.size() <= 64 && kp >= 2048) ? 4 : 2;
    const char* ec = std::getenv("LDA_EXCHANGE_CELLS");
    if (ec && (ec[0] == '2' || ec[0] == '4') && ec[1] == 0) cells = ec[0] - '0';
    if (cells == 4 && !used_lists)
      raise(LDA_ERR_UNSUPPORTED, "four cells per word need used-length escape lists (their capacity is "
                                 "three times the two-cell lists')");
    for (auto c : ctx) check(lda_set_exchange_cells(c, cells), "lda_set_exchange_cells");
  }

  // the compact exchange's first step, on every shard's own stream: part
  // `part`'s buffer packed (lda_exchange_pack)
  // escapes_all[part][g] able to hold G x n int32 (grown on demand: with
  // four cells a C5 shard's list capacity is 750 MB, and G copies of it per
  // device would be 6 GB for lists that are normally ~1 MB)
  void reserve_gathered(int part, size_t n) {
    const size_t G = ctx.size();
    if (gathered_cap[(size_t)part] >= n) return;
    const size_t want = std::min(escape_count, std::max(n + n / 2, (size_t)4096));
    for (size_t g = 0; g < G; ++g) {
      hip_check(hipSetDevice(dev[g]), "hipSetDevice");
      if (escapes_all[(size_t)part][g]) {
        // an unpack of an earlier exchange may still read the old lists
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipFree(escapes_all[(size_t)part][g]), "hipFree");
      }
      escapes_all[(size_t)part][g] = nullptr;
      hip_check(hipMalloc(reinterpret_cast<void**>(&escapes_all[(size_t)part][g]), sizeof(int32_t) * want * G),
                "hipMalloc");
    }
    gathered_cap[(size_t)part] = want;
  }

  void pack_part(int part) {
    if (!use_compact()) return;
    const size_t G = ctx.size();
    if (packed.size() <= (size_t)part) {
      packed.resize((size_t)part + 1, std::vector<void*>(G));
      escapes.resize((size_t)part + 1, std::vector<void*>(G));
      escapes_all.resize((size_t)part + 1, std::vector<int32_t*>(G, nullptr));
      gathered_cap.resize((size_t)part + 1, 0);
      part_m.resize((size_t)part + 1, 0);
    }
    check(lda_exchange_sizes(ctx[0], (int32_t)G, max_tokens, &packed_count, &escape_count), "lda_exchange_sizes");
    if (used_lists && !host_counts) {
      hip_check(hipHostMalloc(reinterpret_cast<void**>(&host_counts), sizeof(int32_t) * G * LDA_MAX_EXCHANGE_PARTS,
                              hipHostMallocPortable),
                "hipHostMalloc");
      count_events.assign(LDA_MAX_EXCHANGE_PARTS, std::vector<hipEvent_t>(G, nullptr));
      for (auto& v : count_events)
        for (size_t g = 0; g < G; ++g) {
          hip_check(hipSetDevice(dev[g]), "hipSetDevice");
          hip_check(hipEventCreateWithFlags(&v[g], hipEventDisableTiming), "hipEventCreate");
        }
    }
    for (size_t g = 0; g < G; ++g) {
      check(lda_exchange_pack(ctx[g], part, (int32_t)G, max_tokens, &packed[(size_t)part][g],
                              &escapes[(size_t)part][g]),
            "lda_exchange_pack");
      if (used_lists) {
        // the list's count word to pinned memory behind the pack, on the
        // shard's stream: the host reads it in gather_part
        hip_check(hipSetDevice(dev[g]), "hipSetDevice");
        hip_check(hipMemcpyAsync(host_counts + (size_t)part * G + g, escapes[(size_t)part][g], sizeof(int32_t),
                                 hipMemcpyDeviceToHost, stream(g)),
                  "hipMemcpyAsync");
        hip_check(hipEventRecord(count_events[(size_t)part][g], stream(g)), "hipEventRecord");
      }
    }
    if (!used_lists) reserve_gathered(part, escape_count);
  }

  // the escape lists' all-gather, on streams[g] behind the packed words'
  // sum: the whole lists, or (used_lists) the host reads the counts the pack
  // staged and gathers 1 + 3 m int32 per shard
  void gather_part(int part, const std::vector<hipStream_t>& streams) {
    if (!use_compact()) return;
    const size_t G = ctx.size();
    size_t n = escape_count;
    if (used_lists) {
      int32_t m = 0;
      for (size_t g = 0; g < G; ++g) {
        hip_check(hipEventSynchronize(count_events[(size_t)part][g]), "hipEventSynchronize");
        m = std::max(m, host_counts[(size_t)part * G + g]);
      }
      const int32_t cap = (int32_t)((escape_count - 1) / 3);
      if (m < 0 || m > cap)
        raise(LDA_ERR_STATE, "escape list overflow: " + std::to_string(m) + " escapes, capacity " +
                                 std::to_string(cap));
      part_m[(size_t)part] = m;
      m_max = std::max(m_max, m);
      ++list_exchanges;
      if (m == 0) return;
      n = 1 + 3 * (size_t)m;
      reserve_gathered(part, n);
    }
    if (local_sum) {
      local_gather(part, n, streams);
      return;
    }
    ncclResult_t r = ncclGroupStart();
    for (size_t g = 0; g < G && r == ncclSuccess; ++g)
      r = ncclAllGather(escapes[(size_t)part][g], escapes_all[(size_t)part][g], n, ncclInt32, comms[g], streams[g]);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
      raise(LDA_ERR_DEVICE, std::string("ncclAllGather: ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
  }

  // ... and its last, on every shard's own stream: the part's buffer = the sum
  void unpack_part(int part) {
    if (!use_compact()) return;
    const int32_t G = (int32_t)ctx.size();
    for (size_t g = 0; g < ctx.size(); ++g) {
      if (used_lists) {
        const int32_t m = part_m[(size_t)part];
        check(lda_exchange_unpack_lists(ctx[g], part, G, max_tokens, m ? escapes_all[(size_t)part][g] : nullptr, m),
              "lda_exchange_unpack_lists");
      } else {
        check(lda_exchange_unpack(ctx[g], part, G, max_tokens, escapes_all[(size_t)part][g]),
              "lda_exchange_unpack");
      }
    }
  }

  // the sum of part `part`'s buffers across the shards, each shard's on
  // streams[g] (its own stream, or its collective stream): compact, one
  // grouped SUM all-reduce of the packed words (pack_part before,
  // gather_part and unpack_part after); or the int32 buffers themselves
  // (all-reduce / the device-side sum)
  void reduce_part(int part, const std::vector<hipStream_t>& streams) {
    std::vector<void*> ptr(ctx.size());
    size_t count = 0;
    for (size_t g = 0; g < ctx.size(); ++g)
      check(lda_delta_buffer_part(ctx[g], part, &ptr[g], &count), "lda_delta_buffer_part");
    const bool cmp = use_compact();
    if (local_sum) {
      if (cmp)
        local_reduce(packed[(size_t)part], packed_count, streams);   // a multiple of 4 int32
      else
        local_reduce(ptr, count, streams);
      return;
    }
    ncclResult_t r = ncclGroupStart();
    for (size_t g = 0; g < ctx.size() && r == ncclSuccess; ++g) {
      if (cmp) {
        void* pk = packed[(size_t)part][g];
        r = ncclAllReduce(pk, pk, packed_count, ncclInt32, ncclSum, comms[g], streams[g]);
      } else {
        r = ncclAllReduce(ptr[g], ptr[g], count, ncclInt32, ncclSum, comms[g], streams[g]);
      }
    }
    const ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
      raise(LDA_ERR_DEVICE, std::string("ncclAllReduce: ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
  }

  void reduce() {
    if (ctx.size() < 2) return;
    std::vector<hipStream_t> st(ctx.size());
    for (size_t g = 0; g < ctx.size(); ++g) st[g] = stream(g);
    pack_part(0);
    reduce_part(0, st);
    gather_part(0, st);
    unpack_part(0);
  }

  void set_parts(int p) {
    parts = ctx.size() < 2 ? 1 : p;   // nothing to overlap on one GPU
    // reserve_cus < 0: the library's default share of CUs left to the collective
    for (auto c : ctx) check(lda_set_exchange_parts(c, parts, parts > 1 ? -1 : 0), "lda_set_exchange_parts");
    if (parts > 1 && comm_streams.empty()) {
      comm_streams.resize(ctx.size());
      events.resize(ctx.size());
      for (size_t g = 0; g < ctx.size(); ++g) {
        if (hipSetDevice(dev[g]) != hipSuccess ||
            hipStreamCreateWithFlags(&comm_streams[g], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&events[g], hipEventDisableTiming) != hipSuccess)
          raise(LDA_ERR_DEVICE, "collective stream");
      }
    }
  }

  // sample + exchange + apply of one sweep
  void sweep() {
    int32_t np = 1, seq = 0;
    check(lda_sweep_parts(ctx[0], &np, &seq), "lda_sweep_parts");
    if (seq) {
      // a warm-start sweep: every part sampled, summed and applied in turn
      for (int i = 0; i < np; ++i) {
        for (auto c : ctx) check(lda_sample_part(c, i), "lda_sample_part");
        reduce();
        apply();
      }
      return;
    }
    if (ctx.size() < 2 || parts < 2) {
      for (auto c : ctx) check(lda_sample(c), "lda_sample");
      reduce();
      apply();
      return;
    }
    std::vector<hipStream_t> st(ctx.size());
    for (size_t g = 0; g < ctx.size(); ++g) st[g] = stream(g);
    auto hip = [](hipError_t e, const char* what) {
      if (e != hipSuccess) raise(LDA_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    };
    for (int i = 0; i < parts; ++i) {
      for (size_t g = 0; g < ctx.size(); ++g) check(lda_sample_part(ctx[g], i), "lda_sample_part");
      pack_part(i);                       // on the shards' streams, before the event
      for (size_t g = 0; g < ctx.size(); ++g) {
        hip(hipSetDevice(dev[g]), "hipSetDevice");
        hip(hipEventRecord(events[g], st[g]), "hipEventRecord");           // part i sampled
        hip(hipStreamWaitEvent(comm_streams[g], events[g], 0), "hipStreamWaitEvent");
      }
      reduce_part(i, comm_streams);
    }
    // every part's escape lists once every sampler part is enqueued: the
    // count reads wait for the parts' packs, not for the packed sums
    for (int i = 0; i < parts; ++i) gather_part(i, comm_streams);
    for (size_t g = 0; g < ctx.size(); ++g) {
      hip(hipSetDevice(dev[g]), "hipSetDevice");
      hip(hipEventRecord(events[g], comm_streams[g]), "hipEventRecord");   // every sum landed
      hip(hipStreamWaitEvent(st[g], events[g], 0), "hipStreamWaitEvent");
    }
    for (int i = 0; i < parts; ++i) unpack_part(i);
    apply();
  }
  void apply() {
    for (auto c : ctx) check(lda_apply(c), "lda_apply");
  }
  // n sweeps; one shard runs them through lda_sweep, which launches plain
  // sweeps as graphs (the reference's small corpora are launch-bound)
  void sweeps(int32_t n) {
    if (ctx.size() == 1) {
      check(lda_sweep(ctx[0], n), "lda_sweep");
      return;
    }
    for (int32_t i = 0; i < n; ++i) sweep();
  }
};

// ------------------------------------------------------------------ model
ParallelTopicModel::ParallelTopicModel(int32_t num_topics, double alpha_sum, double beta)
    : K_(num_topics), alpha_sum_(alpha_sum), beta_(beta) {
  if (num_topics < 1 || num_topics > LDA_MAX_TOPICS) raise(LDA_ERR_UNSUPPORTED, "num_topics out of range");
  if (!(alpha_sum > 0.0) || !(beta > 0.0)) raise(LDA_ERR_INVALID_ARG, "alphaSum and beta must be > 0");
  alpha_.assign((size_t)K_, alpha_sum / K_);
  // the dense sampler holds K <= 1024; above that the large-K sparse one
  sampler_ = K_ > LDA_MAX_TOPICS_DENSE ? LDA_SAMPLER_SPARSE : LDA_SAMPLER_DENSE;
}

void ParallelTopicModel::setTopics(const int32_t* z, int64_t n) {
  if (n != numTokens()) raise(LDA_ERR_INVALID_ARG, "setTopics needs one topic per token");
  for (int64_t i = 0; i < n; ++i)
    if (z[i] < 0 || z[i] >= K_) raise(LDA_ERR_INVALID_ARG, "topic out of range [0, K)");
  markDirty();
  z_cache_.assign(z, z + n);
}

void ParallelTopicModel::setHyper(const double* alpha, double alpha_sum, double beta) {
  for (int k = 0; k < K_; ++k)
    if (!(alpha[k] > 0.0)) raise(LDA_ERR_INVALID_ARG, "alpha must be > 0");
  if (!(beta > 0.0) || !(alpha_sum > 0.0)) raise(LDA_ERR_INVALID_ARG, "alphaSum and beta must be > 0");
  alpha_.assign(alpha, alpha + K_);
  alpha_sum_ = alpha_sum;
  beta_ = beta;
  if (shards_ && !shards_dirty_)
    for (auto c : shards_->ctx) check(lda_set_alpha_beta(c, alpha_.data(), beta_), "lda_set_alpha_beta");
}

uint32_t ParallelTopicModel::sweep() {
  if (shards_ && !shards_dirty_) check(lda_get_sweep(shards_->ctx[0], &sweep_), "lda_get_sweep");
  return sweep_;
}

void ParallelTopicModel::setSweep(uint32_t s) {
  sweep_ = s;
  if (shards_ && !shards_dirty_)
    for (auto c : shards_->ctx) check(lda_set_sweep(c, sweep_), "lda_set_sweep");
}

ParallelTopicModel::~ParallelTopicModel() = default;

// Anything that invalidates the GPU shards first saves the current topic
// assignments (documents keep their z across re-sharding / addInstances).
void ParallelTopicModel::markDirty() {
  if (shards_ && !shards_dirty_) {
    z_cache_ = topics();
    check(lda_get_sweep(shards_->ctx[0], &sweep_), "lda_get_sweep");
  }
  shards_dirty_ = true;
}

void ParallelTopicModel::setRandomSeed(int64_t seed) {
  markDirty();
  seed_ = (uint64_t)seed;
}

void ParallelTopicModel::setNumThreads(int32_t n) {
  if (n < 1) raise(LDA_ERR_INVALID_ARG, "numThreads must be >= 1");
  markDirty();
  num_threads_ = n;
}

void ParallelTopicModel::setWarmStart(int32_t parts, int32_t sweeps) {
  if (parts < 1 || parts > LDA_MAX_EXCHANGE_PARTS || sweeps < 0)
    raise(LDA_ERR_INVALID_ARG, "warm start: parts in [1, 4], sweeps >= 0");
  warm_parts_ = parts;
  warm_sweeps_ = sweeps;
  if (shards_ && !shards_dirty_) applySweepSchedule();
}

void ParallelTopicModel::setStalenessThreads(int32_t threads) {
  staleness_threads_ = threads;
  if (shards_ && !shards_dirty_) applySweepSchedule();
}

// the shards' sequential sweeps: the warm start, then Mallet's staleness for
// T threads; parts cut in the whole corpus, so the sweeps are
// the same for any shard count
void ParallelTopicModel::applySweepSchedule() {
  const int64_t N = numTokens();
  int32_t parts = 1;
  double fr[LDA_MAX_EXCHANGE_PARTS] = {1.0};
  const int32_t T = staleness_threads_ == 0 ? num_threads_ : staleness_threads_;
  if (T > 0) check(lda_staleness_schedule(T, &parts, fr), "lda_staleness_schedule");
  for (auto c : shards_->ctx) {
    check(lda_set_warm_start(c, warm_parts_, warm_sweeps_, 0, N), "lda_set_warm_start");
    check(lda_set_sequential_sweeps(c, parts, parts > 1 ? fr : nullptr, 0, N), "lda_set_sequential_sweeps");
  }
}

void ParallelTopicModel::setDevices(const int32_t* devices, int32_t n) {
  if (n < 0 || (n > 0 && !devices)) raise(LDA_ERR_INVALID_ARG, "setDevices: bad argument");
  devices_.assign(devices, devices + n);
  markDirty();
}

int32_t ParallelTopicModel::numShards() {
  ensureShards();
  return (int32_t)shards_->ctx.size();
}

void ParallelTopicModel::exchangeInfo(int32_t* cells, int32_t* used_lists, int32_t* escapes_max,
                                      int64_t* list_exchanges) {
  ensureShards();
  const ShardGroup& s = *shards_;
  const bool cmp = s.use_compact();
  if (cells) *cells = cmp ? s.cells : 0;
  if (used_lists) *used_lists = cmp && s.used_lists ? 1 : 0;
  if (escapes_max) *escapes_max = s.m_max;
  if (list_exchanges) *list_exchanges = s.list_exchanges;
}

void ParallelTopicModel::setExchangeParts(int32_t parts) {
  if (parts < 1 || parts > LDA_MAX_EXCHANGE_PARTS) raise(LDA_ERR_INVALID_ARG, "parts out of range");
  exchange_parts_ = parts;
  if (shards_ && !shards_dirty_) shards_->set_parts(parts);
}

void ParallelTopicModel::setSampler(int32_t sampler) {
  if (sampler != LDA_SAMPLER_DENSE && sampler != LDA_SAMPLER_SPARSE)
    raise(LDA_ERR_INVALID_ARG, "unknown sampler");
  markDirty();
  sampler_ = sampler;
}

void ParallelTopicModel::setAlphabet(std::vector<std::string> words, int32_t num_types) {
  if (num_types < V_) raise(LDA_ERR_INVALID_ARG, "the alphabet cannot shrink");
  if (!words.empty() && (int32_t)words.size() != num_types)
    raise(LDA_ERR_INVALID_ARG, "alphabet size mismatch");
  if (num_types != V_) markDirty();
  alphabet_ = std::move(words);
  V_ = num_types;
}

void ParallelTopicModel::addInstances(int64_t D, const int64_t* doc_off, const int32_t* words,
                                      const char* const* sources) {
  if (D < 0 || (D > 0 && !doc_off)) raise(LDA_ERR_INVALID_ARG, "bad documents");
  if (V_ < 1) raise(LDA_ERR_STATE, "set the alphabet before addInstances");
  markDirty();  // documents already in the model keep their z
  const int64_t base = doc_off_.back();
  for (int64_t d = 0; d < D; ++d) {
    const int64_t a = doc_off[d] - doc_off[0], b = doc_off[d + 1] - doc_off[0];
    if (b < a) raise(LDA_ERR_INVALID_ARG, "doc_off not monotone");
    for (int64_t i = a; i < b; ++i) {
      if (words[i] < 0 || words[i] >= V_) raise(LDA_ERR_INVALID_ARG, "word id outside the alphabet");
      words_.push_back(words[i]);
    }
    doc_off_.push_back(base + b);
    const bool has = sources && sources[d];
    sources_.push_back(has ? sources[d] : "");
    has_source_.push_back(has ? 1 : 0);
  }
}

void ParallelTopicModel::log(const std::string& line) const {
  if (verbosity_ > 0) {
    std::fputs(line.c_str(), stderr);
    std::fputc('\n', stderr);
  }
}

void ParallelTopicModel::ensureShards() {
  if (shards_ && !shards_dirty_) return;
  if (V_ < 1) raise(LDA_ERR_STATE, "no alphabet: call addInstances first");
  const std::vector<int32_t> keep = z_cache_;  // saved by markDirty (may be shorter than N)
  shards_.reset();
  const int64_t D = numDocs(), N = numTokens();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) raise(LDA_ERR_DEVICE, "no HIP device");
  // explicit placement (setDevices) or setNumThreads' plan
  const int G = devices_.empty() ? plan_shards(num_threads_, ndev, N, V_, K_, D)
                                 : (int)std::min<int64_t>((int64_t)devices_.size(), std::max<int64_t>(D, 1));
  for (int32_t d : devices_)
    if (d < 0 || d >= ndev) raise(LDA_ERR_INVALID_ARG, "setDevices: device ordinal out of range");
  auto sg = std::make_unique<ShardGroup>();
  for (int g = 0; g < G; ++g) sg->dev.push_back(devices_.empty() ? g : devices_[(size_t)g]);
  // token-balanced contiguous document ranges (the cuts Mallet makes by
  // document count; tokens balance the GPUs' work)
  sg->doc_begin.push_back(0);
  for (int g = 1; g < G; ++g) {
    const int64_t target = N * g / G;
    int64_t d = std::lower_bound(doc_off_.begin(), doc_off_.end(), target) - doc_off_.begin();
    d = std::max(d, sg->doc_begin.back());
    sg->doc_begin.push_back(std::min(d, D));
  }
  sg->doc_begin.push_back(D);
  for (int g = 0; g < G; ++g) {
    const int64_t d0 = sg->doc_begin[g], d1 = sg->doc_begin[g + 1];
    lda_config cfg{};
    cfg.num_topics = K_;
    cfg.num_types = V_;
    cfg.num_docs = d1 - d0;
    cfg.alpha = alpha_.data();
    cfg.beta = beta_;
    cfg.seed = seed_;
    cfg.device = sg->dev[(size_t)g];
    cfg.sampler = sampler_;
    cfg.token_base = doc_off_[d0];
    cfg.tokens_per_range = 0;
    lda_ctx* c = nullptr;
    const int32_t* w = words_.empty() ? nullptr : words_.data() + doc_off_[d0];
    check(lda_create(&c, &cfg, doc_off_.data() + d0, w, nullptr), "lda_create");
    sg->ctx.push_back(c);
  }
  // documents already in the model keep their topics
  if (!keep.empty()) {
    for (int g = 0; g < G; ++g) {
      const int64_t t0 = doc_off_[sg->doc_begin[g]], t1 = doc_off_[sg->doc_begin[g + 1]];
      if (t0 >= (int64_t)keep.size() || t1 == t0) continue;
      std::vector<int32_t> z((size_t)(t1 - t0));
      check(lda_get_z(sg->ctx[g], z.data()), "lda_get_z");
      const int64_t m = std::min<int64_t>(t1, (int64_t)keep.size());
      std::copy(keep.begin() + t0, keep.begin() + m, z.begin());
      check(lda_set_z(sg->ctx[g], z.data()), "lda_set_z");
    }
  }
  sg->init_exchange();
  for (int g = 0; g < G; ++g)
    sg->max_tokens = std::max(sg->max_tokens, doc_off_[sg->doc_begin[(size_t)g + 1]] - doc_off_[sg->doc_begin[(size_t)g]]);
  {
    const char* e = std::getenv("LDA_EXCHANGE_INT32");
    sg->compact = compact_exchange_ && !(e && e[0] == '1');
    const char* lc = std::getenv("LDA_LOCAL_COMPACT");
    sg->local_compact = lc && lc[0] == '1';
    if (sg->use_compact()) sg->init_cells(lda_padded_topics(K_));
  }
  if (G > 1) {
    // shards recount (or keep a delta) in the same sweeps: the smallest
    // AUTO recount count of any shard on all of them
    int32_t rmin = INT32_MAX;
    for (auto c : sg->ctx) {
      int32_t mode = 0, r = 0;
      check(lda_get_count_update(c, &mode, &r), "lda_get_count_update");
      rmin = std::min(rmin, r);
    }
    for (auto c : sg->ctx) {
      int32_t mode = 0;
      check(lda_get_count_update(c, &mode, nullptr), "lda_get_count_update");
      if (mode == LDA_COUNT_AUTO) check(lda_set_count_update(c, LDA_COUNT_AUTO, rmin), "lda_set_count_update");
    }
  }
  // the shards' local counts are the pending delta: sum them, apply
  sg->reduce();
  sg->apply();
  sg->set_parts(exchange_parts_);
  for (auto c : sg->ctx) check(lda_set_sweep(c, sweep_), "lda_set_sweep");
  shards_ = std::move(sg);
  applySweepSchedule();
  shards_dirty_ = false;
  z_dirty_ = true;
  // word totals never change between addInstances calls: the bound of beta's
  // countHistogram is taken once here, not by an O(N) pass per optimisation
  {
    std::vector<int32_t> totals((size_t)V_, 0);
    for (int32_t w : words_) totals[(size_t)w]++;
    max_word_total_ = totals.empty() ? 0 : *std::max_element(totals.begin(), totals.end());
  }
  int32_t m = 0;
  for (int64_t d = 0; d < D; ++d) m = std::max<int32_t>(m, (int32_t)(doc_off_[d + 1] - doc_off_[d]));
  if (m != max_doc_len_) {  // statistics gathered so far stay valid unless the shape changes
    max_doc_len_ = m;
    doc_len_counts_.assign((size_t)max_doc_len_ + 1, 0);
    topic_doc_counts_.assign((size_t)K_ * (max_doc_len_ + 1), 0);
  }
}

std::vector<int32_t> ParallelTopicModel::topics() {
  ensureShards();  // documents added since the last sweep get their initial topics
  if (z_dirty_) {
    z_cache_.assign((size_t)numTokens(), 0);
    for (size_t g = 0; g < shards_->ctx.size(); ++g) {
      const int64_t t0 = doc_off_[shards_->doc_begin[g]];
      check(lda_get_z(shards_->ctx[g], z_cache_.data() + t0), "lda_get_z");
    }
    z_dirty_ = false;
  }
  return z_cache_;
}

void ParallelTopicModel::counts(int32_t* nw, int32_t* nwsum) {
  ensureShards();
  check(lda_get_counts(shards_->ctx[0], nw, nwsum, nullptr, nullptr), "lda_get_counts");
}

double ParallelTopicModel::modelLogLikelihood() {
  ensureShards();
  double doc_total = 0.0, word_part = 0.0;
  for (size_t g = 0; g < shards_->ctx.size(); ++g) {
    double dp = 0.0, wp = 0.0;
    check(lda_log_likelihood_parts(shards_->ctx[g], &dp, &wp), "lda_log_likelihood_parts");
    doc_total += dp;
    if (g == 0) word_part = wp;
  }
  return doc_total + word_part;
}

void ParallelTopicModel::optimizeAlpha() {
  const int64_t W = (int64_t)max_doc_len_ + 1;
  if (symmetric_alpha_) {
    // every topic's histogram pooled into one (Mallet keeps it in topic 0's row)
    std::vector<int32_t> pooled((size_t)W, 0);
    for (int k = 0; k < K_; ++k)
      for (int64_t i = 0; i < W; ++i) pooled[(size_t)i] += topic_doc_counts_[(size_t)(k * W + i)];
    std::vector<int64_t> lens;
    std::vector<int32_t> cnt;
    for (int64_t n = 0; n < W; ++n)
      if (doc_len_counts_[(size_t)n] > 0) {
        lens.push_back(n);
        cnt.push_back(doc_len_counts_[(size_t)n]);
      }
    double a = 0.0;
    check(lda_learn_symmetric_concentration(pooled.data(), W - 1, lens.data(), cnt.data(),
                                            (int64_t)lens.size(), K_, alpha_sum_, &a),
          "lda_learn_symmetric_concentration");
    alpha_sum_ = a;
    std::fill(alpha_.begin(), alpha_.end(), alpha_sum_ / K_);
  } else {
    double s = 0.0;
    check(lda_learn_parameters(alpha_.data(), K_, topic_doc_counts_.data(), doc_len_counts_.data(),
                               max_doc_len_, 1.001, 1.0, 1, &s),
          "lda_learn_parameters");
    alpha_sum_ = s;
  }
  std::fill(doc_len_counts_.begin(), doc_len_counts_.end(), 0);
  std::fill(topic_doc_counts_.begin(), topic_doc_counts_.end(), 0);
}

void ParallelTopicModel::optimizeBeta(const std::vector<int32_t>& hist, const std::vector<int32_t>& nwsum) {
  // countHistogram: nw cells by count, up to the largest word total (hist);
  // topicSizeHistogram, sparse: (tokens in topic, number of topics)
  const int64_t max_count = max_word_total_;
  std::vector<int64_t> sizes(nwsum.begin(), nwsum.end());
  std::sort(sizes.begin(), sizes.end());
  std::vector<int64_t> lens;
  std::vector<int32_t> cnt;
  for (int64_t s : sizes) {
    if (!lens.empty() && lens.back() == s) {
      cnt.back()++;
    } else {
      lens.push_back(s);
      cnt.push_back(1);
    }
  }
  double beta_sum = beta_ * V_;
  check(lda_learn_symmetric_concentration(hist.data(), max_count, lens.data(), cnt.data(),
                                          (int64_t)lens.size(), V_, beta_sum, &beta_sum),
        "lda_learn_symmetric_concentration");
  beta_ = beta_sum / V_;
}

void ParallelTopicModel::estimate() {
  ensureShards();
  ll_trace_.clear();
  held_trace_.clear();
  const double total_tokens = (double)numTokens();
  // Mallet's estimate() builds new WorkerRunnables whose alpha statistics
  // start empty (WorkerRunnable.initializeAlphaStatistics): statistics still
  // pending from an earlier estimate() are not carried into this one
  std::fill(doc_len_counts_.begin(), doc_len_counts_.end(), 0);
  std::fill(topic_doc_counts_.begin(), topic_doc_counts_.end(), 0);
  for (auto c : shards_->ctx) check(lda_doc_topic_histograms_clear(c), "lda_doc_topic_histograms_clear");
  // LL/token every 10 sweeps without stopping the sweeps: the kernels are
  // enqueued behind the sweep and their sums collected (and logged) in
  // batches, and at the end
  std::vector<std::pair<int32_t, std::vector<int64_t>>> ll_pending;
  auto collect_ll = [&]() {
    for (const auto& p : ll_pending) {
      double ll = 0.0;
      for (size_t g = 0; g < shards_->ctx.size(); ++g) {
        double dp = 0.0, wp = 0.0;
        check(lda_log_likelihood_collect(shards_->ctx[g], p.second[g], &dp, &wp), "lda_log_likelihood_collect");
        ll += dp + (g == 0 ? wp : 0.0);   // the word part is global: once
      }
      ll /= total_tokens;
      ll_trace_.emplace_back(p.first, ll);
      log("<" + std::to_string(p.first) + "> LL/token: " + java_number5(ll));
    }
    ll_pending.clear();
  };
  // iterations after which something besides the sweep happens (statistics,
  // optimisation, LL), or before which the topics are shown: the sweeps in
  // between run as one batch
  auto work_after = [&](int32_t i) {
    const bool opt = i > burnin_period_ && optimize_interval_ != 0;
    return i % 10 == 0 || (opt && (i % save_sample_interval_ == 0 || i % optimize_interval_ == 0)) ||
           (held_interval_ > 0 && i % held_interval_ == 0);
  };
  auto show_before = [&](int32_t i) { return show_topics_interval_ != 0 && i % show_topics_interval_ == 0; };
  for (int32_t it = 1; it <= num_iterations_; ++it) {
    if (show_before(it)) {
      collect_ll();
      // log() discards the text when silent: do not compute it then (the
      // sweeps are batched the same way either way)
      if (verbosity_ > 0) log("\n" + displayTopWords(words_per_topic_, false));
    }
    int32_t last = it;
    while (last < num_iterations_ && !work_after(last) && !show_before(last + 1)) ++last;
    shards_->sweeps(last - it + 1);
    it = last;
    z_dirty_ = true;
    const bool opt = it > burnin_period_ && optimize_interval_ != 0;
    if (opt && it % save_sample_interval_ == 0)
      for (auto c : shards_->ctx)
        check(lda_doc_topic_histograms_accumulate(c, max_doc_len_), "lda_doc_topic_histograms_accumulate");
    if (opt && it % optimize_interval_ == 0) {
      // every shard's alpha statistics (summed); the count histogram and
      // nwsum of the global counts from shard 0; one wait per shard
      std::vector<int32_t> hist((size_t)max_word_total_ + 1, 0), nwsum((size_t)K_);
      for (size_t g = 0; g < shards_->ctx.size(); ++g)
        check(lda_hyper_statistics(shards_->ctx[g], max_doc_len_, doc_len_counts_.data(), topic_doc_counts_.data(),
                                   max_word_total_, g == 0 ? hist.data() : nullptr,
                                   g == 0 ? nwsum.data() : nullptr),
              "lda_hyper_statistics");
      optimizeAlpha();
      optimizeBeta(hist, nwsum);
      for (auto c : shards_->ctx) check(lda_set_alpha_beta(c, alpha_.data(), beta_), "lda_set_alpha_beta");
    }
    if (it % 10 == 0) {
      if (print_log_likelihood_) {
        std::vector<int64_t> tickets(shards_->ctx.size());
        for (size_t g = 0; g < shards_->ctx.size(); ++g)
          check(lda_log_likelihood_enqueue(shards_->ctx[g], &tickets[g]), "lda_log_likelihood_enqueue");
        ll_pending.emplace_back(it, std::move(tickets));
        if (ll_pending.size() >= 8) collect_ll();
      } else {
        log("<" + std::to_string(it) + ">");
      }
    }
    if (held_interval_ > 0 && it % held_interval_ == 0) {
      // the held-out set against the counts as they stand after this sweep:
      // reads nw / nwsum on shard 0 and writes only its own scratch
      collect_ll();   // keeps the log in iteration order
      const int64_t Dh = (int64_t)held_off_.size() - 1;
      std::vector<double> doc_ll((size_t)Dh);
      int64_t scored = 0;
      const double ll = evaluate(Dh, held_off_.data(), held_words_.data(), held_iterations_, held_thinning_,
                                 held_burn_in_, held_seed_, doc_ll.data(), &scored, nullptr);
      const double per_token = scored > 0 ? ll / (double)scored : 0.0;
      held_trace_.emplace_back(it, per_token);
      log("<" + std::to_string(it) + "> held-out LL/token: " + java_number5(per_token));
    }
  }
  collect_ll();
  // statistics gathered after the last optimisation are dropped, as Mallet's
  // runnables are
  for (auto c : shards_->ctx) check(lda_doc_topic_histograms_clear(c), "lda_doc_topic_histograms_clear");
  // Mallet's estimate() returns when the sweeps are done: wait for the shards'
  // streams (a kernel fault surfaces here, not in a later call)
  for (auto c : shards_->ctx) check(lda_synchronize(c), "lda_synchronize");
}

void ParallelTopicModel::topWords(int32_t n, int32_t* word_ids, int32_t* counts) {
  if (n < 1 || n > LDA_TOP_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_TOP_WORDS_MAX]");
  if (!word_ids || !counts) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  check(lda_top_words(shards_->ctx[0], n, word_ids, counts), "lda_top_words");
}

namespace {
// lda_relevant_words' argument checks, in its order, before any shard is built
void checkRelevance(int32_t n, int32_t L, const double* lambdas) {
  if (n < 1 || n > LDA_TOP_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_TOP_WORDS_MAX]");
  if (L < 1 || L > LDA_RELEVANCE_LAMBDAS_MAX) raise(LDA_ERR_INVALID_ARG, "L must be in [1, LDA_RELEVANCE_LAMBDAS_MAX]");
  if (!lambdas) raise(LDA_ERR_INVALID_ARG, "null lambdas");
  for (int32_t l = 0; l < L; ++l)
    if (!std::isfinite(lambdas[l]) || !(lambdas[l] >= 0.0) || !(lambdas[l] <= 1.0))
      raise(LDA_ERR_INVALID_ARG, "every lambda must be finite and in [0, 1]");
}
}  // namespace

void ParallelTopicModel::relevantWords(int32_t n, int32_t L, const double* lambdas, int32_t* word_ids, int32_t* counts,
                                       int64_t* totals, double* logprob, double* loglift) {
  checkRelevance(n, L, lambdas);
  if (!word_ids || !counts || !totals || !logprob || !loglift) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  check(lda_relevant_words(shards_->ctx[0], n, L, lambdas, word_ids, counts, totals, logprob, loglift),
        "lda_relevant_words");
}

void ParallelTopicModel::salientWords(int32_t n, int32_t* word_ids, int64_t* totals, double* saliency,
                                      double* distinctiveness) {
  if (n < 1 || n > LDA_SALIENT_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_SALIENT_WORDS_MAX]");
  if (!word_ids || !totals || !saliency || !distinctiveness) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  check(lda_salient_words(shards_->ctx[0], n, word_ids, totals, saliency, distinctiveness), "lda_salient_words");
}

void ParallelTopicModel::wordRows(int64_t M, const int32_t* word_ids, int32_t* rows, int64_t* totals) {
  if (M < 0) raise(LDA_ERR_INVALID_ARG, "bad sizes");
  if (M > 0 && !word_ids) raise(LDA_ERR_INVALID_ARG, "null word list");
  for (int64_t j = 0; j < M; ++j)
    if (word_ids[j] < 0 || word_ids[j] >= numTypes()) raise(LDA_ERR_INVALID_ARG, "word id out of range [0, V)");
  if (M == 0) return;
  if (!rows || !totals) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  check(lda_word_rows(shards_->ctx[0], M, word_ids, rows, totals), "lda_word_rows");
}

double relevanceOf(double lambda, double logprob, double loglift) {
  return logprob - (1.0 - lambda) * (logprob - loglift);
}

std::string relevantWordsFormat(int32_t K, int32_t n, double lambda, const int32_t* word_ids, const int32_t* counts,
                                const int64_t* totals, const double* logprob, const double* loglift,
                                const std::function<std::string(int32_t)>& name) {
  std::string out = "#topic rank word count total relevance logprob loglift\n";
  for (int32_t k = 0; k < K; ++k)
    for (int32_t i = 0; i < n; ++i) {
      const size_t at = (size_t)k * n + i;
      if (word_ids[at] < 0) break;
      out += std::to_string(k) + " " + std::to_string(i) + " " + name(word_ids[at]) + " " + std::to_string(counts[at]) +
             " " + std::to_string(totals[at]) + " " + java_double(relevanceOf(lambda, logprob[at], loglift[at])) + " " +
             java_double(logprob[at]) + " " + java_double(loglift[at]) + "\n";
    }
  return out;
}

std::string ParallelTopicModel::relevantWordsText(int32_t n, double lambda) {
  checkRelevance(n, 1, &lambda);
  const size_t cells = (size_t)K_ * (size_t)n;
  std::vector<int32_t> ids(cells), cnt(cells);
  std::vector<int64_t> tot(cells);
  std::vector<double> lp(cells), ll(cells);
  relevantWords(n, 1, &lambda, ids.data(), cnt.data(), tot.data(), lp.data(), ll.data());
  return relevantWordsFormat(K_, n, lambda, ids.data(), cnt.data(), tot.data(), lp.data(), ll.data(), [&](int32_t w) {
    return alphabet_.empty() ? std::to_string(w) : alphabet_[(size_t)w];
  });
}

namespace {
// the arguments of topicDistances / nearestTopics (n null: no n), in
// lda_topic_distances' order, before any shard is built
void checkTopicPair(const ParallelTopicModel& m, const ParallelTopicModel* other, int32_t metric, const int32_t* n,
                    bool outputs) {
  if (metric < LDA_TOPIC_COSINE || metric > LDA_TOPIC_KL)
    raise(LDA_ERR_INVALID_ARG, "metric must be LDA_TOPIC_COSINE, _HELLINGER, _JS or _KL");
  if (n && (*n < 1 || *n > LDA_TOPIC_NEAREST_MAX)) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_TOPIC_NEAREST_MAX]");
  if (!outputs) raise(LDA_ERR_INVALID_ARG, "null output");
  if (other && other->numTypes() != m.numTypes())
    raise(LDA_ERR_INVALID_ARG, "the two models differ in num_types (V)");
}
}  // namespace

void ParallelTopicModel::topicDistances(ParallelTopicModel* other, int32_t metric, double* out) {
  checkTopicPair(*this, other, metric, nullptr, out != nullptr);
  ensureShards();
  if (other && other != this) other->ensureShards();
  check(lda_topic_distances(shards_->ctx[0], other ? other->shards_->ctx[0] : nullptr, metric, out),
        "lda_topic_distances");
}

void ParallelTopicModel::nearestTopics(ParallelTopicModel* other, int32_t metric, int32_t n, int32_t* topics,
                                       double* values) {
  checkTopicPair(*this, other, metric, &n, topics && values);
  ensureShards();
  if (other && other != this) other->ensureShards();
  check(lda_topic_nearest(shards_->ctx[0], other ? other->shards_->ctx[0] : nullptr, metric, n, topics, values),
        "lda_topic_nearest");
}

namespace {
// the arguments of documentDistances / nearestDocuments / documentNeighbors
// (n null: no n; own: the queries are the model's documents), in
// lda_doc_distances' order, before any shard is built.  Without a list the
// documents are all D of them.
void checkDocNear(int32_t K, int64_t D, int32_t metric, const int32_t* n, bool own, const double* theta,
                  const int32_t* counts, bool outputs, int64_t Q, int64_t M, const int64_t* docs,
                  const int32_t* min_tokens, const int64_t* skip) {
  if (metric < LDA_TOPIC_COSINE || metric > LDA_TOPIC_JS)
    raise(LDA_ERR_INVALID_ARG, "metric must be LDA_TOPIC_COSINE, _HELLINGER or _JS");
  if (n && (*n < 1 || *n > LDA_DOC_NEAREST_MAX)) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_DOC_NEAREST_MAX]");
  if (!own && (theta != nullptr) == (counts != nullptr))
    raise(LDA_ERR_INVALID_ARG, "exactly one of theta / counts must be given");
  const bool nearest = n && !own;
  if (Q > 0 && (nearest || M > 0) && !outputs) raise(LDA_ERR_INVALID_ARG, "null output");
  if (Q < 0 || M < 0) raise(LDA_ERR_INVALID_ARG, "bad sizes");
  if (!nearest) {
    if (!docs && M != D) raise(LDA_ERR_INVALID_ARG, "without a document list M must be the number of documents");
    for (int64_t j = 0; docs && j < M; ++j)
      if (docs[j] < 0 || docs[j] >= D) raise(LDA_ERR_INVALID_ARG, "document id out of range [0, D)");
  }
  if (min_tokens && *min_tokens < 1) raise(LDA_ERR_INVALID_ARG, "min_tokens must be at least 1");
  for (int64_t q = 0; skip && q < Q; ++q)
    if (skip[q] < -1 || skip[q] >= D) raise(LDA_ERR_INVALID_ARG, "skip id out of range [-1, D)");
  for (int64_t q = 0; theta && q < Q; ++q) {
    const double* row = theta + (size_t)q * K;
    double sum = 0.0, tq2 = 0.0;
    for (int k = 0; k < K; ++k) {
      if (!(row[k] >= 0.0) || !std::isfinite(row[k]))
        raise(LDA_ERR_INVALID_ARG, "theta holds a negative or non-finite entry");
      sum += row[k];
      tq2 += row[k] * row[k];
    }
    if (!(sum > 0.0) || !(tq2 > 0.0) || !std::isfinite(tq2))
      raise(LDA_ERR_INVALID_ARG, "a theta row sums to zero (or its squared norm leaves fp64's range)");
  }
  for (size_t i = 0; counts && i < (size_t)Q * (size_t)K; ++i)
    if (counts[i] < 0) raise(LDA_ERR_INVALID_ARG, "counts holds a negative entry");
}

// queries per round of documentNeighbors over several shards
constexpr int64_t NEIGHBOR_QUERIES = 1024;
}  // namespace

void ParallelTopicModel::documentDistances(int32_t metric, int64_t Q, const double* theta, const int32_t* counts,
                                           int64_t M, const int64_t* docs, double* out) {
  checkDocNear(K_, numDocs(), metric, nullptr, false, theta, counts, out != nullptr, Q, M, docs, nullptr, nullptr);
  if (Q == 0 || M == 0) return;
  ensureShards();
  const std::vector<int64_t>& begin = shards_->doc_begin;
  const size_t G = shards_->ctx.size();
  std::vector<double> part;
  if (!docs) {
    for (size_t g = 0; g < G; ++g) {
      const int64_t d0 = begin[g], m = begin[g + 1] - d0;
      if (m == 0) continue;
      if (G == 1) {
        check(lda_doc_distances(shards_->ctx[g], metric, Q, theta, counts, 0, m, nullptr, out), "lda_doc_distances");
        return;
      }
      part.resize((size_t)Q * m);
      check(lda_doc_distances(shards_->ctx[g], metric, Q, theta, counts, 0, m, nullptr, part.data()),
            "lda_doc_distances");
      for (int64_t q = 0; q < Q; ++q) std::copy(part.begin() + q * m, part.begin() + (q + 1) * m, out + q * M + d0);
    }
    return;
  }
  // the list's documents by shard (shard-local ids), and where each goes in
  // the caller's order
  std::vector<std::vector<int64_t>> local(G), pos(G);
  for (int64_t j = 0; j < M; ++j) {
    const size_t g = (size_t)(std::upper_bound(begin.begin(), begin.end(), docs[j]) - begin.begin()) - 1;
    local[g].push_back(docs[j] - begin[g]);
    pos[g].push_back(j);
  }
  for (size_t g = 0; g < G; ++g) {
    const int64_t m = (int64_t)local[g].size();
    if (m == 0) continue;
    part.resize((size_t)Q * m);
    check(lda_doc_distances(shards_->ctx[g], metric, Q, theta, counts, 0, m, local[g].data(), part.data()),
          "lda_doc_distances");
    for (int64_t q = 0; q < Q; ++q)
      for (int64_t i = 0; i < m; ++i) out[q * M + pos[g][(size_t)i]] = part[(size_t)(q * m + i)];
  }
}

void ParallelTopicModel::nearestDocuments(int32_t metric, int32_t n, int64_t Q, const double* theta,
                                          const int32_t* counts, const int64_t* skip, int32_t min_tokens,
                                          int64_t* doc_ids, double* values) {
  checkDocNear(K_, numDocs(), metric, &n, false, theta, counts, doc_ids && values, Q, 0, nullptr, &min_tokens, skip);
  if (Q == 0) return;
  ensureShards();
  const std::vector<int64_t>& begin = shards_->doc_begin;
  const size_t G = shards_->ctx.size(), cells = (size_t)Q * (size_t)n;
  if (G == 1) {
    check(lda_doc_nearest(shards_->ctx[0], metric, n, Q, theta, counts, skip, min_tokens, doc_ids, values),
          "lda_doc_nearest");
    return;
  }
  std::vector<int64_t> ids(G * cells), local((size_t)Q);
  std::vector<double> vals(G * cells);
  for (size_t g = 0; g < G; ++g) {
    for (int64_t q = 0; skip && q < Q; ++q)
      local[(size_t)q] = skip[q] >= begin[g] && skip[q] < begin[g + 1] ? skip[q] - begin[g] : -1;
    check(lda_doc_nearest(shards_->ctx[g], metric, n, Q, theta, counts, skip ? local.data() : nullptr, min_tokens,
                          ids.data() + g * cells, vals.data() + g * cells),
          "lda_doc_nearest");
  }
  // per query the best n of the shards' candidates by (value in the metric's
  // order, global id ascending); the values are the device's bits
  const bool descending = metric == LDA_TOPIC_COSINE;
  std::vector<std::pair<double, int64_t>> cand;
  for (int64_t q = 0; q < Q; ++q) {
    cand.clear();
    for (size_t g = 0; g < G; ++g)
      for (int32_t i = 0; i < n; ++i) {
        const size_t at = g * cells + (size_t)q * n + i;
        if (ids[at] < 0) break;
        cand.emplace_back(vals[at], ids[at] + begin[g]);
      }
    std::sort(cand.begin(), cand.end(), [descending](const auto& a, const auto& b) {
      if (a.first != b.first) return descending ? a.first > b.first : a.first < b.first;
      return a.second < b.second;
    });
    for (int32_t i = 0; i < n; ++i) {
      const size_t o = (size_t)q * n + i;
      const bool has = (size_t)i < cand.size();
      doc_ids[o] = has ? cand[(size_t)i].second : -1;
      values[o] = has ? cand[(size_t)i].first : std::numeric_limits<double>::quiet_NaN();
    }
  }
}

void ParallelTopicModel::documentNeighbors(int32_t metric, int32_t n, int64_t M, const int64_t* docs,
                                           int32_t min_tokens, int64_t* doc_ids, double* values) {
  checkDocNear(K_, numDocs(), metric, &n, true, nullptr, nullptr, doc_ids && values, M, M, docs, &min_tokens, nullptr);
  if (M == 0) return;
  ensureShards();
  if (shards_->ctx.size() == 1) {
    check(lda_doc_neighbors(shards_->ctx[0], metric, n, 0, M, docs, min_tokens, doc_ids, values),
          "lda_doc_neighbors");
    return;
  }
  std::vector<int64_t> own;
  std::vector<int32_t> nd;
  for (int64_t q0 = 0; q0 < M; q0 += NEIGHBOR_QUERIES) {
    const int64_t qn = std::min<int64_t>(NEIGHBOR_QUERIES, M - q0);
    own.resize((size_t)qn);
    for (int64_t q = 0; q < qn; ++q) own[(size_t)q] = docs ? docs[q0 + q] : q0 + q;
    nd.resize((size_t)qn * K_);
    docCounts(qn, own.data(), nd.data());
    nearestDocuments(metric, n, qn, nullptr, nd.data(), own.data(), min_tokens, doc_ids + q0 * n, values + q0 * n);
  }
}

std::string documentNeighborsFormat(int64_t M, int32_t n, const int64_t* docs, const int64_t* doc_ids,
                                    const double* values, const std::function<std::string(int64_t)>& name) {
  std::string out = "#doc neighbor name value\n";
  for (int64_t j = 0; j < M; ++j)
    for (int32_t i = 0; i < n; ++i) {
      const size_t at = (size_t)j * n + i;
      if (doc_ids[at] < 0) break;
      out += std::to_string(docs ? docs[j] : j) + " " + std::to_string(doc_ids[at]) + " " + name(doc_ids[at]) + " " +
             java_double(values[at]) + "\n";
    }
  return out;
}

std::string ParallelTopicModel::documentNeighborsText(int32_t n, int32_t metric, int32_t min_tokens) {
  const int64_t D = numDocs();
  checkDocNear(K_, D, metric, &n, true, nullptr, nullptr, true, D, D, nullptr, &min_tokens, nullptr);
  std::vector<int64_t> ids((size_t)D * n);
  std::vector<double> vals((size_t)D * n);
  documentNeighbors(metric, n, D, nullptr, min_tokens, ids.data(), vals.data());
  return documentNeighborsFormat(D, n, nullptr, ids.data(), vals.data(), [&](int64_t d) {
    return has_source_[(size_t)d] ? sources_[(size_t)d] : std::string("null-source");
  });
}

void ParallelTopicModel::docReadout(int32_t mtop, int64_t M, const int64_t* docs, int32_t* out0, int32_t* out1) {
  if (M < 0) raise(LDA_ERR_INVALID_ARG, "bad sizes");
  const int64_t D = numDocs();
  if (!docs && M != D) raise(LDA_ERR_INVALID_ARG, "without a document list M must be the number of documents");
  for (int64_t j = 0; docs && j < M; ++j)
    if (docs[j] < 0 || docs[j] >= D) raise(LDA_ERR_INVALID_ARG, "document id out of range [0, D)");
  if (M == 0) return;
  if (!out0 || (mtop > 0 && !out1)) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  const int64_t width = mtop > 0 ? mtop : K_;
  auto call = [&](size_t g, int64_t m, const int64_t* local, int32_t* o0, int32_t* o1) {
    if (mtop > 0)
      check(lda_doc_top_topics(shards_->ctx[g], mtop, 0, m, local, o0, o1), "lda_doc_top_topics");
    else
      check(lda_doc_counts(shards_->ctx[g], 0, m, local, o0), "lda_doc_counts");
  };
  const std::vector<int64_t>& begin = shards_->doc_begin;
  const size_t G = shards_->ctx.size();
  if (!docs) {
    // the shards' document ranges are consecutive: each writes its own rows
    for (size_t g = 0; g < G; ++g) {
      const int64_t d0 = begin[g], m = begin[g + 1] - d0;
      if (m > 0) call(g, m, nullptr, out0 + d0 * width, out1 ? out1 + d0 * width : nullptr);
    }
    return;
  }
  if (G == 1) {
    call(0, M, docs, out0, out1);
    return;
  }
  std::vector<std::vector<int64_t>> local(G), pos(G);
  for (int64_t j = 0; j < M; ++j) {
    const size_t g = (size_t)(std::upper_bound(begin.begin(), begin.end(), docs[j]) - begin.begin()) - 1;
    local[g].push_back(docs[j] - begin[g]);
    pos[g].push_back(j);
  }
  std::vector<int32_t> p0, p1;
  for (size_t g = 0; g < G; ++g) {
    const int64_t m = (int64_t)local[g].size();
    if (m == 0) continue;
    p0.resize((size_t)(m * width));
    if (mtop > 0) p1.resize((size_t)(m * width));
    call(g, m, local[g].data(), p0.data(), p1.data());
    for (int64_t i = 0; i < m; ++i) {
      const int64_t j = pos[g][(size_t)i];
      std::copy(p0.begin() + i * width, p0.begin() + (i + 1) * width, out0 + j * width);
      if (mtop > 0) std::copy(p1.begin() + i * width, p1.begin() + (i + 1) * width, out1 + j * width);
    }
  }
}

void ParallelTopicModel::docTopTopics(int32_t mtop, int64_t M, const int64_t* docs, int32_t* topics,
                                      int32_t* counts) {
  if (mtop < 1 || mtop > LDA_TOP_TOPICS_MAX) raise(LDA_ERR_INVALID_ARG, "m must be in [1, LDA_TOP_TOPICS_MAX]");
  docReadout(mtop, M, docs, topics, counts);
}

void ParallelTopicModel::docCounts(int64_t M, const int64_t* docs, int32_t* nd) { docReadout(0, M, docs, nd, nullptr); }

namespace {
// lda_topic_top_docs' argument checks, before any shard is built
void checkTopicDocs(int32_t n, double smoothing, int32_t min_tokens) {
  if (n < 1 || n > LDA_TOPIC_DOCS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_TOPIC_DOCS_MAX]");
  if (!(smoothing >= 0.0) || !std::isfinite(smoothing))
    raise(LDA_ERR_INVALID_ARG, "smoothing must be finite and not negative");
  if (min_tokens < 1) raise(LDA_ERR_INVALID_ARG, "min_tokens must be at least 1");
}
}  // namespace

double topicDocWeight(int32_t K, double smoothing, int32_t count, int32_t length) {
  const double Ks = (double)K * smoothing;
  return ((double)count + smoothing) / ((double)length + Ks);
}

void ParallelTopicModel::topicTopDocs(int32_t n, double smoothing, int32_t min_tokens, int64_t* doc_ids,
                                      int32_t* counts, int32_t* lengths) {
  checkTopicDocs(n, smoothing, min_tokens);
  if (!doc_ids || !counts || !lengths) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  const size_t G = shards_->ctx.size(), cells = (size_t)K_ * (size_t)n;
  if (G == 1) {
    check(lda_topic_top_docs(shards_->ctx[0], n, smoothing, min_tokens, doc_ids, counts, lengths),
          "lda_topic_top_docs");
    return;
  }
  // every shard's K x n lists (local ids), then per topic the best n of the
  // shards' candidates by (weight descending, global id ascending), the
  // weight recomputed from (count, length) with the device's expression
  std::vector<int64_t> ids(G * cells);
  std::vector<int32_t> cnt(G * cells), len(G * cells);
  for (size_t g = 0; g < G; ++g)
    check(lda_topic_top_docs(shards_->ctx[g], n, smoothing, min_tokens, ids.data() + g * cells,
                             cnt.data() + g * cells, len.data() + g * cells),
          "lda_topic_top_docs");
  struct Cand {
    double w;
    int64_t id;
    int32_t count, length;
  };
  std::vector<Cand> cand;
  for (int32_t k = 0; k < K_; ++k) {
    cand.clear();
    for (size_t g = 0; g < G; ++g)
      for (int32_t i = 0; i < n; ++i) {
        const size_t at = g * cells + (size_t)k * n + i;
        if (ids[at] < 0) break;
        cand.push_back({topicDocWeight(K_, smoothing, cnt[at], len[at]), ids[at] + shards_->doc_begin[g], cnt[at],
                        len[at]});
      }
    std::sort(cand.begin(), cand.end(),
              [](const Cand& a, const Cand& b) { return a.w > b.w || (a.w == b.w && a.id < b.id); });
    for (int32_t i = 0; i < n; ++i) {
      const size_t o = (size_t)k * n + i;
      const bool has = (size_t)i < cand.size();
      doc_ids[o] = has ? cand[(size_t)i].id : -1;
      counts[o] = has ? cand[(size_t)i].count : 0;
      lengths[o] = has ? cand[(size_t)i].length : 0;
    }
  }
}

std::string topicDocumentsFormat(int32_t K, int32_t n, double smoothing, const int64_t* doc_ids, const int32_t* counts,
                                 const int32_t* lengths, const std::function<std::string(int64_t)>& name) {
  std::string out = "#topic doc name proportion ...\n";
  for (int32_t k = 0; k < K; ++k)
    for (int32_t i = 0; i < n; ++i) {
      const size_t at = (size_t)k * n + i;
      if (doc_ids[at] < 0) break;
      out += std::to_string(k) + " " + std::to_string(doc_ids[at]) + " " + name(doc_ids[at]) + " " +
             java_double(topicDocWeight(K, smoothing, counts[at], lengths[at])) + "\n";
    }
  return out;
}

std::string ParallelTopicModel::topicDocuments(int32_t max, double smoothing, int32_t min_tokens) {
  checkTopicDocs(max, smoothing, min_tokens);
  const size_t cells = (size_t)K_ * (size_t)max;
  std::vector<int64_t> ids(cells);
  std::vector<int32_t> cnt(cells), len(cells);
  topicTopDocs(max, smoothing, min_tokens, ids.data(), cnt.data(), len.data());
  return topicDocumentsFormat(K_, max, smoothing, ids.data(), cnt.data(), len.data(), [&](int64_t d) {
    return has_source_[(size_t)d] ? sources_[(size_t)d] : std::string("null-source");
  });
}

namespace {
// lda_topic_phrases' argument checks, before any shard is built
void checkTopicPhrases(int32_t n, int32_t min_len, int32_t max_len, int32_t min_count) {
  if (n < 1 || n > LDA_PHRASES_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_PHRASES_MAX]");
  if (min_len < 2 || min_len > max_len || max_len > LDA_PHRASE_LEN_MAX)
    raise(LDA_ERR_INVALID_ARG, "the lengths must satisfy 2 <= min_len <= max_len <= LDA_PHRASE_LEN_MAX");
  if (min_count < 1) raise(LDA_ERR_INVALID_ARG, "min_count must be at least 1");
}
}  // namespace

void topicPhrasesBound(int32_t K, int32_t n, int32_t G, const int64_t* shard_counts, const int64_t* totals,
                       int64_t* bound, int32_t* proven) {
  for (int32_t k = 0; k < K; ++k) {
    int64_t B = 0;
    for (int32_t g = 0; g < G; ++g) B += shard_counts[((size_t)g * K + k) * LDA_PHRASES_MAX + LDA_PHRASES_MAX - 1];
    int32_t lead = 0;
    while (lead < n && totals[(size_t)k * n + lead] > B) ++lead;
    bound[k] = B;
    proven[k] = B == 0 ? n : lead;
  }
}

void ParallelTopicModel::topicPhrases(int32_t n, int32_t min_len, int32_t max_len, int32_t min_count,
                                      int32_t* phrase_words, int32_t* lengths, int64_t* counts, int64_t* first,
                                      int64_t* topic_runs, int64_t* topic_distinct, int64_t* skipped_long,
                                      int32_t* proven) {
  checkTopicPhrases(n, min_len, max_len, min_count);
  if (!phrase_words || !lengths || !counts || !first || !topic_runs || !topic_distinct || !skipped_long || !proven)
    raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  const size_t G = shards_->ctx.size(), K = (size_t)K_, L = (size_t)max_len;
  if (G == 1) {
    check(lda_topic_phrases(shards_->ctx[0], n, min_len, max_len, min_count, phrase_words, lengths, counts, first,
                            topic_runs, topic_distinct, skipped_long),
          "lda_topic_phrases");
    std::fill(proven, proven + K, n);
    return;
  }
  // every shard's best LDA_PHRASES_MAX per topic, united by content; the
  // candidates' exact totals and smallest starts from lda_phrase_lookup on
  // every shard; then the order of lda_topic_phrases on the totals
  const size_t M = LDA_PHRASES_MAX, cells = K * M;
  std::vector<int32_t> sw(cells * L), sl(cells);
  std::vector<int64_t> sc(G * cells), sf(cells), runs(K), distinct(K);
  std::fill(topic_runs, topic_runs + K, (int64_t)0);
  std::fill(topic_distinct, topic_distinct + K, (int64_t)-1);
  *skipped_long = 0;
  std::vector<std::map<std::vector<int32_t>, size_t>> seen(K);
  std::vector<int32_t> q_topics, q_words;
  std::vector<int64_t> q_off{0};
  for (size_t g = 0; g < G; ++g) {
    int64_t skipped = 0;
    check(lda_topic_phrases(shards_->ctx[g], (int32_t)M, min_len, max_len, 1, sw.data(), sl.data(),
                            sc.data() + g * cells, sf.data(), runs.data(), distinct.data(), &skipped),
          "lda_topic_phrases");
    *skipped_long += skipped;
    for (size_t k = 0; k < K; ++k) {
      topic_runs[k] += runs[k];
      for (size_t i = 0; i < M && sl[k * M + i] > 0; ++i) {
        const int32_t* w = sw.data() + (k * M + i) * L;
        std::vector<int32_t> ph(w, w + sl[k * M + i]);
        if (seen[k].emplace(ph, q_topics.size()).second) {
          q_topics.push_back((int32_t)k);
          q_words.insert(q_words.end(), ph.begin(), ph.end());
          q_off.push_back((int64_t)q_words.size());
        }
      }
    }
  }
  const size_t Q = q_topics.size();
  std::vector<int64_t> total(Q, 0), start(Q, INT64_MAX), qc(Q), qf(Q);
  for (size_t g = 0; g < G && Q > 0; ++g) {
    check(lda_phrase_lookup(shards_->ctx[g], min_len, max_len, (int64_t)Q, q_topics.data(), q_off.data(),
                            q_words.data(), qc.data(), qf.data()),
          "lda_phrase_lookup");
    const int64_t t0 = doc_off_[(size_t)shards_->doc_begin[g]];
    for (size_t q = 0; q < Q; ++q) {
      total[q] += qc[q];
      if (qf[q] >= 0) start[q] = std::min(start[q], qf[q] + t0);
    }
  }
  std::vector<std::pair<const std::vector<int32_t>*, size_t>> cand;
  for (size_t k = 0; k < K; ++k) {
    cand.clear();
    for (const auto& e : seen[k])
      if (total[e.second] >= min_count) cand.push_back({&e.first, e.second});
    // the map iterates in word order (a prefix first): a stable sort by total
    // descending leaves equal totals in that order
    std::stable_sort(cand.begin(), cand.end(),
                     [&](const auto& a, const auto& b) { return total[a.second] > total[b.second]; });
    for (size_t i = 0; i < (size_t)n; ++i) {
      const size_t o = k * (size_t)n + i;
      const bool has = i < cand.size();
      const size_t len = has ? cand[i].first->size() : 0;
      for (size_t j = 0; j < L; ++j) phrase_words[o * L + j] = j < len ? (*cand[i].first)[j] : -1;
      lengths[o] = (int32_t)len;
      counts[o] = has ? total[cand[i].second] : 0;
      first[o] = has ? start[cand[i].second] : -1;
    }
  }
  std::vector<int64_t> bound(K);
  topicPhrasesBound(K_, n, (int32_t)G, sc.data(), counts, bound.data(), proven);
}

std::string topicPhrasesFormat(int32_t K, int32_t n, int32_t max_len, const int32_t* phrase_words,
                               const int32_t* lengths, const int64_t* counts,
                               const std::function<std::string(int32_t)>& name) {
  std::string out = "#topic rank count phrase\n";
  for (int32_t k = 0; k < K; ++k)
    for (int32_t i = 0; i < n; ++i) {
      const size_t at = (size_t)k * n + i;
      if (lengths[at] <= 0) break;
      out += std::to_string(k) + " " + std::to_string(i) + " " + std::to_string(counts[at]);
      for (int32_t j = 0; j < lengths[at]; ++j) out += " " + name(phrase_words[at * (size_t)max_len + j]);
      out += "\n";
    }
  return out;
}

std::string ParallelTopicModel::topicPhrasesText(int32_t n, int32_t min_len, int32_t max_len, int32_t min_count) {
  checkTopicPhrases(n, min_len, max_len, min_count);
  const size_t K = (size_t)K_, cells = K * (size_t)n;
  std::vector<int32_t> words(cells * (size_t)max_len), len(cells), proven(K);
  std::vector<int64_t> cnt(cells), first(cells), runs(K), distinct(K);
  int64_t skipped = 0;
  topicPhrases(n, min_len, max_len, min_count, words.data(), len.data(), cnt.data(), first.data(), runs.data(),
               distinct.data(), &skipped, proven.data());
  return topicPhrasesFormat(K_, n, max_len, words.data(), len.data(), cnt.data(), [&](int32_t w) {
    return alphabet_.empty() ? std::to_string(w) : alphabet_[(size_t)w];
  });
}

// ---- topic co-occurrence -----------------------------------
namespace {
// lda_topic_cooccurrence's argument checks, before any shard is built
void checkCooccurrence(int64_t min_tokens, int32_t min_count, double min_prop) {
  if (min_tokens < 1) raise(LDA_ERR_INVALID_ARG, "min_tokens must be at least 1");
  if (min_count < 1) raise(LDA_ERR_INVALID_ARG, "min_count must be at least 1");
  if (!(min_prop >= 0.0 && min_prop <= 1.0)) raise(LDA_ERR_INVALID_ARG, "min_prop must be in [0, 1]");
}
void checkMeasure(int32_t measure) {
  if (correlationTable(measure) < 0) raise(LDA_ERR_INVALID_ARG, "unknown measure (LDATM_CORR_*)");
}
}  // namespace

int32_t correlationTable(int32_t measure) {
  switch (measure) {
    case LDATM_CORR_PMI:
    case LDATM_CORR_NPMI:
    case LDATM_CORR_JACCARD:
      return LDATM_COOC_CODOCS;
    case LDATM_CORR_OVERLAP:
      return LDATM_COOC_OVERLAP;
    case LDATM_CORR_COSINE:
    case LDATM_CORR_PEARSON:
      return LDATM_COOC_PRODUCT;
    default:
      return -1;
  }
}

void topicCorrelationFinish(int32_t measure, int32_t K, int64_t docs_used, const int64_t* tokens,
                            const int64_t* present, int32_t table_kind, const int64_t* table, double* out) {
  checkMeasure(measure);
  if (K < 1) raise(LDA_ERR_INVALID_ARG, "K must be at least 1");
  if (docs_used < 0) raise(LDA_ERR_INVALID_ARG, "docs_used must not be negative");
  if (!tokens || !present || !table) raise(LDA_ERR_INVALID_ARG, "null input (tokens, present, table)");
  if (!out) raise(LDA_ERR_INVALID_ARG, "null output");
  if (table_kind != correlationTable(measure))
    raise(LDA_ERR_INVALID_ARG, "wrong table for the measure: pmi, npmi and jaccard take codocs, overlap takes "
                               "overlap, cosine and pearson take product");
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double D = (double)docs_used;
  const size_t Ks = (size_t)K;
  for (size_t k = 0; k < Ks; ++k)
    for (size_t l = 0; l < Ks; ++l) {
      const int64_t t = table[k * Ks + l];
      double v = nan;
      switch (measure) {
        case LDATM_CORR_PMI:
        case LDATM_CORR_NPMI: {
          const int64_t ck = present[k], cl = present[l];
          if (ck == 0 || cl == 0) break;
          const bool npmi = measure == LDATM_CORR_NPMI;
          if (t == 0) {
            v = npmi ? -1.0 : -inf;
          } else if (npmi && t == docs_used) {
            v = 1.0;
          } else {
            const double pmi = std::log(D * (double)t / ((double)ck * (double)cl));
            v = npmi ? pmi / -std::log((double)t / D) : pmi;
          }
          break;
        }
        case LDATM_CORR_JACCARD: {
          const int64_t u = present[k] + present[l] - t;
          if (u != 0) v = (double)t / (double)u;
          break;
        }
        case LDATM_CORR_OVERLAP: {
          const int64_t u = tokens[k] + tokens[l] - t;
          if (u != 0) v = (double)t / (double)u;
          break;
        }
        case LDATM_CORR_COSINE: {
          const int64_t skk = table[k * Ks + k], sll = table[l * Ks + l];
          if (skk != 0 && sll != 0) v = (double)t / (std::sqrt((double)skk) * std::sqrt((double)sll));
          break;
        }
        default: {   // LDATM_CORR_PEARSON: the three terms exactly, then one conversion each
          const __int128 Dp = docs_used, nk = tokens[k], nl = tokens[l];
          const __int128 cov = Dp * t - nk * nl;
          const __int128 vk = Dp * table[k * Ks + k] - nk * nk, vl = Dp * table[l * Ks + l] - nl * nl;
          if (vk != 0 && vl != 0) v = (double)cov / std::sqrt((double)vk * (double)vl);
          break;
        }
      }
      out[k * Ks + l] = v;
    }
}

void topicPartnersSelect(int32_t K, int32_t n, const double* matrix, int32_t* ids, double* values) {
  if (K < 1) raise(LDA_ERR_INVALID_ARG, "K must be at least 1");
  if (n < 1) raise(LDA_ERR_INVALID_ARG, "n must be at least 1");
  if (!matrix) raise(LDA_ERR_INVALID_ARG, "null matrix");
  if (!ids || !values) raise(LDA_ERR_INVALID_ARG, "null output");
  std::vector<int32_t> cand;
  for (int32_t k = 0; k < K; ++k) {
    const double* row = matrix + (size_t)k * (size_t)K;
    cand.clear();
    for (int32_t l = 0; l < K; ++l)
      if (l != k && std::isfinite(row[l])) cand.push_back(l);
    const size_t keep = std::min<size_t>((size_t)n, cand.size());
    std::partial_sort(cand.begin(), cand.begin() + (std::ptrdiff_t)keep, cand.end(),
                      [&](int32_t a, int32_t b) { return row[a] > row[b] || (row[a] == row[b] && a < b); });
    for (int32_t i = 0; i < n; ++i) {
      const bool has = (size_t)i < keep;
      ids[(size_t)k * n + i] = has ? cand[(size_t)i] : -1;
      values[(size_t)k * n + i] = has ? row[cand[(size_t)i]] : std::numeric_limits<double>::quiet_NaN();
    }
  }
}

std::string topicCorrelationsFormat(int32_t K, int32_t n, const int32_t* ids, const double* values) {
  std::string out = "#topic partner value\n";
  for (int32_t k = 0; k < K; ++k)
    for (int32_t i = 0; i < n; ++i) {
      const size_t at = (size_t)k * n + i;
      if (ids[at] < 0) break;
      out += std::to_string(k) + " " + std::to_string(ids[at]) + " " + java_double(values[at]) + "\n";
    }
  return out;
}

void ParallelTopicModel::topicCooccurrence(int64_t min_tokens, int32_t min_count, double min_prop, int64_t* docs_used,
                                           int64_t* tokens, int64_t* present, int64_t* codocs, int64_t* overlap,
                                           int64_t* product) {
  checkCooccurrence(min_tokens, min_count, min_prop);
  if (!docs_used || !tokens || !present)
    raise(LDA_ERR_INVALID_ARG, "null output (docs_used, tokens and present are required)");
  ensureShards();
  const size_t G = shards_->ctx.size(), K = (size_t)K_, cells = K * K;
  check(lda_topic_cooccurrence(shards_->ctx[0], min_tokens, min_count, min_prop, docs_used, tokens, present, codocs,
                               overlap, product),
        "lda_topic_cooccurrence");
  if (G == 1) return;
  // the other shards one at a time into a buffer of one shard's size
  int64_t* outs[3] = {codocs, overlap, product};
  std::vector<int64_t> head(2 * K), tabs[3];
  for (int t = 0; t < 3; ++t)
    if (outs[t]) tabs[t].resize(cells);
  for (size_t g = 1; g < G; ++g) {
    int64_t used = 0;
    check(lda_topic_cooccurrence(shards_->ctx[g], min_tokens, min_count, min_prop, &used, head.data(),
                                 head.data() + K, outs[0] ? tabs[0].data() : nullptr,
                                 outs[1] ? tabs[1].data() : nullptr, outs[2] ? tabs[2].data() : nullptr),
          "lda_topic_cooccurrence");
    *docs_used += used;
    for (size_t k = 0; k < K; ++k) {
      tokens[k] += head[k];
      present[k] += head[K + k];
    }
    for (int t = 0; t < 3; ++t)
      if (outs[t])
        for (size_t i = 0; i < cells; ++i) outs[t][i] += tabs[t][i];
  }
}

void ParallelTopicModel::topicCorrelations(int32_t measure, int64_t min_tokens, int32_t min_count, double min_prop,
                                           double* out) {
  checkMeasure(measure);
  checkCooccurrence(min_tokens, min_count, min_prop);
  if (!out) raise(LDA_ERR_INVALID_ARG, "null output");
  const size_t K = (size_t)K_;
  const int32_t kind = correlationTable(measure);
  int64_t used = 0;
  std::vector<int64_t> tokens(K), present(K), table(K * K);
  topicCooccurrence(min_tokens, min_count, min_prop, &used, tokens.data(), present.data(),
                    kind == LDATM_COOC_CODOCS ? table.data() : nullptr,
                    kind == LDATM_COOC_OVERLAP ? table.data() : nullptr,
                    kind == LDATM_COOC_PRODUCT ? table.data() : nullptr);
  topicCorrelationFinish(measure, K_, used, tokens.data(), present.data(), kind, table.data(), out);
}

void ParallelTopicModel::topicPartners(int32_t measure, int64_t min_tokens, int32_t min_count, double min_prop,
                                       int32_t n, int32_t* ids, double* values) {
  checkMeasure(measure);
  checkCooccurrence(min_tokens, min_count, min_prop);
  if (n < 1) raise(LDA_ERR_INVALID_ARG, "n must be at least 1");
  if (!ids || !values) raise(LDA_ERR_INVALID_ARG, "null output");
  std::vector<double> matrix((size_t)K_ * (size_t)K_);
  topicCorrelations(measure, min_tokens, min_count, min_prop, matrix.data());
  topicPartnersSelect(K_, n, matrix.data(), ids, values);
}

std::string ParallelTopicModel::topicCorrelationsText(int32_t measure, int32_t n, int64_t min_tokens,
                                                      int32_t min_count, double min_prop) {
  checkMeasure(measure);
  checkCooccurrence(min_tokens, min_count, min_prop);
  if (n < 1) raise(LDA_ERR_INVALID_ARG, "n must be at least 1");
  const size_t cells = (size_t)K_ * (size_t)n;
  std::vector<int32_t> ids(cells);
  std::vector<double> values(cells);
  topicPartners(measure, min_tokens, min_count, min_prop, n, ids.data(), values.data());
  return topicCorrelationsFormat(K_, n, ids.data(), values.data());
}

// ---- topics by document group -------------------------------
namespace {
void checkGroupKind(int32_t kind) {
  if (kind < LDATM_GROUP_TOKENS || kind > LDATM_GROUP_LIFT) raise(LDA_ERR_INVALID_ARG, "unknown kind (LDATM_GROUP_*)");
}
// lda_group_topics' host-side argument checks, in its order, before any shard is built
void checkGroups(const int32_t* doc_group, int64_t D, int32_t G) {
  if (D > 0 && !doc_group) raise(LDA_ERR_INVALID_ARG, "null doc_group");
  for (int64_t d = 0; d < D; ++d)
    if (doc_group[d] < -1 || doc_group[d] >= G)
      raise(LDA_ERR_INVALID_ARG, "doc_group[" + std::to_string(d) + "] = " + std::to_string(doc_group[d]) +
                                     " is outside [-1, G)");
}
}  // namespace

void groupPrevalenceFinish(int32_t kind, int32_t G, int32_t K, const int64_t* group_docs, const int64_t* group_tokens,
                           const int64_t* tokens, const int64_t* present, const uint64_t* shares, double* out) {
  checkGroupKind(kind);
  if (G < 1) raise(LDA_ERR_INVALID_ARG, "G must be at least 1");
  if (K < 1) raise(LDA_ERR_INVALID_ARG, "K must be at least 1");
  if (!group_docs || !group_tokens || !tokens)
    raise(LDA_ERR_INVALID_ARG, "null input (group_docs, group_tokens and tokens are required)");
  if (kind == LDATM_GROUP_DOCUMENTS && !present)
    raise(LDA_ERR_INVALID_ARG, "missing table for the kind: documents takes present");
  if (kind == LDATM_GROUP_MEAN && !shares) raise(LDA_ERR_INVALID_ARG, "missing table for the kind: mean takes shares");
  if (!out) raise(LDA_ERR_INVALID_ARG, "null output");
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const size_t Gs = (size_t)G, Ks = (size_t)K;
  // lift's corpus side: N_k and N over the groups
  std::vector<int64_t> nk(Ks, 0);
  int64_t n_all = 0;
  if (kind == LDATM_GROUP_LIFT)
    for (size_t g = 0; g < Gs; ++g) {
      n_all += group_tokens[g];
      for (size_t k = 0; k < Ks; ++k) nk[k] += tokens[g * Ks + k];
    }
  for (size_t g = 0; g < Gs; ++g)
    for (size_t k = 0; k < Ks; ++k) {
      const size_t at = g * Ks + k;
      double v = nan;
      switch (kind) {
        case LDATM_GROUP_TOKENS:
          if (group_tokens[g] != 0) v = (double)tokens[at] / (double)group_tokens[g];
          break;
        case LDATM_GROUP_DOCUMENTS:
          if (group_docs[g] != 0) v = (double)present[at] / (double)group_docs[g];
          break;
        case LDATM_GROUP_MEAN:
          if (group_docs[g] != 0) v = (double)shares[at] / (4294967296.0 * (double)group_docs[g]);
          break;
        default:   // LDATM_GROUP_LIFT
          if (group_tokens[g] == 0 || nk[k] == 0 || n_all == 0) break;
          v = tokens[at] == 0 ? -inf
                              : std::log(((double)tokens[at] / (double)group_tokens[g]) /
                                         ((double)nk[k] / (double)n_all));
          break;
      }
      out[at] = v;
    }
}

void groupTopTopicsSelect(int32_t G, int32_t K, int32_t n, const double* matrix, int32_t* ids, double* values) {
  if (G < 1) raise(LDA_ERR_INVALID_ARG, "G must be at least 1");
  if (K < 1) raise(LDA_ERR_INVALID_ARG, "K must be at least 1");
  if (n < 1) raise(LDA_ERR_INVALID_ARG, "n must be at least 1");
  if (!matrix) raise(LDA_ERR_INVALID_ARG, "null matrix");
  if (!ids || !values) raise(LDA_ERR_INVALID_ARG, "null output");
  std::vector<int32_t> cand;
  for (int32_t g = 0; g < G; ++g) {
    const double* row = matrix + (size_t)g * (size_t)K;
    cand.clear();
    for (int32_t k = 0; k < K; ++k)
      if (std::isfinite(row[k])) cand.push_back(k);
    const size_t keep = std::min<size_t>((size_t)n, cand.size());
    std::partial_sort(cand.begin(), cand.begin() + (std::ptrdiff_t)keep, cand.end(),
                      [&](int32_t a, int32_t b) { return row[a] > row[b] || (row[a] == row[b] && a < b); });
    for (int32_t i = 0; i < n; ++i) {
      const bool has = (size_t)i < keep;
      ids[(size_t)g * n + i] = has ? cand[(size_t)i] : -1;
      values[(size_t)g * n + i] = has ? row[cand[(size_t)i]] : std::numeric_limits<double>::quiet_NaN();
    }
  }
}

std::string groupTopicsFormat(int32_t G, int32_t n, const int32_t* ids, const double* values) {
  std::string out = "#group topic value\n";
  for (int32_t g = 0; g < G; ++g)
    for (int32_t i = 0; i < n; ++i) {
      const size_t at = (size_t)g * n + i;
      if (ids[at] < 0) break;
      out += std::to_string(g) + " " + std::to_string(ids[at]) + " " + java_double(values[at]) + "\n";
    }
  return out;
}

void ParallelTopicModel::groupTopics(const int32_t* doc_group, int32_t G, int64_t min_tokens, int32_t min_count,
                                     double min_prop, int64_t* group_docs, int64_t* group_tokens, int64_t* tokens,
                                     int64_t* present, uint64_t* shares) {
  if (G < 1) raise(LDA_ERR_INVALID_ARG, "G must be at least 1");
  if (!group_docs || !group_tokens || !tokens)
    raise(LDA_ERR_INVALID_ARG, "null output (group_docs, group_tokens and tokens are required)");
  checkCooccurrence(min_tokens, min_count, min_prop);
  checkGroups(doc_group, numDocs(), G);
  if ((int64_t)G * K_ > LDA_GROUP_TOPICS_MAX_CELLS)
    raise(LDA_ERR_UNSUPPORTED, "group topics: G x K above LDA_GROUP_TOPICS_MAX_CELLS");
  ensureShards();
  const size_t S = shards_->ctx.size(), Gs = (size_t)G, cells = Gs * (size_t)K_;
  auto slice = [&](size_t s) { return doc_group ? doc_group + shards_->doc_begin[s] : nullptr; };
  check(lda_group_topics(shards_->ctx[0], slice(0), G, min_tokens, min_count, min_prop, group_docs, group_tokens,
                         tokens, present, shares),
        "lda_group_topics");
  if (S == 1) return;
  // the other shards one at a time into buffers of one shard's size
  std::vector<int64_t> gd(Gs), gt(Gs), tok(cells), pre(present ? cells : 0);
  std::vector<uint64_t> shr(shares ? cells : 0);
  for (size_t s = 1; s < S; ++s) {
    check(lda_group_topics(shards_->ctx[s], slice(s), G, min_tokens, min_count, min_prop, gd.data(), gt.data(),
                           tok.data(), present ? pre.data() : nullptr, shares ? shr.data() : nullptr),
          "lda_group_topics");
    for (size_t g = 0; g < Gs; ++g) {
      group_docs[g] += gd[g];
      group_tokens[g] += gt[g];
    }
    for (size_t i = 0; i < cells; ++i) tokens[i] += tok[i];
    if (present)
      for (size_t i = 0; i < cells; ++i) present[i] += pre[i];
    if (shares)
      for (size_t i = 0; i < cells; ++i) shares[i] += shr[i];
  }
}

void ParallelTopicModel::groupPrevalence(const int32_t* doc_group, int32_t G, int32_t kind, int64_t min_tokens,
                                         int32_t min_count, double min_prop, double* out) {
  checkGroupKind(kind);
  if (G < 1) raise(LDA_ERR_INVALID_ARG, "G must be at least 1");
  checkCooccurrence(min_tokens, min_count, min_prop);
  if (!out) raise(LDA_ERR_INVALID_ARG, "null output");
  const size_t Gs = (size_t)G, cells = Gs * (size_t)K_;
  std::vector<int64_t> gd(Gs), gt(Gs), tok(cells), pre(kind == LDATM_GROUP_DOCUMENTS ? cells : 0);
  std::vector<uint64_t> shr(kind == LDATM_GROUP_MEAN ? cells : 0);
  groupTopics(doc_group, G, min_tokens, min_count, min_prop, gd.data(), gt.data(), tok.data(),
              pre.empty() ? nullptr : pre.data(), shr.empty() ? nullptr : shr.data());
  groupPrevalenceFinish(kind, G, K_, gd.data(), gt.data(), tok.data(), pre.empty() ? nullptr : pre.data(),
                        shr.empty() ? nullptr : shr.data(), out);
}

std::string ParallelTopicModel::groupTopicsText(const int32_t* doc_group, int32_t G, int32_t kind, int32_t n,
                                                int64_t min_tokens, int32_t min_count, double min_prop) {
  checkGroupKind(kind);
  if (G < 1) raise(LDA_ERR_INVALID_ARG, "G must be at least 1");
  if (n < 1) raise(LDA_ERR_INVALID_ARG, "n must be at least 1");
  checkCooccurrence(min_tokens, min_count, min_prop);
  std::vector<double> matrix((size_t)G * (size_t)K_);
  groupPrevalence(doc_group, G, kind, min_tokens, min_count, min_prop, matrix.data());
  std::vector<int32_t> ids((size_t)G * (size_t)n);
  std::vector<double> values((size_t)G * (size_t)n);
  groupTopTopicsSelect(G, K_, n, matrix.data(), ids.data(), values.data());
  return groupTopicsFormat(G, n, ids.data(), values.data());
}

void ParallelTopicModel::subCorpusTopWords(const uint8_t* doc_mask, int32_t n, int32_t* word_ids, int32_t* counts,
                                           int64_t* totals) {
  if (n < 1 || n > LDA_TOP_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_TOP_WORDS_MAX]");
  if (!word_ids || !counts || !totals) raise(LDA_ERR_INVALID_ARG, "null output");
  if (numDocs() > 0 && !doc_mask) raise(LDA_ERR_INVALID_ARG, "null doc_mask");
  ensureShards();
  // the tables live for this call only, whatever its end
  struct Release {
    std::vector<lda_ctx*>& ctx;
    ~Release() {
      for (auto c : ctx) (void)lda_subcorpus_release(c);
    }
  } release{shards_->ctx};
  const size_t S = shards_->ctx.size();
  for (size_t s = 0; s < S; ++s)
    check(lda_subcorpus_count(shards_->ctx[s], doc_mask ? doc_mask + shards_->doc_begin[s] : nullptr, 0),
          "lda_subcorpus_count");
  // the top n of a sum is not a merge of the shards' top n: add the tables, then select
  for (size_t s = 1; s < S; ++s) check(lda_subcorpus_merge(shards_->ctx[0], shards_->ctx[s]), "lda_subcorpus_merge");
  check(lda_subcorpus_top_words(shards_->ctx[0], n, word_ids, counts, totals), "lda_subcorpus_top_words");
}

namespace {
// Mallet's TopicModelDiagnostics thresholds (its DEFAULT_DOC_PROPORTIONS)
constexpr double DIAG_PROPS[LDATM_DIAG_PROPS] = {0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5};

// the sampler ABI's checks of K word lists, against the model's K and V
void checkWordLists(int32_t K, int32_t V, int32_t n, const int32_t* word_ids) {
  if (n < 1 || n > LDA_DIAG_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_DIAG_WORDS_MAX]");
  if (!word_ids) raise(LDA_ERR_INVALID_ARG, "null word_ids");
  for (int32_t k = 0; k < K; ++k) {
    const int32_t* l = word_ids + (size_t)k * n;
    for (int32_t i = 0; i < n; ++i) {
      if (l[i] < -1 || l[i] >= V) raise(LDA_ERR_INVALID_ARG, "word_ids: id outside [-1, V)");
      for (int32_t j = 0; l[i] >= 0 && j < i; ++j)
        if (l[j] == l[i]) raise(LDA_ERR_INVALID_ARG, "word_ids: the same id twice in one topic's list");
    }
  }
}
}  // namespace

void ParallelTopicModel::topicCodocuments(int32_t n, const int32_t* word_ids, int32_t P, const double* props,
                                          int64_t* codoc, int64_t* doc_stats) {
  // lda_topic_codocuments' checks, against the model's K and V, before any device work
  checkWordLists(K_, V_, n, word_ids);
  if (P < 0 || P > LDA_DIAG_PROPS_MAX) raise(LDA_ERR_INVALID_ARG, "P must be in [0, LDA_DIAG_PROPS_MAX]");
  if (P > 0 && !props) raise(LDA_ERR_INVALID_ARG, "null props");
  for (int32_t i = 0; i < P; ++i)
    if (!(props[i] > 0.0 && props[i] <= 1.0) || (i > 0 && !(props[i] > props[i - 1])))
      raise(LDA_ERR_INVALID_ARG, "props must be strictly ascending in (0, 1]");
  if (!codoc || !doc_stats) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  const size_t tri = (size_t)K_ * ((size_t)n * (n + 1) / 2), cells = (size_t)K_ * (size_t)(2 + P);
  std::fill(codoc, codoc + tri, 0);
  std::fill(doc_stats, doc_stats + cells, 0);
  std::vector<int32_t> part(tri);
  std::vector<int64_t> stats(cells);
  for (auto c : shards_->ctx) {
    check(lda_topic_codocuments(c, n, word_ids, P, props, part.data(), stats.data()), "lda_topic_codocuments");
    for (size_t i = 0; i < tri; ++i) codoc[i] += part[i];
    for (size_t i = 0; i < cells; ++i) doc_stats[i] += stats[i];
  }
}

void ParallelTopicModel::topicStatistics(int32_t n, int32_t* word_ids, int32_t* counts, int64_t* totals,
                                         double* share_sums, uint64_t* sumsq, int64_t* codoc, int64_t* doc_stats) {
  if (n < 1 || n > LDA_DIAG_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_DIAG_WORDS_MAX]");
  if (!word_ids) raise(LDA_ERR_INVALID_ARG, "null word_ids");
  if (!counts || !totals || !share_sums || !sumsq || !codoc || !doc_stats)
    raise(LDA_ERR_INVALID_ARG, "null output");
  topWords(n, word_ids, counts);
  check(lda_topic_word_stats(shards_->ctx[0], n, word_ids, counts, totals, share_sums, sumsq),
        "lda_topic_word_stats");
  topicCodocuments(n, word_ids, LDATM_DIAG_PROPS, DIAG_PROPS, codoc, doc_stats);
}

void diagnosticsFinish(int32_t K, int32_t V, int32_t n, double beta, const int32_t* nwsum, int32_t max_len,
                       const int64_t* topic_doc_counts, const int32_t* word_ids, const int32_t* counts,
                       const int64_t* totals, const double* share_sums, const uint64_t* sumsq, const int64_t* codoc,
                       const int64_t* doc_stats, double* out) {
  if (K < 1 || V < 1 || max_len < 0) raise(LDA_ERR_INVALID_ARG, "bad sizes");
  if (n < 1 || n > LDA_DIAG_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_DIAG_WORDS_MAX]");
  if (!nwsum) raise(LDA_ERR_INVALID_ARG, "null nwsum");
  if (!topic_doc_counts) raise(LDA_ERR_INVALID_ARG, "null topic_doc_counts");
  if (!word_ids) raise(LDA_ERR_INVALID_ARG, "null word_ids");
  if (!counts || !totals || !share_sums || !sumsq || !codoc || !doc_stats)
    raise(LDA_ERR_INVALID_ARG, "null statistics");
  if (!out) raise(LDA_ERR_INVALID_ARG, "null output");
  const size_t L1 = (size_t)max_len + 1, tri = (size_t)n * (n + 1) / 2;
  const int32_t S = 2 + LDATM_DIAG_PROPS;
  double N = 0.0;
  for (int32_t k = 0; k < K; ++k) N += (double)nwsum[k];
  auto ratio = [](double a, double b) { return b == 0.0 ? 0.0 : a / b; };
  auto xlog = [](double x, double arg) { return x == 0.0 ? 0.0 : x * std::log(arg); };
  for (int32_t k = 0; k < K; ++k) {
    const int64_t* H = topic_doc_counts + (size_t)k * L1;
    const int64_t* st = doc_stats + (size_t)k * S;
    const int64_t* C = codoc + (size_t)k * tri;
    int64_t docs = 0;
    for (size_t c = 1; c < L1; ++c) docs += H[c];
    if (docs != st[0])
      raise(LDA_ERR_INTERNAL, "diagnostics: the topic's document histogram does not add up to its document count");
    double* o = out + (size_t)k * LDATM_DIAG_COLUMNS;
    std::fill(o, o + LDATM_DIAG_COLUMNS, 0.0);
    if (nwsum[k] == 0) continue;
    const double T = (double)nwsum[k], Dk = (double)st[0];
    int32_t slot[LDA_DIAG_WORDS_MAX], m = 0;   // the non-empty slots, in list order
    for (int32_t i = 0; i < n; ++i)
      if (word_ids[(size_t)k * n + i] >= 0) slot[m++] = i;
    auto cnt = [&](int32_t i) { return (double)counts[(size_t)k * n + slot[i]]; };
    auto diag = [&](int32_t i) { return (double)C[(size_t)slot[i] * (slot[i] + 1) / 2 + slot[i]]; };
    o[LDATM_DIAG_TOKENS] = T;
    double hsum = 0.0;
    for (size_t c = 1; c < L1; ++c) hsum += (double)H[c] * ((double)c * std::log((double)c));
    o[LDATM_DIAG_DOCUMENT_ENTROPY] = std::log(T) - hsum / T;
    double coh = 0.0;
    for (int32_t i = 1; i < m; ++i)
      for (int32_t j = 0; j < i; ++j)
        coh += std::log(((double)C[(size_t)slot[i] * (slot[i] + 1) / 2 + slot[j]] + beta) / (diag(j) + beta));
    o[LDATM_DIAG_COHERENCE] = coh;
    double uni = 0.0, corp = 0.0, csum = 0.0, dsum = 0.0, excl = 0.0;
    for (int32_t i = 0; i < m; ++i) {
      const double p = cnt(i) / T;
      uni += xlog(p, p * (double)V);
      corp += xlog(p, p / ((double)totals[(size_t)k * n + slot[i]] / N));
      csum += cnt(i);
      dsum += diag(i);
      excl += ((beta + cnt(i)) / ((double)V * beta + T)) / share_sums[(size_t)k * n + slot[i]];
    }
    o[LDATM_DIAG_UNIFORM_DIST] = uni;
    o[LDATM_DIAG_CORPUS_DIST] = corp;
    o[LDATM_DIAG_EFF_NUM_WORDS] = ratio(T * T, (double)sumsq[k]);
    double js = 0.0;
    for (int32_t i = 0; i < m; ++i) {
      const double p = ratio(cnt(i), csum), q = ratio(diag(i), dsum), mu = (p + q) / 2.0;
      js += 0.5 * xlog(p, p / mu) + 0.5 * xlog(q, q / mu);
    }
    o[LDATM_DIAG_TOKEN_DOC_DIFF] = js;
    o[LDATM_DIAG_RANK_1_DOCS] = ratio((double)st[1], Dk);
    o[LDATM_DIAG_ALLOCATION_RATIO] = ratio((double)st[2 + 6], (double)st[2 + 1]);   // 0.5 over 0.02
    o[LDATM_DIAG_ALLOCATION_COUNT] = ratio((double)st[2 + 5], Dk);                  // 0.3
    o[LDATM_DIAG_EXCLUSIVITY] = m > 0 ? excl / (double)m : 0.0;
  }
}

void ParallelTopicModel::topicDiagnostics(int32_t n, double* out, int32_t* word_ids) {
  if (n < 1 || n > LDA_DIAG_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_DIAG_WORDS_MAX]");
  if (!out) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  const size_t cells = (size_t)K_ * (size_t)n, tri = (size_t)K_ * ((size_t)n * (n + 1) / 2);
  std::vector<int32_t> ids(cells), counts(cells), nwsum((size_t)K_);
  std::vector<int64_t> totals(cells), codoc(tri), stats((size_t)K_ * (2 + LDATM_DIAG_PROPS));
  std::vector<double> shares(cells);
  std::vector<uint64_t> sumsq((size_t)K_);
  topicStatistics(n, ids.data(), counts.data(), totals.data(), shares.data(), sumsq.data(), codoc.data(),
                  stats.data());
  this->counts(nullptr, nwsum.data());
  // the shards' topicDocCounts of the current z, summed
  const size_t L1 = (size_t)max_doc_len_ + 1;
  std::vector<int64_t> hist((size_t)K_ * L1, 0);
  std::vector<int32_t> len(L1), part((size_t)K_ * L1);
  for (auto c : shards_->ctx) {
    std::fill(len.begin(), len.end(), 0);
    std::fill(part.begin(), part.end(), 0);
    check(lda_doc_topic_histograms(c, max_doc_len_, len.data(), part.data()), "lda_doc_topic_histograms");
    for (size_t i = 0; i < part.size(); ++i) hist[i] += part[i];
  }
  diagnosticsFinish(K_, V_, n, beta_, nwsum.data(), max_doc_len_, hist.data(), ids.data(), counts.data(),
                    totals.data(), shares.data(), sumsq.data(), codoc.data(), stats.data(), out);
  if (word_ids) std::copy(ids.begin(), ids.end(), word_ids);
}

namespace {
// lda_word_cooccurrences' checks of the window and a host corpus, against the
// model's V, before any device work
void checkCooccurrenceCorpus(int32_t V, int32_t window, int64_t Dh, const int64_t* doc_off, const int32_t* words) {
  if (window < 0 || window > LDA_COOC_WINDOW_MAX)
    raise(LDA_ERR_INVALID_ARG, "window must be in [0, LDA_COOC_WINDOW_MAX]");
  if (!doc_off) return;
  if (Dh < 0) raise(LDA_ERR_INVALID_ARG, "bad sizes");
  for (int64_t d = 1; d <= Dh; ++d)
    if (doc_off[d] < doc_off[d - 1]) raise(LDA_ERR_INVALID_ARG, "doc_off not monotone");
  const int64_t N = doc_off[Dh] - doc_off[0];
  if (N > 0 && !words) raise(LDA_ERR_INVALID_ARG, "words is null");
  for (int64_t i = 0; i < N; ++i)
    if (words[i] < -1 || words[i] >= V) raise(LDA_ERR_INVALID_ARG, "word id out of range [-1, V)");
}
}  // namespace

void ParallelTopicModel::wordCooccurrences(int32_t n, const int32_t* word_ids, int32_t window, int64_t Dh,
                                           const int64_t* doc_off, const int32_t* words, int64_t* cooc,
                                           int64_t* units) {
  checkWordLists(K_, V_, n, word_ids);
  if (!cooc || !units) raise(LDA_ERR_INVALID_ARG, "null output");
  checkCooccurrenceCorpus(V_, window, Dh, doc_off, words);
  ensureShards();
  if (doc_off) {
    check(lda_word_cooccurrences(shards_->ctx[0], n, word_ids, window, Dh, doc_off, words, cooc, units),
          "lda_word_cooccurrences");
    return;
  }
  const size_t tri = (size_t)K_ * ((size_t)n * (n + 1) / 2);
  std::fill(cooc, cooc + tri, 0);
  *units = 0;
  std::vector<int64_t> part(tri);
  for (auto c : shards_->ctx) {
    int64_t u = 0;
    check(lda_word_cooccurrences(c, n, word_ids, window, 0, nullptr, nullptr, part.data(), &u),
          "lda_word_cooccurrences");
    for (size_t i = 0; i < tri; ++i) cooc[i] += part[i];
    *units += u;
  }
}

void coherenceFinish(int32_t K, int32_t n, int32_t measure, double epsilon, const int64_t* cooc, int64_t units,
                     double* sums, int64_t* pairs) {
  if (K < 1 || units < 0) raise(LDA_ERR_INVALID_ARG, "bad sizes");
  if (n < 1 || n > LDA_DIAG_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_DIAG_WORDS_MAX]");
  if (measure < LDATM_COHERENCE_UMASS || measure > LDATM_COHERENCE_NPMI)
    raise(LDA_ERR_INVALID_ARG, "measure must be LDATM_COHERENCE_UMASS, _UCI or _NPMI");
  if (!cooc) raise(LDA_ERR_INVALID_ARG, "null cooc");
  if (!sums || !pairs) raise(LDA_ERR_INVALID_ARG, "null output");
  const double eps = epsilon >= 0.0 ? epsilon : measure == LDATM_COHERENCE_UMASS ? 1.0 : 1e-12;
  const double N = (double)units;
  const size_t tri = (size_t)n * (n + 1) / 2;
  for (int32_t k = 0; k < K; ++k) {
    const int64_t* C = cooc + (size_t)k * tri;
    double sum = 0.0;
    int64_t kept = 0;
    for (int32_t i = 1; units > 0 && i < n; ++i) {
      const int64_t Di = C[(size_t)i * (i + 1) / 2 + i];
      if (Di == 0) continue;
      for (int32_t j = 0; j < i; ++j) {
        const int64_t Dj = C[(size_t)j * (j + 1) / 2 + j], Dij = C[(size_t)i * (i + 1) / 2 + j];
        if (Dj == 0) continue;
        if (measure == LDATM_COHERENCE_UMASS) {
          sum += std::log(((double)Dij + eps) / (double)Dj);
        } else {
          if (Dij == units) continue;
          const double p = (double)Dij / N + eps;
          const double uci = std::log(p / (((double)Di / N) * ((double)Dj / N)));
          sum += measure == LDATM_COHERENCE_UCI ? uci : uci / -std::log(p);
        }
        ++kept;
      }
    }
    sums[k] = sum;
    pairs[k] = kept;
  }
}

void ParallelTopicModel::topicCoherence(int32_t measure, int32_t n, int32_t window, double epsilon, int64_t Dh,
                                        const int64_t* doc_off, const int32_t* words, double* values, int64_t* pairs,
                                        int32_t* word_ids_out, int64_t* cooc_out, int64_t* units) {
  if (measure < LDATM_COHERENCE_UMASS || measure > LDATM_COHERENCE_NPMI)
    raise(LDA_ERR_INVALID_ARG, "measure must be LDATM_COHERENCE_UMASS, _UCI or _NPMI");
  if (n < 1 || n > LDA_DIAG_WORDS_MAX) raise(LDA_ERR_INVALID_ARG, "n must be in [1, LDA_DIAG_WORDS_MAX]");
  checkCooccurrenceCorpus(V_, window, Dh, doc_off, words);
  if (!values || !pairs || !units) raise(LDA_ERR_INVALID_ARG, "null output");
  ensureShards();
  const size_t cells = (size_t)K_ * (size_t)n, tri = (size_t)K_ * ((size_t)n * (n + 1) / 2);
  std::vector<int32_t> ids(cells), counts(cells);
  std::vector<int64_t> cooc(tri);
  topWords(n, ids.data(), counts.data());
  wordCooccurrences(n, ids.data(), window, Dh, doc_off, words, cooc.data(), units);
  coherenceFinish(K_, n, measure, epsilon, cooc.data(), *units, values, pairs);
  for (int32_t k = 0; k < K_; ++k) values[k] = pairs[k] > 0 ? values[k] / (double)pairs[k] : 0.0;
  if (word_ids_out) std::copy(ids.begin(), ids.end(), word_ids_out);
  if (cooc_out) std::copy(cooc.begin(), cooc.end(), cooc_out);
}

std::vector<double> ParallelTopicModel::getTopicProbabilities(int64_t doc) {
  if (doc < 0 || doc >= numDocs()) raise(LDA_ERR_INVALID_ARG, "document index out of range");
  // the document's counts from the device (no copy of z); the arithmetic,
  // the sequential sum included, is unchanged
  std::vector<int32_t> nd((size_t)K_);
  docCounts(1, &doc, nd.data());
  std::vector<double> dist((size_t)K_, 0.0);
  for (int k = 0; k < K_; ++k) dist[(size_t)k] = (double)nd[(size_t)k];
  double sum = 0.0;
  for (int k = 0; k < K_; ++k) {
    dist[(size_t)k] += alpha_[(size_t)k];
    sum += dist[(size_t)k];
  }
  for (int k = 0; k < K_; ++k) dist[(size_t)k] /= sum;
  return dist;
}

// IDSorter order: weight descending; equal weights by ascending id (Mallet's
// stable sort of an array already in id order; parity unpinned)
static void sort_ids(std::vector<std::pair<int32_t, double>>& v) {
  std::stable_sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.second > b.second; });
}

std::string ParallelTopicModel::documentTopics(double threshold, int32_t max) {
  ensureShards();
  if (max < 0 || max > K_) max = K_;
  const int64_t D = numDocs();
  std::string out = "#doc source topic proportion ...\n";
  auto head = [&](int64_t d) {
    out += std::to_string(d);
    out += ' ';
    out += has_source_[(size_t)d] ? sources_[(size_t)d] : std::string("null-source");
    out += ' ';
  };
  auto weight = [&](int k, int32_t cnt, int64_t len) {
    return (alpha_[(size_t)k] + cnt) / ((double)len + alpha_sum_);
  };
  // The device orders by the same expression with alphaSum = the sum of alpha
  // added in index order.  That is this model's order when alpha_sum_ holds
  // those bits (the constructor's alphaSum / K * K may not), or when alpha is
  // uniform: the numerators are then alpha + an integer, equal or at least 1
  // apart, and their order does not depend on the denominator's last bits.
  double seq_sum = 0.0;
  bool uniform = true;
  for (int k = 0; k < K_; ++k) {
    seq_sum += alpha_[(size_t)k];
    uniform = uniform && alpha_[(size_t)k] == alpha_[0];
  }
  const bool device_order = max >= 1 && max <= LDA_TOP_TOPICS_MAX && (uniform || seq_sum == alpha_sum_);
  if (device_order) {
    // the order from the device, a chunk of documents at a time; the weights
    // are recomputed here from the returned counts, so the text is the same
    const int64_t chunk = std::max<int64_t>(1, (int64_t(1) << 20) / max);
    std::vector<int32_t> top, cnt;
    std::vector<int64_t> ids;
    for (int64_t d0 = 0; d0 < D; d0 += chunk) {
      const int64_t m = std::min(chunk, D - d0);
      top.resize((size_t)(m * max));
      cnt.resize((size_t)(m * max));
      ids.resize((size_t)m);
      std::iota(ids.begin(), ids.end(), d0);
      docTopTopics(max, m, D == m ? nullptr : ids.data(), top.data(), cnt.data());
      for (int64_t d = d0; d < d0 + m; ++d) {
        head(d);
        const int64_t len = doc_off_[d + 1] - doc_off_[d];
        for (int i = 0; i < max; ++i) {
          const size_t at = (size_t)((d - d0) * max + i);
          const double w = weight(top[at], cnt[at], len);
          if (w < threshold) break;
          out += std::to_string(top[at]) + " " + java_double(w) + " ";
        }
        out += " \n";
      }
    }
    return out;
  }
  // every topic (or more than the device selects): the documents' count rows
  // from the device in bounded chunks, sorted here
  const int64_t chunk = std::max<int64_t>(1, (int64_t(1) << 22) / K_);
  std::vector<int32_t> nd;
  std::vector<int64_t> ids;
  std::vector<std::pair<int32_t, double>> sorted((size_t)K_);
  for (int64_t d0 = 0; d0 < D; d0 += chunk) {
    const int64_t m = std::min(chunk, D - d0);
    nd.resize((size_t)(m * K_));
    ids.resize((size_t)m);
    std::iota(ids.begin(), ids.end(), d0);
    docCounts(m, D == m ? nullptr : ids.data(), nd.data());
    for (int64_t d = d0; d < d0 + m; ++d) {
      head(d);
      const int64_t len = doc_off_[d + 1] - doc_off_[d];
      const int32_t* cnt = nd.data() + (size_t)((d - d0) * K_);
      for (int k = 0; k < K_; ++k) sorted[(size_t)k] = {k, weight(k, cnt[k], len)};
      sort_ids(sorted);
      for (int i = 0; i < max; ++i) {
        if (sorted[(size_t)i].second < threshold) break;
        out += std::to_string(sorted[(size_t)i].first) + " " + java_double(sorted[(size_t)i].second) + " ";
      }
      out += " \n";
    }
  }
  return out;
}

std::string ParallelTopicModel::displayTopWords(int32_t num_words, bool using_new_lines) {
  ensureShards();
  // Mallet prints numWords - 1 words: up to LDA_TOP_WORDS_MAX of them are
  // selected on the device (K x n ids and counts come back); more than that
  // take the whole table to the host as before
  const int32_t n_dev = num_words - 1;
  const bool device = n_dev >= 1 && n_dev <= LDA_TOP_WORDS_MAX;
  std::vector<int32_t> nw, top_ids, top_counts;
  if (device) {
    top_ids.resize((size_t)K_ * n_dev);
    top_counts.resize((size_t)K_ * n_dev);
    topWords(n_dev, top_ids.data(), top_counts.data());
  } else if (n_dev >= 1) {
    nw.resize((size_t)V_ * K_);
    check(lda_get_counts(shards_->ctx[0], nw.data(), nullptr, nullptr, nullptr), "lda_get_counts");
  }
  std::string out;
  std::vector<std::pair<int32_t, double>> words;
  for (int k = 0; k < K_; ++k) {
    words.clear();
    if (device) {
      for (int32_t i = 0; i < n_dev && top_ids[(size_t)k * n_dev + i] >= 0; ++i)
        words.emplace_back(top_ids[(size_t)k * n_dev + i], (double)top_counts[(size_t)k * n_dev + i]);
    } else if (n_dev >= 1) {
      for (int32_t w = 0; w < V_; ++w) {
        const int32_t c = nw[(size_t)w * K_ + k];
        if (c > 0) words.emplace_back(w, (double)c);
      }
      sort_ids(words);
    }
    auto name = [&](int32_t w) { return alphabet_.empty() ? std::to_string(w) : alphabet_[(size_t)w]; };
    // Mallet's loop starts its word counter at 1 and stops before numWords
    const size_t n = (size_t)std::max(0, std::min<int32_t>(num_words - 1, (int32_t)words.size()));
    if (using_new_lines) {
      out += std::to_string(k) + "\t" + java_number5(alpha_[(size_t)k]) + "\n";
      for (size_t i = 0; i < n; ++i)
        out += name(words[i].first) + "\t" + java_number5(words[i].second) + "\n";
    } else {
      out += std::to_string(k) + "\t" + java_number5(alpha_[(size_t)k]) + "\t";
      for (size_t i = 0; i < n; ++i) out += name(words[i].first) + " ";
      out += "\n";
    }
  }
  return out;
}

// ---- checkpoint: little-endian binary, every field needed to continue the
// run bit for bit (topics, hyperparameters, options and the Philox sweep
// counter).  The alpha statistics arrays are still written (format v2) but
// carry nothing across: estimate() clears them at its start and end, as
// Mallet 2.0.7's new WorkerRunnables drop theirs, so a resumed model starts
// its statistics empty whatever the file holds.
namespace {
// v4: without the alpha-statistics histograms (estimate() starts them
// empty, as Mallet's new WorkerRunnables do, so a file never needs them)
constexpr char kMagic[8] = {'L', 'D', 'A', 'T', 'M', 0, 'v', '4'};
constexpr char kMagicV3[8] = {'L', 'D', 'A', 'T', 'M', 0, 'v', '3'};  // v3: + staleness threads
constexpr char kMagicV2[8] = {'L', 'D', 'A', 'T', 'M', 0, 'v', '2'};  // v2: + warm start
constexpr char kMagicV1[8] = {'L', 'D', 'A', 'T', 'M', 0, 'v', '1'};

struct Writer {
  std::ofstream f;
  template <typename T>
  void pod(const T& v) { f.write(reinterpret_cast<const char*>(&v), sizeof(T)); }
  template <typename T>
  void vec(const std::vector<T>& v) {
    pod<int64_t>((int64_t)v.size());
    if (!v.empty()) f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  }
  void str(const std::string& s) {
    pod<int64_t>((int64_t)s.size());
    f.write(s.data(), (std::streamsize)s.size());
  }
};

struct Reader {
  std::ifstream f;
  template <typename T>
  T pod() {
    T v{};
    f.read(reinterpret_cast<char*>(&v), sizeof(T));
    if (!f) raise(LDA_ERR_INVALID_ARG, "checkpoint truncated");
    return v;
  }
  int64_t count(int64_t limit) {
    const int64_t n = pod<int64_t>();
    if (n < 0 || n > limit) raise(LDA_ERR_INVALID_ARG, "checkpoint corrupt (bad length)");
    return n;
  }
  template <typename T>
  std::vector<T> vec(int64_t limit) {
    std::vector<T> v((size_t)count(limit));
    if (!v.empty()) f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    if (!f) raise(LDA_ERR_INVALID_ARG, "checkpoint truncated");
    return v;
  }
  std::string str() {
    std::string s((size_t)count(1 << 30), '\0');
    f.read(&s[0], (std::streamsize)s.size());
    if (!f) raise(LDA_ERR_INVALID_ARG, "checkpoint truncated");
    return s;
  }
};
}  // namespace

void ParallelTopicModel::save(const std::string& path) {
  // live shards: their state; otherwise the snapshot (possibly no topics yet:
  // a model saved before its first use re-initialises them on load)
  const bool live = shards_ && !shards_dirty_;
  const std::vector<int32_t> z = live ? topics() : z_cache_;
  if (live) check(lda_get_sweep(shards_->ctx[0], &sweep_), "lda_get_sweep");
  Writer w{std::ofstream(path, std::ios::binary)};
  if (!w.f) raise(LDA_ERR_INVALID_ARG, "cannot open " + path);
  w.f.write(kMagic, 8);
  w.pod(K_);
  w.pod(V_);
  w.pod(alpha_sum_);
  w.pod(beta_);
  w.vec(alpha_);
  w.pod(seed_);
  w.pod(sweep_);
  for (int32_t v : {num_iterations_, optimize_interval_, burnin_period_, save_sample_interval_,
                    show_topics_interval_, words_per_topic_, (int32_t)symmetric_alpha_,
                    (int32_t)print_log_likelihood_, num_threads_, sampler_})
    w.pod(v);
  w.vec(doc_off_);
  w.vec(words_);
  w.vec(z);
  w.pod<int64_t>((int64_t)alphabet_.size());
  for (const auto& a : alphabet_) w.str(a);
  w.vec(has_source_);
  for (const auto& src : sources_) w.str(src);
  w.pod(max_doc_len_);
  w.pod(warm_parts_);
  w.pod(warm_sweeps_);
  w.pod(staleness_threads_);
  w.f.flush();
  if (!w.f) raise(LDA_ERR_INVALID_ARG, "write failed: " + path);
}

std::unique_ptr<ParallelTopicModel> ParallelTopicModel::load(const std::string& path) {
  Reader r{std::ifstream(path, std::ios::binary)};
  if (!r.f) raise(LDA_ERR_INVALID_ARG, "cannot open " + path);
  char magic[8];
  r.f.read(magic, 8);
  const bool v1 = r.f && std::memcmp(magic, kMagicV1, 8) == 0;
  const bool v2 = r.f && std::memcmp(magic, kMagicV2, 8) == 0;
  const bool v3 = r.f && std::memcmp(magic, kMagicV3, 8) == 0;
  if (!r.f || (!v1 && !v2 && !v3 && std::memcmp(magic, kMagic, 8) != 0))
    raise(LDA_ERR_INVALID_ARG, "not an lda_topic_model checkpoint");
  const int32_t K = r.pod<int32_t>(), V = r.pod<int32_t>();
  const double alpha_sum = r.pod<double>(), beta = r.pod<double>();
  auto m = std::make_unique<ParallelTopicModel>(K, alpha_sum, beta);
  m->V_ = V;
  m->alpha_ = r.vec<double>(K);
  if ((int32_t)m->alpha_.size() != K) raise(LDA_ERR_INVALID_ARG, "checkpoint corrupt (alpha)");
  m->seed_ = r.pod<uint64_t>();
  m->sweep_ = r.pod<uint32_t>();
  int32_t opt[10];
  for (int32_t& v : opt) v = r.pod<int32_t>();
  m->num_iterations_ = opt[0];
  m->optimize_interval_ = opt[1];
  m->burnin_period_ = opt[2];
  m->save_sample_interval_ = opt[3];
  m->show_topics_interval_ = opt[4];
  m->words_per_topic_ = opt[5];
  m->symmetric_alpha_ = opt[6] != 0;
  m->print_log_likelihood_ = opt[7] != 0;
  m->num_threads_ = opt[8];
  m->sampler_ = opt[9];
  const int64_t big = (int64_t)1 << 40;
  m->doc_off_ = r.vec<int64_t>(big);
  m->words_ = r.vec<int32_t>(big);
  m->z_cache_ = r.vec<int32_t>(big);
  const int64_t D = (int64_t)m->doc_off_.size() - 1;
  if (D < 0 || m->doc_off_[0] != 0 || m->doc_off_.back() != (int64_t)m->words_.size() ||
      (!m->z_cache_.empty() && m->z_cache_.size() != m->words_.size()))
    raise(LDA_ERR_INVALID_ARG, "checkpoint corrupt (documents)");
  for (int32_t wid : m->words_)
    if (wid < 0 || wid >= V) raise(LDA_ERR_INVALID_ARG, "checkpoint corrupt (word id)");
  for (int32_t t : m->z_cache_)
    if (t < 0 || t >= K) raise(LDA_ERR_INVALID_ARG, "checkpoint corrupt (topic)");
  const int64_t na = r.count(V);
  for (int64_t i = 0; i < na; ++i) m->alphabet_.push_back(r.str());
  m->has_source_ = r.vec<uint8_t>(D);
  for (int64_t d = 0; d < (int64_t)m->has_source_.size(); ++d) m->sources_.push_back(r.str());
  m->max_doc_len_ = r.pod<int32_t>();
  if (v1 || v2 || v3) {            // the histograms older files carry: read past them
    const std::vector<int32_t> dl = r.vec<int32_t>(big), td = r.vec<int32_t>(big);
    if (m->max_doc_len_ >= 0 &&
        (dl.size() != (size_t)m->max_doc_len_ + 1 || td.size() != (size_t)K * (m->max_doc_len_ + 1)))
      raise(LDA_ERR_INVALID_ARG, "checkpoint corrupt (statistics)");
  }
  if ((int64_t)m->has_source_.size() != D) raise(LDA_ERR_INVALID_ARG, "checkpoint corrupt (sources)");
  if (m->max_doc_len_ >= 0) {
    m->doc_len_counts_.assign((size_t)m->max_doc_len_ + 1, 0);
    m->topic_doc_counts_.assign((size_t)K * (m->max_doc_len_ + 1), 0);
  }
  if (!v1) {
    m->warm_parts_ = r.pod<int32_t>();
    m->warm_sweeps_ = r.pod<int32_t>();
  }
  // files before v3 continue with the snapshot sweeps they were made with
  m->staleness_threads_ = (v1 || v2) ? -1 : r.pod<int32_t>();
  m->shards_dirty_ = true;
  return m;
}

void ParallelTopicModel::infer(int64_t Dh, const int64_t* doc_off, const int32_t* words,
                               int32_t num_iterations, int32_t thinning, int32_t burn_in,
                               uint64_t seed, double* theta) {
  ensureShards();
  if (Dh < 0 || (Dh > 0 && (!doc_off || !theta))) raise(LDA_ERR_INVALID_ARG, "bad documents");
  // tokens of types unknown to the model are dropped (Mallet's inferencer
  // skips type indices beyond its typeTopicCounts); lda_infer also skips
  // known types without training tokens
  std::vector<int64_t> off((size_t)Dh + 1, 0);
  std::vector<int32_t> kept;
  for (int64_t d = 0; d < Dh; ++d) {
    for (int64_t i = doc_off[d] - doc_off[0]; i < doc_off[d + 1] - doc_off[0]; ++i)
      if (words[i] >= 0 && words[i] < V_) kept.push_back(words[i]);
    off[(size_t)d + 1] = (int64_t)kept.size();
  }
  check(lda_infer(shards_->ctx[0], Dh, off.data(), kept.empty() ? nullptr : kept.data(),
                  num_iterations, thinning, burn_in, seed, theta),
        "lda_infer");
}

void ParallelTopicModel::scoreTheta(int32_t metric, int64_t Q, const double* theta, int64_t M, const int64_t* docs,
                                    double* scores) {
  ensureShards();
  const int64_t D = numDocs();
  if (Q < 0 || M < 0) raise(LDA_ERR_INVALID_ARG, "bad sizes");
  if (M == 0) return;
  if (!docs && M != D) raise(LDA_ERR_INVALID_ARG, "without a document list M must be the number of documents");
  for (int64_t j = 0; docs && j < M; ++j)
    if (docs[j] < 0 || docs[j] >= D) raise(LDA_ERR_INVALID_ARG, "document id out of range [0, D)");
  if (Q == 0 || M == 0) return;
  if (!theta || !scores) raise(LDA_ERR_INVALID_ARG, "null argument");
  const std::vector<int64_t>& begin = shards_->doc_begin;
  const size_t G = shards_->ctx.size();
  std::vector<double> part;
  if (!docs) {
    for (size_t g = 0; g < G; ++g) {
      const int64_t d0 = begin[g], m = begin[g + 1] - d0;
      if (m == 0) continue;
      if (G == 1) {
        check(lda_score_docs(shards_->ctx[g], metric, Q, theta, 0, m, nullptr, scores), "lda_score_docs");
        return;
      }
      part.resize((size_t)Q * m);
      check(lda_score_docs(shards_->ctx[g], metric, Q, theta, 0, m, nullptr, part.data()), "lda_score_docs");
      for (int64_t q = 0; q < Q; ++q)
        std::copy(part.begin() + q * m, part.begin() + (q + 1) * m, scores + q * M + d0);
    }
    return;
  }
  // the list's documents by shard (shard-local ids), and where each goes in
  // the caller's order
  std::vector<std::vector<int64_t>> local(G), pos(G);
  for (int64_t j = 0; j < M; ++j) {
    const size_t g = (size_t)(std::upper_bound(begin.begin(), begin.end(), docs[j]) - begin.begin()) - 1;
    local[g].push_back(docs[j] - begin[g]);
    pos[g].push_back(j);
  }
  for (size_t g = 0; g < G; ++g) {
    const int64_t m = (int64_t)local[g].size();
    if (m == 0) continue;
    part.resize((size_t)Q * m);
    check(lda_score_docs(shards_->ctx[g], metric, Q, theta, 0, m, local[g].data(), part.data()), "lda_score_docs");
    for (int64_t q = 0; q < Q; ++q)
      for (int64_t i = 0; i < m; ++i) scores[q * M + pos[g][(size_t)i]] = part[(size_t)(q * m + i)];
  }
}

void ParallelTopicModel::scoreTop(int32_t metric, int64_t Q, const double* theta, int32_t n, int64_t* doc_ids,
                                  double* scores) {
  ensureShards();
  if (Q < 0 || n < 0) raise(LDA_ERR_INVALID_ARG, "bad sizes");
  if (metric != LDA_SCORE_COSINE && metric != LDA_SCORE_MSE)
    raise(LDA_ERR_INVALID_ARG, "metric must be LDA_SCORE_COSINE or LDA_SCORE_MSE");
  if (Q == 0 || n == 0) return;
  if (!theta || !doc_ids || !scores) raise(LDA_ERR_INVALID_ARG, "null argument");
  using Hit = std::pair<double, int64_t>;   // (score, global document id)
  const bool largest = metric == LDA_SCORE_COSINE;
  auto better = [largest](const Hit& a, const Hit& b) {
    if (a.first != b.first) return largest ? a.first > b.first : a.first < b.first;
    return a.second < b.second;
  };
  std::vector<std::vector<Hit>> best((size_t)Q);
  // chunks of at most 2^22 scores on the host, shard by shard
  const int64_t chunk = std::max<int64_t>(1, (int64_t(1) << 22) / Q);
  std::vector<double> part;
  for (size_t g = 0; g < shards_->ctx.size(); ++g) {
    const int64_t d0 = shards_->doc_begin[g], Dg = shards_->doc_begin[g + 1] - d0;
    for (int64_t j0 = 0; j0 < Dg; j0 += chunk) {
      const int64_t m = std::min(chunk, Dg - j0);
      part.resize((size_t)Q * m);
      check(lda_score_docs(shards_->ctx[g], metric, Q, theta, j0, m, nullptr, part.data()), "lda_score_docs");
      for (int64_t q = 0; q < Q; ++q) {
        std::vector<Hit>& b = best[(size_t)q];
        for (int64_t i = 0; i < m; ++i) b.emplace_back(part[(size_t)(q * m + i)], d0 + j0 + i);
        if ((int64_t)b.size() > n) {
          std::nth_element(b.begin(), b.begin() + n, b.end(), better);
          b.resize((size_t)n);
        }
      }
    }
  }
  for (int64_t q = 0; q < Q; ++q) {
    std::vector<Hit>& b = best[(size_t)q];
    std::sort(b.begin(), b.end(), better);
    for (int64_t i = 0; i < n; ++i) {
      const bool have = i < (int64_t)b.size();
      doc_ids[q * n + i] = have ? b[(size_t)i].second : -1;
      scores[q * n + i] = have ? b[(size_t)i].first : std::numeric_limits<double>::quiet_NaN();
    }
  }
}

double ParallelTopicModel::heldOutLogLik(int64_t Dh, const double* theta, const int64_t* doc_off,
                                         const int32_t* words, double* doc_ll) {
  ensureShards();
  double total = 0.0;
  check(lda_heldout_loglik(shards_->ctx[0], Dh, theta, doc_off, words, doc_ll, &total), "lda_heldout_loglik");
  return total;
}

void ParallelTopicModel::completionSplit(int32_t V, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                                         std::vector<int64_t>& obs_off, std::vector<int32_t>& obs,
                                         std::vector<int64_t>& sc_off, std::vector<int32_t>& sc) {
  obs_off.assign((size_t)Dh + 1, 0);
  sc_off.assign((size_t)Dh + 1, 0);
  obs.clear();
  sc.clear();
  std::vector<int32_t> kept;
  for (int64_t d = 0; d < Dh; ++d) {
    kept.clear();
    for (int64_t i = doc_off[d] - doc_off[0]; i < doc_off[d + 1] - doc_off[0]; ++i)
      if (words[i] >= 0 && words[i] < V) kept.push_back(words[i]);
    const size_t h = kept.size() / 2;
    obs.insert(obs.end(), kept.begin(), kept.begin() + (std::ptrdiff_t)h);
    sc.insert(sc.end(), kept.begin() + (std::ptrdiff_t)h, kept.end());
    obs_off[(size_t)d + 1] = (int64_t)obs.size();
    sc_off[(size_t)d + 1] = (int64_t)sc.size();
  }
}

double ParallelTopicModel::evaluate(int64_t Dh, const int64_t* doc_off, const int32_t* words,
                                    int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed,
                                    double* doc_ll, int64_t* tokens_scored, double* theta_out) {
  ensureShards();
  if (Dh < 0 || (Dh > 0 && (!doc_off || !doc_ll))) raise(LDA_ERR_INVALID_ARG, "bad documents");
  for (int64_t d = 1; d <= Dh; ++d)
    if (doc_off[d] < doc_off[d - 1]) raise(LDA_ERR_INVALID_ARG, "doc_off not monotone");
  if (Dh > 0 && doc_off[Dh] > doc_off[0] && !words) raise(LDA_ERR_INVALID_ARG, "words is null");
  std::vector<int64_t> obs_off, sc_off;
  std::vector<int32_t> obs, sc;
  completionSplit(V_, Dh, doc_off, words, obs_off, obs, sc_off, sc);
  if (tokens_scored) *tokens_scored = (int64_t)sc.size();
  double total = 0.0;
  check(lda_doc_completion(shards_->ctx[0], Dh, obs_off.data(), obs.empty() ? nullptr : obs.data(), sc_off.data(),
                           sc.empty() ? nullptr : sc.data(), num_iterations, thinning, burn_in, seed, doc_ll,
                           &total, theta_out),
        "lda_doc_completion");
  return total;
}

double ParallelTopicModel::leftToRight(int64_t Dh, const int64_t* doc_off, const int32_t* words,
                                       int32_t num_particles, int32_t resampling, uint64_t seed, double* doc_ll,
                                       int64_t* tokens_scored) {
  ensureShards();
  if (Dh < 0 || (Dh > 0 && (!doc_off || !doc_ll))) raise(LDA_ERR_INVALID_ARG, "bad documents");
  for (int64_t d = 1; d <= Dh; ++d)
    if (doc_off[d] < doc_off[d - 1]) raise(LDA_ERR_INVALID_ARG, "doc_off not monotone");
  if (Dh > 0 && doc_off[Dh] > doc_off[0] && !words) raise(LDA_ERR_INVALID_ARG, "words is null");
  std::vector<int64_t> off((size_t)Dh + 1, 0);
  std::vector<int32_t> kept;
  for (int64_t d = 0; d < Dh; ++d) {
    for (int64_t i = doc_off[d] - doc_off[0]; i < doc_off[d + 1] - doc_off[0]; ++i)
      if (words[i] >= 0 && words[i] < V_) kept.push_back(words[i]);
    off[(size_t)d + 1] = (int64_t)kept.size();
  }
  double total = 0.0;
  int64_t scored = 0;
  check(lda_left_to_right(shards_->ctx[0], Dh, off.data(), kept.empty() ? nullptr : kept.data(), num_particles,
                          resampling, seed, doc_ll, &total, &scored, nullptr, nullptr),
        "lda_left_to_right");
  if (tokens_scored) *tokens_scored = scored;
  return total;
}

void ParallelTopicModel::setHeldOut(int64_t Dh, const int64_t* doc_off, const int32_t* words, int32_t interval,
                                    int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed) {
  if (interval < 0 || Dh < 0 || num_iterations < 0 || burn_in < 0 || thinning < 1)
    raise(LDA_ERR_INVALID_ARG, "bad held-out settings");
  if (interval > 0 && Dh > 0 && !doc_off) raise(LDA_ERR_INVALID_ARG, "null doc_off");
  held_off_.assign(1, 0);
  held_words_.clear();
  held_interval_ = 0;
  if (interval == 0) return;
  for (int64_t d = 1; d <= Dh; ++d)
    if (doc_off[d] < doc_off[d - 1]) raise(LDA_ERR_INVALID_ARG, "doc_off not monotone");
  const int64_t n = Dh > 0 ? doc_off[Dh] - doc_off[0] : 0;
  if (n > 0 && !words) raise(LDA_ERR_INVALID_ARG, "words is null");
  held_off_.resize((size_t)Dh + 1);
  for (int64_t d = 0; d <= Dh && Dh > 0; ++d) held_off_[(size_t)d] = doc_off[d] - doc_off[0];
  held_words_.assign(words, words + n);
  held_interval_ = interval;
  held_iterations_ = num_iterations;
  held_thinning_ = thinning;
  held_burn_in_ = burn_in;
  held_seed_ = seed;
}

}  // namespace lda_host

// ------------------------------------------------------------------ C ABI
struct ldatm {
  std::unique_ptr<lda_host::ParallelTopicModel> owned;
  lda_host::ParallelTopicModel& model;
  ldatm(int32_t K, double a, double b)
      : owned(std::make_unique<lda_host::ParallelTopicModel>(K, a, b)), model(*owned) {}
  explicit ldatm(std::unique_ptr<lda_host::ParallelTopicModel> m) : owned(std::move(m)), model(*owned) {}
};

namespace {
thread_local std::string g_tm_error;

template <typename F>
lda_status guard(F&& f) {
  try {
    f();
    return LDA_OK;
  } catch (const lda_host::Error& e) {
    g_tm_error = e.message;
    return e.status;
  } catch (const std::bad_alloc&) {
    g_tm_error = "host allocation failed";
    return LDA_ERR_OUT_OF_MEMORY;
  } catch (const std::exception& e) {
    g_tm_error = e.what();
    return LDA_ERR_INVALID_ARG;
  } catch (...) {
    g_tm_error = "internal error: unknown exception";
    return LDA_ERR_INTERNAL;
  }
}

lda_status copy_text(const std::string& s, char* buf, size_t cap, size_t* len) {
  if (len) *len = s.size();
  if (buf) {
    if (cap < s.size() + 1) {
      g_tm_error = "buffer too small";
      return LDA_ERR_INVALID_ARG;
    }
    std::memcpy(buf, s.c_str(), s.size() + 1);
  }
  return LDA_OK;
}

lda_status write_file(const char* path, const std::string& s) {
  if (!path) {
    g_tm_error = "null path";
    return LDA_ERR_INVALID_ARG;
  }
  bool ok = false;
  const lda_status st = guard([&] {
    std::ofstream f(path, std::ios::binary);
    if (!f) throw lda_host::Error{LDA_ERR_INVALID_ARG, std::string("cannot open ") + path};
    f << s;
    ok = f.good();
  });
  if (st) return st;
  if (!ok) g_tm_error = std::string("write failed: ") + path;
  return ok ? LDA_OK : LDA_ERR_INVALID_ARG;
}

#define TM_CHECK(m)                 \
  if (!(m)) {                       \
    g_tm_error = "null model";      \
    return LDA_ERR_INVALID_ARG;     \
  }
}  // namespace

extern "C" {

const char* ldatm_last_error(void) { return g_tm_error.c_str(); }

lda_status ldatm_format_double(double x, int32_t style, char* buf, size_t cap) {
  if (style != 0 && style != 1) {
    g_tm_error = "style must be 0 or 1";
    return LDA_ERR_INVALID_ARG;
  }
  std::string t;
  const lda_status st = guard([&] { t = style == 0 ? lda_host::java_double(x) : lda_host::java_number5(x); });
  return st ? st : copy_text(t, buf, cap, nullptr);
}

lda_status ldatm_create(ldatm** out, int32_t num_topics, double alpha_sum, double beta) {
  if (!out) return LDA_ERR_INVALID_ARG;
  *out = nullptr;
  return guard([&] { *out = new ldatm(num_topics, alpha_sum, beta); });
}

void ldatm_destroy(ldatm* m) { delete m; }

lda_status ldatm_set_alphabet(ldatm* m, int32_t num_types, const char* const* words) {
  TM_CHECK(m);
  return guard([&] {
    std::vector<std::string> w;
    if (words)
      for (int32_t i = 0; i < num_types; ++i) w.emplace_back(words[i] ? words[i] : "");
    m->model.setAlphabet(std::move(w), num_types);
  });
}

lda_status ldatm_add_instances(ldatm* m, int64_t D, const int64_t* doc_off, const int32_t* words,
                               const char* const* sources) {
  TM_CHECK(m);
  return guard([&] { m->model.addInstances(D, doc_off, words, sources); });
}

#define TM_SETTER(name, call)                          \
  lda_status name(ldatm* m, int32_t n) {               \
    TM_CHECK(m);                                       \
    return guard([&] { m->model.call; });              \
  }
TM_SETTER(ldatm_set_num_iterations, setNumIterations(n))
TM_SETTER(ldatm_set_optimize_interval, setOptimizeInterval(n))
TM_SETTER(ldatm_set_burnin_period, setBurninPeriod(n))
TM_SETTER(ldatm_set_symmetric_alpha, setSymmetricAlpha(n != 0))
TM_SETTER(ldatm_set_num_threads, setNumThreads(n))
TM_SETTER(ldatm_set_sampler, setSampler(n))
TM_SETTER(ldatm_set_exchange_parts, setExchangeParts(n))

lda_status ldatm_set_warm_start(ldatm* m, int32_t parts, int32_t sweeps) {
  TM_CHECK(m);
  return guard([&] { m->model.setWarmStart(parts, sweeps); });
}

lda_status ldatm_set_staleness_threads(ldatm* m, int32_t threads) {
  TM_CHECK(m);
  return guard([&] { m->model.setStalenessThreads(threads); });
}

lda_status ldatm_set_devices(ldatm* m, int32_t n, const int32_t* devices) {
  TM_CHECK(m);
  return guard([&] { m->model.setDevices(devices, n); });
}

lda_status ldatm_num_shards(ldatm* m, int32_t* shards) {
  TM_CHECK(m && shards);
  return guard([&] { *shards = m->model.numShards(); });
}

lda_status ldatm_exchange_info(ldatm* m, int32_t* cells_per_word, int32_t* used_lists, int32_t* escapes_max,
                               int64_t* list_exchanges) {
  TM_CHECK(m);
  return guard([&] { m->model.exchangeInfo(cells_per_word, used_lists, escapes_max, list_exchanges); });
}

int32_t ldatm_plan_shards(int32_t num_threads, int32_t num_devices, int64_t num_tokens,
                          int32_t num_types, int32_t num_topics, int64_t num_docs) {
  return lda_host::plan_shards(num_threads, num_devices, num_tokens, num_types, num_topics, num_docs);
}
TM_SETTER(ldatm_set_verbosity, setVerbosity(n))
TM_SETTER(ldatm_set_print_log_likelihood, setPrintLogLikelihood(n != 0))

lda_status ldatm_set_save_sample_interval(ldatm* m, int32_t n) {
  TM_CHECK(m);
  if (n < 1) {
    g_tm_error = "saveSampleInterval must be >= 1";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] { m->model.setSaveSampleInterval(n); });
}

lda_status ldatm_set_topic_display(ldatm* m, int32_t interval, int32_t n) {
  TM_CHECK(m);
  return guard([&] { m->model.setTopicDisplay(interval, n); });
}

lda_status ldatm_set_random_seed(ldatm* m, int64_t seed) {
  TM_CHECK(m);
  return guard([&] { m->model.setRandomSeed(seed); });
}

lda_status ldatm_set_topics(ldatm* m, int64_t n, const int32_t* z) {
  TM_CHECK(m);
  TM_CHECK(z || n == 0);
  return guard([&] { m->model.setTopics(z, n); });
}

lda_status ldatm_set_hyper(ldatm* m, const double* alpha, double alpha_sum, double beta) {
  TM_CHECK(m && alpha);
  return guard([&] { m->model.setHyper(alpha, alpha_sum, beta); });
}

lda_status ldatm_get_sweep(ldatm* m, uint32_t* sweep) {
  TM_CHECK(m && sweep);
  return guard([&] { *sweep = m->model.sweep(); });
}

lda_status ldatm_set_sweep(ldatm* m, uint32_t sweep) {
  TM_CHECK(m);
  return guard([&] { m->model.setSweep(sweep); });
}

lda_status ldatm_estimate(ldatm* m) {
  TM_CHECK(m);
  return guard([&] { m->model.estimate(); });
}

lda_status ldatm_get_ll_trace(ldatm* m, int32_t* iterations, double* ll, int32_t cap, int32_t* n) {
  TM_CHECK(m);
  const auto& t = m->model.llTrace();
  if (n) *n = (int32_t)t.size();
  for (int32_t i = 0; i < cap && i < (int32_t)t.size(); ++i) {
    if (iterations) iterations[i] = t[(size_t)i].first;
    if (ll) ll[i] = t[(size_t)i].second;
  }
  return LDA_OK;
}

lda_status ldatm_set_held_out(ldatm* m, int64_t Dh, const int64_t* doc_off, const int32_t* words, int32_t interval,
                              int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed) {
  TM_CHECK(m);
  return guard([&] { m->model.setHeldOut(Dh, doc_off, words, interval, num_iterations, thinning, burn_in, seed); });
}

lda_status ldatm_get_held_out_trace(ldatm* m, int32_t* iterations, double* ll, int32_t cap, int32_t* n) {
  TM_CHECK(m);
  const auto& t = m->model.heldOutTrace();
  if (n) *n = (int32_t)t.size();
  for (int32_t i = 0; i < cap && i < (int32_t)t.size(); ++i) {
    if (iterations) iterations[i] = t[(size_t)i].first;
    if (ll) ll[i] = t[(size_t)i].second;
  }
  return LDA_OK;
}

lda_status ldatm_model_log_likelihood(ldatm* m, double* out) {
  TM_CHECK(m);
  return guard([&] { *out = m->model.modelLogLikelihood(); });
}

lda_status ldatm_get_shape(ldatm* m, int32_t* K, int32_t* V, int64_t* D, int64_t* N) {
  TM_CHECK(m);
  if (K) *K = m->model.numTopics();
  if (V) *V = m->model.numTypes();
  if (D) *D = m->model.numDocs();
  if (N) *N = m->model.numTokens();
  return LDA_OK;
}

lda_status ldatm_get_hyper(ldatm* m, double* alpha, double* alpha_sum, double* beta) {
  TM_CHECK(m);
  if (alpha) std::copy(m->model.alpha().begin(), m->model.alpha().end(), alpha);
  if (alpha_sum) *alpha_sum = m->model.alphaSum();
  if (beta) *beta = m->model.beta();
  return LDA_OK;
}

lda_status ldatm_get_z(ldatm* m, int32_t* z) {
  TM_CHECK(m);
  return guard([&] {
    const std::vector<int32_t> t = m->model.topics();
    if ((int64_t)t.size() != m->model.numTokens()) throw lda_host::Error{LDA_ERR_STATE, "no topic assignments yet"};
    std::copy(t.begin(), t.end(), z);
  });
}

lda_status ldatm_get_counts(ldatm* m, int32_t* nw, int32_t* nwsum) {
  TM_CHECK(m);
  return guard([&] { m->model.counts(nw, nwsum); });
}

lda_status ldatm_get_topic_probabilities(ldatm* m, int64_t doc, double* out) {
  TM_CHECK(m);
  return guard([&] {
    const std::vector<double> p = m->model.getTopicProbabilities(doc);
    std::copy(p.begin(), p.end(), out);
  });
}

lda_status ldatm_top_words(ldatm* m, int32_t n, int32_t* word_ids, int32_t* counts) {
  TM_CHECK(m);
  return guard([&] { m->model.topWords(n, word_ids, counts); });
}

lda_status ldatm_topic_distances(ldatm* m, ldatm* other, int32_t metric, double* out) {
  TM_CHECK(m);
  return guard([&] { m->model.topicDistances(other ? &other->model : nullptr, metric, out); });
}

lda_status ldatm_nearest_topics(ldatm* m, ldatm* other, int32_t metric, int32_t n, int32_t* topics,
                                double* values) {
  TM_CHECK(m);
  return guard([&] { m->model.nearestTopics(other ? &other->model : nullptr, metric, n, topics, values); });
}

lda_status ldatm_doc_top_topics(ldatm* m, int32_t mtop, int64_t M, const int64_t* docs, int32_t* topics,
                                int32_t* counts) {
  TM_CHECK(m);
  return guard([&] { m->model.docTopTopics(mtop, M, docs, topics, counts); });
}

lda_status ldatm_doc_counts(ldatm* m, int64_t M, const int64_t* docs, int32_t* nd) {
  TM_CHECK(m);
  return guard([&] { m->model.docCounts(M, docs, nd); });
}

lda_status ldatm_topic_codocuments(ldatm* m, int32_t n, const int32_t* word_ids, int32_t P, const double* props,
                                   int64_t* codoc, int64_t* doc_stats) {
  TM_CHECK(m);
  return guard([&] { m->model.topicCodocuments(n, word_ids, P, props, codoc, doc_stats); });
}

lda_status ldatm_topic_statistics(ldatm* m, int32_t n, int32_t* word_ids, int32_t* counts, int64_t* totals,
                                  double* share_sums, uint64_t* sumsq, int64_t* codoc, int64_t* doc_stats) {
  TM_CHECK(m);
  return guard([&] { m->model.topicStatistics(n, word_ids, counts, totals, share_sums, sumsq, codoc, doc_stats); });
}

lda_status ldatm_diagnostics_finish(int32_t K, int32_t V, int32_t n, double beta, const int32_t* nwsum,
                                    int32_t max_len, const int64_t* topic_doc_counts, const int32_t* word_ids,
                                    const int32_t* counts, const int64_t* totals, const double* share_sums,
                                    const uint64_t* sumsq, const int64_t* codoc, const int64_t* doc_stats,
                                    double* out) {
  return guard([&] {
    lda_host::diagnosticsFinish(K, V, n, beta, nwsum, max_len, topic_doc_counts, word_ids, counts, totals,
                                share_sums, sumsq, codoc, doc_stats, out);
  });
}

lda_status ldatm_topic_diagnostics(ldatm* m, int32_t n, double* out, int32_t* word_ids) {
  TM_CHECK(m);
  return guard([&] { m->model.topicDiagnostics(n, out, word_ids); });
}

lda_status ldatm_word_cooccurrences(ldatm* m, int32_t n, const int32_t* word_ids, int32_t window, int64_t Dh,
                                    const int64_t* doc_off, const int32_t* words, int64_t* cooc, int64_t* units) {
  TM_CHECK(m);
  return guard([&] { m->model.wordCooccurrences(n, word_ids, window, Dh, doc_off, words, cooc, units); });
}

lda_status ldatm_coherence_finish(int32_t K, int32_t n, int32_t measure, double epsilon, const int64_t* cooc,
                                  int64_t units, double* sums, int64_t* pairs) {
  return guard([&] { lda_host::coherenceFinish(K, n, measure, epsilon, cooc, units, sums, pairs); });
}

lda_status ldatm_topic_coherence(ldatm* m, int32_t measure, int32_t n, int32_t window, double epsilon, int64_t Dh,
                                 const int64_t* doc_off, const int32_t* words, double* values, int64_t* pairs,
                                 int32_t* word_ids_out, int64_t* cooc_out, int64_t* units) {
  TM_CHECK(m);
  return guard([&] {
    m->model.topicCoherence(measure, n, window, epsilon, Dh, doc_off, words, values, pairs, word_ids_out, cooc_out,
                            units);
  });
}

lda_status ldatm_document_topics_text(ldatm* m, double threshold, int32_t max, char* buf, size_t cap,
                                      size_t* len) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.documentTopics(threshold, max); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_print_document_topics(ldatm* m, const char* path, double threshold, int32_t max) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.documentTopics(threshold, max); });
  return st ? st : write_file(path, s);
}

lda_status ldatm_top_words_text(ldatm* m, int32_t num_words, int32_t using_new_lines, char* buf,
                                size_t cap, size_t* len) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.displayTopWords(num_words, using_new_lines != 0); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_print_top_words(ldatm* m, const char* path, int32_t num_words, int32_t using_new_lines) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.displayTopWords(num_words, using_new_lines != 0); });
  return st ? st : write_file(path, s);
}

lda_status ldatm_topic_top_docs(ldatm* m, int32_t n, double smoothing, int32_t min_tokens, int64_t* doc_ids,
                                int32_t* counts, int32_t* lengths) {
  TM_CHECK(m);
  return guard([&] { m->model.topicTopDocs(n, smoothing, min_tokens, doc_ids, counts, lengths); });
}

lda_status ldatm_topic_documents_text(ldatm* m, int32_t max, double smoothing, int32_t min_tokens, char* buf,
                                      size_t cap, size_t* len) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.topicDocuments(max, smoothing, min_tokens); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_print_topic_documents(ldatm* m, const char* path, int32_t max, double smoothing,
                                       int32_t min_tokens) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.topicDocuments(max, smoothing, min_tokens); });
  return st ? st : write_file(path, s);
}

lda_status ldatm_topic_documents_format(int32_t K, int32_t n, double smoothing, const int64_t* doc_ids,
                                        const int32_t* counts, const int32_t* lengths, const char* const* names,
                                        int64_t num_names, char* buf, size_t cap, size_t* len) {
  if (K < 1 || n < 1 || !(smoothing >= 0.0) || !std::isfinite(smoothing) || !doc_ids || !counts || !lengths ||
      num_names < 0 || (num_names > 0 && !names)) {
    g_tm_error = "bad argument";
    return LDA_ERR_INVALID_ARG;
  }
  std::string s;
  lda_status st = guard([&] {
    s = lda_host::topicDocumentsFormat(K, n, smoothing, doc_ids, counts, lengths, [&](int64_t d) {
      return d < num_names && names[d] ? std::string(names[d]) : std::string("null-source");
    });
  });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_document_distances(ldatm* m, int32_t metric, int64_t Q, const double* theta, const int32_t* counts,
                                    int64_t M, const int64_t* docs, double* out) {
  TM_CHECK(m);
  return guard([&] { m->model.documentDistances(metric, Q, theta, counts, M, docs, out); });
}

lda_status ldatm_nearest_documents(ldatm* m, int32_t metric, int32_t n, int64_t Q, const double* theta,
                                   const int32_t* counts, const int64_t* skip, int32_t min_tokens, int64_t* doc_ids,
                                   double* values) {
  TM_CHECK(m);
  return guard([&] { m->model.nearestDocuments(metric, n, Q, theta, counts, skip, min_tokens, doc_ids, values); });
}

lda_status ldatm_document_neighbors(ldatm* m, int32_t metric, int32_t n, int64_t M, const int64_t* docs,
                                    int32_t min_tokens, int64_t* doc_ids, double* values) {
  TM_CHECK(m);
  return guard([&] { m->model.documentNeighbors(metric, n, M, docs, min_tokens, doc_ids, values); });
}

lda_status ldatm_document_neighbors_text(ldatm* m, int32_t n, int32_t metric, int32_t min_tokens, char* buf,
                                         size_t cap, size_t* len) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.documentNeighborsText(n, metric, min_tokens); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_print_document_neighbors(ldatm* m, const char* path, int32_t n, int32_t metric,
                                          int32_t min_tokens) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.documentNeighborsText(n, metric, min_tokens); });
  return st ? st : write_file(path, s);
}

lda_status ldatm_document_neighbors_format(int64_t M, int32_t n, const int64_t* docs, const int64_t* doc_ids,
                                           const double* values, const char* const* names, int64_t num_names,
                                           char* buf, size_t cap, size_t* len) {
  if (M < 0 || n < 1 || (M > 0 && (!doc_ids || !values)) || num_names < 0 || (num_names > 0 && !names)) {
    g_tm_error = "bad argument";
    return LDA_ERR_INVALID_ARG;
  }
  std::string s;
  lda_status st = guard([&] {
    s = lda_host::documentNeighborsFormat(M, n, docs, doc_ids, values, [&](int64_t d) {
      return d < num_names && names[d] ? std::string(names[d]) : std::string("null-source");
    });
  });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_relevant_words(ldatm* m, int32_t n, int32_t L, const double* lambdas, int32_t* word_ids,
                                int32_t* counts, int64_t* totals, double* logprob, double* loglift) {
  TM_CHECK(m);
  return guard([&] { m->model.relevantWords(n, L, lambdas, word_ids, counts, totals, logprob, loglift); });
}

lda_status ldatm_salient_words(ldatm* m, int32_t n, int32_t* word_ids, int64_t* totals, double* saliency,
                               double* distinctiveness) {
  TM_CHECK(m);
  return guard([&] { m->model.salientWords(n, word_ids, totals, saliency, distinctiveness); });
}

lda_status ldatm_word_rows(ldatm* m, int64_t M, const int32_t* word_ids, int32_t* rows, int64_t* totals) {
  TM_CHECK(m);
  return guard([&] { m->model.wordRows(M, word_ids, rows, totals); });
}

lda_status ldatm_relevant_words_text(ldatm* m, int32_t n, double lambda, char* buf, size_t cap, size_t* len) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.relevantWordsText(n, lambda); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_print_relevant_words(ldatm* m, const char* path, int32_t n, double lambda) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.relevantWordsText(n, lambda); });
  return st ? st : write_file(path, s);
}

lda_status ldatm_relevant_words_format(int32_t K, int32_t n, double lambda, const int32_t* word_ids,
                                       const int32_t* counts, const int64_t* totals, const double* logprob,
                                       const double* loglift, const char* const* names, int64_t num_names, char* buf,
                                       size_t cap, size_t* len) {
  if (K < 1 || n < 1 || !std::isfinite(lambda) || !(lambda >= 0.0) || !(lambda <= 1.0) || !word_ids || !counts ||
      !totals || !logprob || !loglift || num_names < 0 || (num_names > 0 && !names)) {
    g_tm_error = "bad argument";
    return LDA_ERR_INVALID_ARG;
  }
  std::string s;
  lda_status st = guard([&] {
    s = lda_host::relevantWordsFormat(K, n, lambda, word_ids, counts, totals, logprob, loglift, [&](int32_t w) {
      return w >= 0 && w < num_names && names[w] ? std::string(names[w]) : std::to_string(w);
    });
  });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_topic_phrases(ldatm* m, int32_t n, int32_t min_len, int32_t max_len, int32_t min_count,
                               int32_t* phrase_words, int32_t* lengths, int64_t* counts, int64_t* first,
                               int64_t* topic_runs, int64_t* topic_distinct, int64_t* skipped_long, int32_t* proven) {
  TM_CHECK(m);
  return guard([&] {
    m->model.topicPhrases(n, min_len, max_len, min_count, phrase_words, lengths, counts, first, topic_runs,
                          topic_distinct, skipped_long, proven);
  });
}

lda_status ldatm_topic_phrases_text(ldatm* m, int32_t n, int32_t min_len, int32_t max_len, int32_t min_count,
                                    char* buf, size_t cap, size_t* len) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.topicPhrasesText(n, min_len, max_len, min_count); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_print_topic_phrases(ldatm* m, const char* path, int32_t n, int32_t min_len, int32_t max_len,
                                     int32_t min_count) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.topicPhrasesText(n, min_len, max_len, min_count); });
  return st ? st : write_file(path, s);
}

lda_status ldatm_topic_phrases_format(int32_t K, int32_t n, int32_t max_len, const int32_t* phrase_words,
                                      const int32_t* lengths, const int64_t* counts, const char* const* names,
                                      int64_t num_names, char* buf, size_t cap, size_t* len) {
  if (K < 1 || n < 1 || max_len < 1 || !phrase_words || !lengths || !counts || num_names < 0 ||
      (num_names > 0 && !names)) {
    g_tm_error = "bad argument";
    return LDA_ERR_INVALID_ARG;
  }
  std::string s;
  lda_status st = guard([&] {
    s = lda_host::topicPhrasesFormat(K, n, max_len, phrase_words, lengths, counts, [&](int32_t w) {
      return w >= 0 && w < num_names && names[w] ? std::string(names[w]) : std::to_string(w);
    });
  });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_topic_phrases_bound(int32_t K, int32_t n, int32_t shards, const int64_t* shard_counts,
                                     const int64_t* totals, int64_t* bound, int32_t* proven) {
  if (K < 1 || n < 1 || n > LDA_PHRASES_MAX || shards < 1 || !shard_counts || !totals || !bound || !proven) {
    g_tm_error = "bad argument";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] { lda_host::topicPhrasesBound(K, n, shards, shard_counts, totals, bound, proven); });
}

lda_status ldatm_topic_cooccurrence(ldatm* m, int64_t min_tokens, int32_t min_count, double min_prop,
                                    int64_t* docs_used, int64_t* tokens, int64_t* present, int64_t* codocs,
                                    int64_t* overlap, int64_t* product) {
  TM_CHECK(m);
  return guard([&] {
    m->model.topicCooccurrence(min_tokens, min_count, min_prop, docs_used, tokens, present, codocs, overlap, product);
  });
}

lda_status ldatm_topic_correlation_finish(int32_t measure, int32_t K, int64_t docs_used, const int64_t* tokens,
                                          const int64_t* present, int32_t table_kind, const int64_t* table,
                                          double* out) {
  return guard([&] {
    lda_host::topicCorrelationFinish(measure, K, docs_used, tokens, present, table_kind, table, out);
  });
}

lda_status ldatm_topic_correlations(ldatm* m, int32_t measure, int64_t min_tokens, int32_t min_count,
                                    double min_prop, double* out) {
  TM_CHECK(m);
  return guard([&] { m->model.topicCorrelations(measure, min_tokens, min_count, min_prop, out); });
}

lda_status ldatm_topic_partners(ldatm* m, int32_t measure, int64_t min_tokens, int32_t min_count, double min_prop,
                                int32_t n, int32_t* ids, double* values) {
  TM_CHECK(m);
  return guard([&] { m->model.topicPartners(measure, min_tokens, min_count, min_prop, n, ids, values); });
}

lda_status ldatm_topic_partners_select(int32_t K, int32_t n, const double* matrix, int32_t* ids, double* values) {
  return guard([&] { lda_host::topicPartnersSelect(K, n, matrix, ids, values); });
}

lda_status ldatm_topic_correlations_text(ldatm* m, int32_t measure, int32_t n, int64_t min_tokens,
                                         int32_t min_count, double min_prop, char* buf, size_t cap, size_t* len) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.topicCorrelationsText(measure, n, min_tokens, min_count, min_prop); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_print_topic_correlations(ldatm* m, const char* path, int32_t measure, int32_t n,
                                          int64_t min_tokens, int32_t min_count, double min_prop) {
  TM_CHECK(m);
  std::string s;
  lda_status st = guard([&] { s = m->model.topicCorrelationsText(measure, n, min_tokens, min_count, min_prop); });
  return st ? st : write_file(path, s);
}

lda_status ldatm_topic_correlations_format(int32_t K, int32_t n, const int32_t* ids, const double* values,
                                           char* buf, size_t cap, size_t* len) {
  if (K < 1 || n < 1 || !ids || !values) {
    g_tm_error = "bad argument";
    return LDA_ERR_INVALID_ARG;
  }
  std::string s;
  lda_status st = guard([&] { s = lda_host::topicCorrelationsFormat(K, n, ids, values); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_group_topics(ldatm* m, const int32_t* doc_group, int32_t G, int64_t min_tokens, int32_t min_count,
                              double min_prop, int64_t* group_docs, int64_t* group_tokens, int64_t* tokens,
                              int64_t* present, uint64_t* shares) {
  TM_CHECK(m);
  return guard([&] {
    m->model.groupTopics(doc_group, G, min_tokens, min_count, min_prop, group_docs, group_tokens, tokens, present,
                         shares);
  });
}

lda_status ldatm_group_prevalence_finish(int32_t kind, int32_t G, int32_t K, const int64_t* group_docs,
                                         const int64_t* group_tokens, const int64_t* tokens, const int64_t* present,
                                         const uint64_t* shares, double* out) {
  return guard([&] {
    lda_host::groupPrevalenceFinish(kind, G, K, group_docs, group_tokens, tokens, present, shares, out);
  });
}

lda_status ldatm_group_prevalence(ldatm* m, const int32_t* doc_group, int32_t G, int32_t kind, int64_t min_tokens,
                                  int32_t min_count, double min_prop, double* out) {
  TM_CHECK(m);
  return guard([&] { m->model.groupPrevalence(doc_group, G, kind, min_tokens, min_count, min_prop, out); });
}

lda_status ldatm_group_top_topics_select(int32_t G, int32_t K, int32_t n, const double* matrix, int32_t* ids,
                                         double* values) {
  return guard([&] { lda_host::groupTopTopicsSelect(G, K, n, matrix, ids, values); });
}

lda_status ldatm_group_topics_text(ldatm* m, const int32_t* doc_group, int32_t G, int32_t kind, int32_t n,
                                   int64_t min_tokens, int32_t min_count, double min_prop, char* buf, size_t cap,
                                   size_t* len) {
  TM_CHECK(m);
  std::string s;
  lda_status st =
      guard([&] { s = m->model.groupTopicsText(doc_group, G, kind, n, min_tokens, min_count, min_prop); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_print_group_topics(ldatm* m, const char* path, const int32_t* doc_group, int32_t G, int32_t kind,
                                    int32_t n, int64_t min_tokens, int32_t min_count, double min_prop) {
  TM_CHECK(m);
  std::string s;
  lda_status st =
      guard([&] { s = m->model.groupTopicsText(doc_group, G, kind, n, min_tokens, min_count, min_prop); });
  return st ? st : write_file(path, s);
}

lda_status ldatm_group_topics_format(int32_t G, int32_t n, const int32_t* ids, const double* values, char* buf,
                                     size_t cap, size_t* len) {
  if (G < 1 || n < 1 || !ids || !values) {
    g_tm_error = "bad argument";
    return LDA_ERR_INVALID_ARG;
  }
  std::string s;
  lda_status st = guard([&] { s = lda_host::groupTopicsFormat(G, n, ids, values); });
  return st ? st : copy_text(s, buf, cap, len);
}

lda_status ldatm_subcorpus_top_words(ldatm* m, const uint8_t* doc_mask, int32_t n, int32_t* word_ids, int32_t* counts,
                                     int64_t* totals) {
  TM_CHECK(m);
  return guard([&] { m->model.subCorpusTopWords(doc_mask, n, word_ids, counts, totals); });
}

lda_status ldatm_save(ldatm* m, const char* path) {
  TM_CHECK(m);
  if (!path) {
    g_tm_error = "null path";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] { m->model.save(path); });
}

lda_status ldatm_load(ldatm** out, const char* path) {
  if (!out || !path) {
    g_tm_error = "null argument";
    return LDA_ERR_INVALID_ARG;
  }
  *out = nullptr;
  return guard([&] {
    auto loaded = lda_host::ParallelTopicModel::load(path);
    *out = new ldatm(std::move(loaded));
  });
}

lda_status ldatm_infer(ldatm* m, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                       int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed,
                       double* theta) {
  TM_CHECK(m);
  return guard([&] { m->model.infer(Dh, doc_off, words, num_iterations, thinning, burn_in, seed, theta); });
}

lda_status ldatm_score_theta(ldatm* m, int32_t metric, int64_t Q, const double* theta, int64_t M,
                             const int64_t* docs, double* scores) {
  TM_CHECK(m);
  if (!scores) {
    g_tm_error = "null scores";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] { m->model.scoreTheta(metric, Q, theta, M, docs, scores); });
}

lda_status ldatm_score(ldatm* m, int32_t metric, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                       int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed, int64_t M,
                       const int64_t* docs, double* scores, double* theta_out) {
  TM_CHECK(m);
  if (!scores) {
    g_tm_error = "null scores";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] {
    std::vector<double> own;
    double* theta = theta_out;
    if (!theta && Dh > 0) {
      own.resize((size_t)Dh * (size_t)m->model.numTopics());
      theta = own.data();
    }
    m->model.infer(Dh, doc_off, words, num_iterations, thinning, burn_in, seed, theta);
    m->model.scoreTheta(metric, Dh, theta, M, docs, scores);
  });
}

lda_status ldatm_heldout_loglik(ldatm* m, int64_t Dh, const double* theta, const int64_t* doc_off,
                                const int32_t* words, double* doc_ll, double* total) {
  TM_CHECK(m);
  if (Dh > 0 && !doc_ll) {
    g_tm_error = "null doc_ll";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] {
    const double t = m->model.heldOutLogLik(Dh, theta, doc_off, words, doc_ll);
    if (total) *total = t;
  });
}

lda_status ldatm_evaluate(ldatm* m, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                          int32_t num_iterations, int32_t thinning, int32_t burn_in, uint64_t seed,
                          double* doc_ll, double* total, int64_t* tokens_scored, double* theta_out) {
  TM_CHECK(m);
  if (Dh > 0 && !doc_ll) {
    g_tm_error = "null doc_ll";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] {
    const double t = m->model.evaluate(Dh, doc_off, words, num_iterations, thinning, burn_in, seed, doc_ll,
                                       tokens_scored, theta_out);
    if (total) *total = t;
  });
}

lda_status ldatm_left_to_right(ldatm* m, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                               int32_t num_particles, int32_t resampling, uint64_t seed, double* doc_ll,
                               double* total, int64_t* tokens_scored) {
  TM_CHECK(m);
  if (Dh > 0 && !doc_ll) {
    g_tm_error = "null doc_ll";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] {
    const double t = m->model.leftToRight(Dh, doc_off, words, num_particles, resampling, seed, doc_ll,
                                          tokens_scored);
    if (total) *total = t;
  });
}

lda_status ldatm_completion_split(int32_t num_types, int64_t Dh, const int64_t* doc_off, const int32_t* words,
                                  int64_t* obs_off, int32_t* obs_words, int64_t* sc_off, int32_t* sc_words) {
  if (Dh < 0 || !doc_off || !obs_off || !sc_off || (Dh > 0 && doc_off[Dh] > doc_off[0] && !words)) {
    g_tm_error = "null argument";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] {
    std::vector<int64_t> oo, so;
    std::vector<int32_t> o, s;
    lda_host::ParallelTopicModel::completionSplit(num_types, Dh, doc_off, words, oo, o, so, s);
    std::copy(oo.begin(), oo.end(), obs_off);
    std::copy(so.begin(), so.end(), sc_off);
    if (obs_words) std::copy(o.begin(), o.end(), obs_words);
    if (sc_words) std::copy(s.begin(), s.end(), sc_words);
  });
}

lda_status ldatm_score_top(ldatm* m, int32_t metric, int64_t Q, const double* theta, int32_t n, int64_t* doc_ids,
                           double* scores) {
  TM_CHECK(m);
  if (!doc_ids || !scores) {
    g_tm_error = "null output";
    return LDA_ERR_INVALID_ARG;
  }
  return guard([&] { m->model.scoreTop(metric, Q, theta, n, doc_ids, scores); });
}

}  // extern "C"
