// bc_engine_impl.h -- what the engine's translation units (bc_engine.hip, bc_keys.hip, bc_finish.hip, bc_probe.hip,
// bc_synth.hip, bc_text.hip) share: struct bc_engine and the small structs that own what the text renderers keep on the
// device between calls, the HIP_TRY / ScratchGuard pair every function of the C ABI is written with (and StreamTimer
// beside them), the functions one of them defines and another calls, and the undocumented hooks of the exchange
// (bc_comm.hip includes it for those alone).  A kernel is launched only from the file that defines it: what crosses a
// file is a host function declared here.  Internal: no other file includes it.
#ifndef BC_ENGINE_IMPL_H
#define BC_ENGINE_IMPL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/barcode_count_hip.h"
#include "bc_enrich.h"
#include "bc_jit.h"
#include "bc_plan.hpp"

// A failed HIP call becomes a status + message; running out of device or pinned memory is BC_ERR_NOMEM, not BC_ERR_HIP.
#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      bc::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                    \
      if (_e == hipErrorOutOfMemory) (void)hipGetLastError(); /* not sticky: the engine stays usable */ \
      return _e == hipErrorOutOfMemory ? BC_ERR_NOMEM : BC_ERR_HIP;                        \
    }                                                                                      \
  } while (0)

// Device / pinned scratch that is released on every way out of a function (HIP_TRY returns early).
struct ScratchGuard {
  std::vector<void*> dev, pinned;
  std::vector<hipEvent_t> events;
  ~ScratchGuard() {
    for (void* p : dev) (void)hipFree(p);
    for (void* p : pinned) (void)hipHostFree(p);
    for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
  }
  template <typename T>
  hipError_t dmalloc(T** out, size_t bytes) {
    void* p = nullptr;
    const hipError_t rc = hipMalloc(&p, bytes ? bytes : 16);
    if (rc == hipSuccess) dev.push_back(p);
    *out = (T*)p;
    return rc;
  }
  template <typename T>
  hipError_t hmalloc(T** out, size_t bytes) {
    void* p = nullptr;
    const hipError_t rc = hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault);
    if (rc == hipSuccess) pinned.push_back(p);
    *out = (T*)p;
    return rc;
  }
  hipError_t event(hipEvent_t* out) {
    const hipError_t rc = hipEventCreateWithFlags(out, hipEventDisableTiming);
    if (rc == hipSuccess) events.push_back(*out);
    return rc;
  }
  // p, a dmalloc of this guard (or NULL), is the caller's from now on
  template <typename T>
  T* release(T* p) {
    if (p) dev.erase(std::find(dev.begin(), dev.end(), (void*)p));
    return p;
  }
};

// The device time a stream spends between start() and stop(), from two events that a guard owns.
struct StreamTimer {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipStream_t stream = nullptr;
  hipError_t start(ScratchGuard& g, hipStream_t s) {
    stream = s;
    for (hipEvent_t* ev : {&ev0, &ev1}) {
      const hipError_t rc = hipEventCreate(ev);
      if (rc != hipSuccess) return rc;
      g.events.push_back(*ev);
    }
    return hipEventRecord(ev0, stream);
  }
  // waits for the stream; *ms is written only when everything before it went well
  hipError_t stop(float* ms) {
    hipError_t rc = hipEventRecord(ev1, stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream);
    if (rc == hipSuccess) (void)hipEventElapsedTime(ms, ev0, ev1);
    return rc;
  }
};

// ---- what the text renderers (bc_text.hip) keep on the device between calls ----
// counts_epoch of the engine moves whenever what bc_engine_finish would hand out may have changed (counts_changed());
// a result derived from the counts carries the epoch it was made for, is served only while the two agree, and is dropped
// and rebuilt by the next render after that.  An epoch of 0 never agrees.

// The IDs of the counted sets (bc_line.h), built at the first render, and the canonical map of the enrichment renderers
// beside it.  Both live among the engine's allocs and go with the engine: there is nothing to drop.
struct LabelPool {
  bool ready = false;
  uint32_t* d_off = nullptr;             // per group N_g + 1 offsets, back to back
  uint8_t* d_bytes = nullptr;
  uint32_t off_start[bc::kMaxGroups] = {0};
  uint32_t max_len[bc::kMaxGroups] = {0};  // the longest ID of each counted set
  bool canon_ready = false;              // the canonical map has been built
  uint32_t* d_canon = nullptr;           // canon[off_g + i]; NULL when no set shares an ID
};

// The folded marginal sums of a dense plan (bc_enrich_render.h): S * SUM singles, then S * P doubles.  Never served for
// a table somebody else may write (caller-owned, or its pointer handed out): their epoch stays 0 then.
struct DenseSums {
  uint64_t epoch = 0;
  unsigned long long* d = nullptr;
  uint64_t passes = 0;                   // table passes made for them since the engine was created
  void drop() {
    if (d) (void)hipFree(d);
    d = nullptr;
    epoch = 0;
  }
};

// The keys and counts of a sparse plan in the order of its files: the raw-key renderer's (key, count) pairs, re-keyed
// and sorted (bc_raw_render.h, bc_sort.h), or the wide-key renderer's keys of key_words u64 each, gathered into order
// (bc_wide_render.h).  The S + 1 renders of one merged run sort once.
struct SortedRows {
  uint64_t epoch = 0;
  uint64_t* d_keys = nullptr;
  uint32_t* d_cnts = nullptr;
  uint64_t n = 0;
  uint64_t sorts = 0;                    // sorts made since the engine was created
  float sort_ms = 0.f;                   // export + (re-key | order keys) + sort (+ gather) of the last one, from HIP events
  void drop() {
    if (d_keys) (void)hipFree(d_keys);
    if (d_cnts) (void)hipFree(d_cnts);
    d_keys = nullptr;
    d_cnts = nullptr;
    n = 0;
    epoch = 0;
  }
};

// One kind of a raw-key plan's enrichment (bc_raw_enrich_render.h): the (projected key, sum) segments made from the
// sorted rows (project, bc_sort.h, bc_reduce.h), in one allocation -- n keys, n sums, n_seg + 1 segment starts, u64 all.
struct RawEnrichSegs {
  uint64_t epoch = 0;
  void* d = nullptr;
  uint64_t n = 0;
  uint32_t n_seg = 0;
  void drop() {
    if (d) (void)hipFree(d);
    d = nullptr;
    n = 0;
    n_seg = 0;
    epoch = 0;
  }
};

// most reads of one log-mode match launch + fold (BC_COUNT_LOG_CHUNK is clamped to it)
constexpr uint64_t kLogChunkMax = 1ull << 27;

struct bc_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t copy_stream = nullptr;
  bc::HostDevPlan h;
  bc::DevPlan* d_plan = nullptr;
  std::vector<void*> allocs;
  uint32_t* d_table = nullptr;
  bool own_table = false;
  uint64_t table_entries = 0;
  uint32_t* d_bits = nullptr;   // two-level counting: the first-occurrence bit of every tuple (large dense tables)
  uint64_t n_bit_words = 0;
  bool bits_dirty = false;      // some bit may be set: fold before anyone reads the table
  bool table_exposed = false;   // bc_engine_table_ptr has handed the table out: every sync folds, as for a caller's table
  uint64_t dirty_bytes = 0;     // the dirty-block map behind the bit map (DevPlan::dirty_off): one flag per 64 entries
  bool table_all_dirty = false; // somebody wrote the table without flagging (a fold, the wave-per-read kernel, a caller
                                // holding its pointer): the next reset zeroes all of it
  uint64_t reads_since_fold = 0;  // upper bound on the bits set since then: picks the fold kernel
  // log-mode counting (bc_fold.h): BC_COUNT_LOG = 0 never | 1 whenever the plan allows it | auto (default): submits of
  // at least log_min_reads reads (BC_COUNT_LOG_MIN_READS).  Either way the counts are the same.
  int count_log = 2;
  uint64_t log_min_reads = 1ull << 24;
  uint64_t log_chunk = kLogChunkMax;   // reads per match launch + fold (BC_COUNT_LOG_CHUNK, a multiple of 64)
  bool log_hot = false;              // the hot-counter cache in log mode too (BC_COUNT_LOG_HOT=0|1; off: 4.62 vs 4.75 ms
                                     // for config 3's match kernel -- the fold's LDS atomics take hot tuples in stride)
  uint64_t log_cap = 0;              // entries allocated in d_log / d_grouped
  uint32_t* d_log = nullptr;
  uint32_t* d_grouped = nullptr;
  uint64_t gz_segments = 0;          // segments of ordinary gzip streams inflated on the device (bc_engine_gz_segments_inflated)
  uint64_t gz_blocks = 0;            // BGZF blocks inflated on the device for this engine (bc_engine_gz_blocks_inflated)
  uint64_t log_folds = 0;            // folds run since the engine was created (bc_engine_count_log_folds)
  uint32_t* d_fold_meta = nullptr;   // [cnt | start | cursor | item_off], kFoldMaxBuckets + 1 words each
  // What the last reset owes (settle_owed()): a reset only records it, and whoever touches table, dirty map or bit map
  // next pays it first, on the engine's stream -- except a log-mode submit, whose match kernel touches none of them:
  // there the table's part runs on reset_stream beside the match kernel and is joined before the fold
  // (BC_COUNT_LOG_DEFER_RESET=0|1), and the fold takes the bit map as all zero without anyone writing the zeros first
  // (bc_fold.h, a fresh fold; BC_COUNT_LOG_FRESH=0|1).  The table's part is only ever owed for a table nobody else can
  // see (engine-owned, its pointer not handed out): whoever holds a pointer may order work after the reset by the stream.
  bool owed_table = false;           // the dirty-block reset, or (owed_table_all) table and dirty map zeroed whole
  bool owed_table_all = false;
  bool owed_bits = false;            // the bit map zeroed
  bool defer_reset = true;
  bool fold_fresh = true;
  hipStream_t reset_stream = nullptr;  // created with the first deferred reset
  hipEvent_t reset_fork = nullptr, reset_join = nullptr;
  unsigned long long* d_counters = nullptr;
  uint32_t barcode_num = 0;
  uint32_t n_sets[bc::kMaxGroups] = {0};
  std::vector<std::vector<std::string>> set_seqs;  // per group: the known sequences in index order
  bool has_sample_group = false;
  uint8_t* trace_outcome = nullptr;
  uint64_t* trace_idx = nullptr;
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  std::vector<float> launch_ms;  // resolved launch times not yet handed out (bc_engine_kernel_ms[_each])
  // compacted results
  std::vector<uint64_t> row_idx;
  std::vector<uint32_t> row_cnt;
  // host staging (bc_engine_submit_host)
  static constexpr int kStages = 2;
  uint8_t* pin[kStages] = {nullptr, nullptr};
  uint8_t* dev[kStages] = {nullptr, nullptr};
  hipEvent_t copied[kStages] = {nullptr, nullptr};
  hipEvent_t consumed[kStages] = {nullptr, nullptr};
  size_t stage_bytes = 0;
  uint32_t lds_limit = 0;
  uint32_t n_cus = 0;
  bc::JitKernels jit;  // scheme-specialised kernels, one per kernel shape (NW, NWW, lengths, tables, tracing)
  uint64_t reads_seen = 0;  // reads submitted so far: a cache miss is only worth a compile for a long run
  int jit_mode = 1;  // BC_JIT = 0: never | 1 (default): cache hit -> at once, else compiled in the background once 2^20
                     // reads have been seen | force (2): always, compiled synchronously | cached (3): cache hits only
  std::string last_kernel;
  // the last match launch: the specialised kernel's shape key (0: the generic kernel ran), its dynamic LDS and its grid
  // (bc_internal_last_launch)
  uint64_t last_key = 0;
  uint32_t last_lds = 0, last_grid = 0, last_resident = 0;
  bool pipe = true;   // software-pipelined tile fetch (BC_PIPE=0|1)
  bool qshare = true; // the specialised kernel's tile regions: one per wave, shared by sequence and quality lines
                      // (BC_QUAL_REGION=own|shared, read when the engine is created)
  int lhash_mode = 1; // LDS exact-match tables (PlanSetup::lhash_mode)
  // random-barcode mode: the hash set of (tuple, random barcode) keys
  unsigned long long* d_slots = nullptr;
  uint32_t* d_vals = nullptr;  // sparse plans without a random barcode: the count of each key
  uint64_t n_slots = 0;
  uint32_t key_words = 1;      // u64 words per key: 1, or the plan's wide keys (bc_long.h)
  uint32_t* d_ready = nullptr;  // wide keys: a slot's payload has been published
  std::vector<uint64_t> row_wide;  // compacted rows of a wide-key plan: key_words words per row (row_idx stays empty)
  uint64_t key_bound = 0;  // upper bound on the keys held: reads submitted / keys imported so far
  // the wave-per-read kernel's plan (bc_long.h): built when a submit needs it -- reads above 320 bases -- or at
  // creation when the lane-per-read kernel cannot run the plan at all (long_only)
  bool long_only = false, long_ready = false;
  bool long_lowered = false;          // lh holds the lowered plan already (long_only, or a wide-key lane plan: the key
                                      // layout that rows, renderers and exchange read is lh's)
  uint64_t wide_lane_reads = 0;       // reads submitted to the lane-per-read kernel under a wide-key plan (h.plan.wide:
                                      // BC_WIDE_LANE=1 and an eligible plan) since creation (bc_engine_wide_lane_reads)
  bc::LongHost lh;
  bc::LongPlan* d_long = nullptr;
  const bc_plan* src_plan = nullptr;  // (the caller keeps the plan alive for the engine's lifetime)
  bool table_materialized = false;  // random-barcode plans: d_table holds the per-tuple distinct counts of the current
                                    // key set (bc_engine_materialize_table), possibly summed over ranks since
  // what the text renderers keep between calls (the structs above)
  uint64_t counts_epoch = 1;
  LabelPool labels;
  DenseSums sums;
  SortedRows raw_rows, wide_rows;
  RawEnrichSegs raw_enrich[2];           // [0] Single, [1] Double: made from raw_rows, and dropped with them
  uint64_t raw_enrich_builds = 0;        // kinds built since the engine was created (bc_engine_raw_enrich_reduces)
  float raw_enrich_ms = 0.f;             // project + sort + reduce of the last one, from HIP events
  // The strand setting (bc_strand.hip), read from the plan at creation.  BC_STRAND_FORWARD: nothing below is ever
  // allocated and no submit goes near it.
  int strand = BC_STRAND_FORWARD;
  uint64_t strand_chunk = 1ull << 24;    // reads per orient / two-pass round (BC_STRAND_CHUNK, a multiple of 256)
  uint8_t* d_strand = nullptr;           // the scratch batch, the list, select's block counts and the outcome bytes
  size_t strand_bytes = 0;
  unsigned long long* d_strand_stats = nullptr;  // retried | matched_reverse | BC_MATCHED ahead of the reverse pass
  uint32_t* strand_count_pin = nullptr;  // pinned: the number of reads select has listed
};

namespace bc {

// whatever bc_engine_finish would hand out may have changed (bc_engine::counts_epoch)
inline void counts_changed(bc_engine* e) { ++e->counts_epoch; }

// ---- defined in bc_engine.hip ----
uint32_t grid_for(uint64_t n);  // workgroups of 256 for a grid-stride loop over n items
// src -> a device allocation the engine owns until it is freed; *out: its address
int upload(bc_engine* e, const void* src, size_t bytes, uint64_t* out);
// Everything a reset owes (bc_engine::owed_*), on the engine's stream: first thing in every path that reads or writes
// table, dirty map or bit map.
int settle_owed(bc_engine* e);
// bc_fix_error's kernel: one wavefront on the null stream of the current device, *d_out its verdict; the caller reads
// hipGetLastError()
void fix_error_launch(const DevGroup& G, uint32_t q1, uint32_t q2, uint32_t qn, uint32_t qx, uint32_t* d_out);
// staging copy pageable <-> pinned, cut into slices for a few threads (BC_STAGE_THREADS)
void staged_copy(void* dst, const void* src, size_t n);
// One checked batch counted as it stands, enqueued on the engine's stream: what every submit of a BC_STRAND_FORWARD
// engine is, and each pass of the others.  trace_outcome / trace_idx: where the per-read outcomes and indexes go
// (both NULL: not recorded).
int submit_forward(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens, uint32_t stride,
                   uint32_t read_len, uint64_t n_reads, uint8_t* trace_outcome, uint64_t* trace_idx);

// ---- defined in bc_strand.hip ----
// A checked batch of an engine whose strand is not BC_STRAND_FORWARD; a caller's trace receives the reads' final
// outcomes from trace_off on.  BC_STRAND_BOTH: waits for the device once per chunk of strand_chunk reads.
int submit_strand(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens, uint32_t stride,
                  uint32_t read_len, uint64_t n_reads, uint64_t trace_off);
void strand_free(bc_engine* e);  // (the stream has drained)

// ---- defined in bc_keys.hip ----
// Keeps the key table at most half full for `more` further keys (plans with a random barcode or raw captures; a no-op
// for the others).  Growing allocates a table of twice the size (or more) and re-inserts the old keys on the device.
int set_reserve(bc_engine* e, uint64_t more);
// Empties the key table where it stands (enqueued on the engine's stream) and forgets what was derived from its keys.
int clear_key_table(bc_engine* e);
// The (tuple key, count) pairs of a narrow-key map as they stand, into buffers that `g` owns: a random-barcode plan's key
// set first aggregated into per-tuple distinct counts.  e->d_slots is not NULL; the stream has drained on return.
int export_pairs(bc_engine* e, const char* who, ScratchGuard& g, uint64_t** d_key, uint32_t** d_cnt, uint64_t* n);
// The same for a wide-key map (bc_long.h): n keys of e->key_words words each, and their counts, a random-barcode plan's
// key set first re-inserted with its random planes cleared.  What bc_engine_finish hands out and the wide-key renderer
// sorts.  e->d_slots is not NULL; the stream has drained on return.
int export_wide(bc_engine* e, const char* who, ScratchGuard& g, unsigned long long** d_key, uint32_t** d_cnt, uint64_t* n);

// ---- defined in bc_finish.hip ----
// What every reader of a dense plan's counts does first (bc_engine_finish, bc_engine_enrich, the renderers): wait for the
// submits, and for a random-barcode plan turn the key set into per-tuple counts unless that has been done for the
// current keys.  Afterwards entry i counts table[i] + bit i of the bit map (when e->bits_dirty: two-level counting, not
// folded).
int dense_counts_ready(bc_engine* e);
// The shape of a dense plan's enrichment (bc_engine_enrich); false + set_error() for plans that have none.
bool enrich_shape(const bc_engine* e, const char* who, EnrichShape* sh, uint64_t* n_samples);

}  // namespace bc

// Hooks for the engine library's own end-of-run exchange (bc_comm.hip); not part of the documented ABI.
extern "C" {
// (bc_engine.hip) the table as it stands, with the bit map beside it (*bits: NULL when nothing is pending there) ...
void* bc_internal_table_unfolded(bc_engine* e, const void** bits);
// ... and the caller's word that the table has been overwritten with plain counts
int bc_internal_table_now_plain(bc_engine* e);
// (bc_probe.hip) bc_table_pack_u8 with the first-occurrence bit map of two-level counting read alongside
int bc_internal_table_pack_u8(const void* d_table_u32, const void* d_bits, uint64_t n, void* d_out_u8, void* d_ovf_idx_u64,
                              void* d_ovf_val_u32, uint64_t ovf_capacity, uint64_t* n_ovf, int device_id, void* hip_stream);
}

#endif
