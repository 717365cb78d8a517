// bc_engine.hip -- gfx950 kernels and the engine half of the C ABI (include/barcode_count_hip.h).
//
// Replaces, per GPU, the worker pool of the reference (main.rs:93-120: threads-1 clones of
// SequenceParser popping packed records from a mutex-guarded queue, parse.rs:53-86) by one
// kernel launch per batch: one LANE per read (64 reads per wavefront), reads staged through
// LDS with 16-byte coalesced loads, outcome counters reduced per workgroup, one no-return
// global atomic per matched read into the dense (sample, barcode tuple) counter table that
// stands in for Results' nested HashMap (info.rs:661-665).
//
// This file is the hot path: the generic match kernels and their launch, log-mode counting and the owed reset, the
// engine's creation, submits, sync and reset, and the small accessors.  The key tables are bc_keys.hip, the rows and
// the dense enrichment bc_finish.hip, probes and table packing bc_probe.hip, the read generator bc_synth.hip.
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include <algorithm>
#include <thread>
#include <string>
#include <vector>

#include "../../include/barcode_count_hip.h"
#include "bc_kernel.h"
#include "bc_engine_impl.h"
#include "bc_fold.h"

namespace bc {

// generic kernel: any plan, read from device memory
template <int NW, int NWW>
__global__ __launch_bounds__(kTPB, ((NW <= 4 && NWW <= 2) ? BC_MIN_WAVES : 1)) void match_count_kernel(
    const DevPlan* __restrict__ plp, const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual,
    const uint16_t* __restrict__ lens, const uint16_t* __restrict__ qlens, uint32_t stride, uint32_t read_len, uint32_t nd,
    uint64_t n_reads, uint32_t region,
    uint32_t* __restrict__ table, uint32_t* __restrict__ bits, unsigned long long* __restrict__ slots,
    uint32_t* __restrict__ vals, uint64_t smask,
    unsigned long long* __restrict__ counters, uint8_t* __restrict__ trace_outcome, uint64_t* __restrict__ trace_idx,
    uint32_t flags, uint32_t* __restrict__ count_log) {
  if (lens)
    match_count_body<NW, NWW, true>(*plp, seq, qual, lens, qlens, stride, read_len, nd, n_reads, region, table, bits, slots, vals, smask,
                                    counters, trace_outcome, trace_idx, flags, count_log);
  else
    match_count_body<NW, NWW, false>(*plp, seq, qual, lens, nullptr, stride, read_len, nd, n_reads, region, table, bits, slots, vals, smask,
                                     counters, trace_outcome, trace_idx, flags, count_log);
}

// ... for a plan with wide keys (DevPlan::wide): the key is assembled in registers and inserted by all lanes at once
template <int NW, int NWW>
__global__ __launch_bounds__(kTPB, ((NW <= 4 && NWW <= 2) ? BC_MIN_WAVES : 1)) void match_count_wide_kernel(
    const DevPlan* __restrict__ plp, const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual,
    const uint16_t* __restrict__ lens, const uint16_t* __restrict__ qlens, uint32_t stride, uint32_t read_len, uint32_t nd,
    uint64_t n_reads, uint32_t region, unsigned long long* __restrict__ slots, uint32_t* __restrict__ vals,
    uint32_t* __restrict__ ready, uint64_t smask, unsigned long long* __restrict__ counters,
    uint8_t* __restrict__ trace_outcome, uint64_t* __restrict__ trace_idx, uint32_t flags) {
  if (lens)
    match_count_body<NW, NWW, true, false, true>(*plp, seq, qual, lens, qlens, stride, read_len, nd, n_reads, region, nullptr, nullptr,
                                                 slots, vals, smask, counters, trace_outcome, trace_idx, flags, nullptr, ready);
  else
    match_count_body<NW, NWW, false, false, true>(*plp, seq, qual, lens, nullptr, stride, read_len, nd, n_reads, region, nullptr,
                                                  nullptr, slots, vals, smask, counters, trace_outcome, trace_idx, flags, nullptr, ready);
}

// The wave-per-read kernel (bc_long.h): reads, groups, references and budgets beyond the lane-per-read kernel's widths
__global__ __launch_bounds__(256) void long_match_kernel(const LongPlan* __restrict__ plp, const uint8_t* __restrict__ seq,
                                                         const uint8_t* __restrict__ qual, const uint16_t* __restrict__ lens,
                                                         const uint16_t* __restrict__ qlens, uint32_t stride, uint32_t read_len,
                                                         uint64_t n_reads, uint32_t* __restrict__ table,
                                                         unsigned long long* __restrict__ slots, uint32_t* __restrict__ vals,
                                                         uint32_t* __restrict__ ready, uint64_t smask,
                                                         unsigned long long* __restrict__ counters,
                                                         uint8_t* __restrict__ trace_outcome, uint64_t* __restrict__ trace_idx) {
  __shared__ uint64_t s_wide[4][kMaxKeyWords];  // the wave's wide key (plans with wide keys)
  const LongPlan& pl = *plp;
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t* wide_key = s_wide[threadIdx.x >> 6];
  const uint64_t n_waves = (uint64_t)gridDim.x * 4u;
  uint32_t acc[kNCounters];
#pragma unroll
  for (int k = 0; k < kNCounters; ++k) acc[k] = 0;
  for (uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); r < n_reads; r += n_waves) {
    const uint32_t len = lens ? (uint32_t)lens[r] : read_len;
    const uint32_t qlen = qlens ? (uint32_t)qlens[r] : len;
    uint64_t didx, rcode;
    uint32_t outcome = long_match_read(pl, seq + r * stride, len, qual ? qual + r * stride : seq, qual ? qlen : 0u, didx, rcode, wide_key);
    const uint64_t key = pl.has_random ? didx * pl.rspace + rcode : didx;
    if (lane == 0) {
      if (outcome == kMatched && pl.wide) {
        // Results::add_count under a wide key (info.rs:742-802): a set of (tuple, random) keys, or a map of tuple counts
        if (pl.has_random || !pl.discard_counts) {
          bool is_new;
          const uint64_t slot = wide_find_or_insert(slots, ready, smask, pl.key_words, wide_key, is_new);
          if (pl.has_random) {
            if (!is_new) outcome = kDuplicate;
          } else {
            atomicAdd(&vals[slot], 1u);
          }
        }
      } else if (outcome == kMatched) {
        if (pl.has_random) {
          if (!set_insert(slots, smask, key)) outcome = kDuplicate;  // Results::add_count, info.rs:770-802
        } else if (!pl.discard_counts) {
          if (pl.sparse)
            atomicAdd(&vals[map_slot(slots, smask, didx)], 1u);
          else
            atomicAdd(&table[didx], 1u);  // info.rs:761-767
        }
      }
      if (trace_outcome) {
        trace_outcome[r] = (uint8_t)outcome;
        trace_idx[r] = pl.wide ? (outcome == kMatched || outcome == kDuplicate ? wide_key[0] : 0ull) : key;
      }
      acc[outcome < (uint32_t)kNCounters ? outcome : kUnsupported] += 1u;
      acc[kTotalReads] += 1u;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kNCounters; ++k)
      if (acc[k]) atomicAdd(&counters[k], (unsigned long long)acc[k]);
  }
}

// ------------------------------------------------------------------------------------------------
// plan-time kernels
// ------------------------------------------------------------------------------------------------
// correction table of a short barcode: fix_error's verdict for every N-free capture
__global__ void build_dtable_kernel(const DevPlan* __restrict__ plp, uint32_t g, uint32_t* __restrict__ out) {
  const DevGroup& G = plp->groups[g];
  const uint32_t nq = 1u << (2 * G.len);
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  out[q] = dtable_entry(G, q);
}

// bc_fix_error (bc_probe.hip): one wavefront, one query, plain fix_error semantics (no exact-member shortcut).  It
// lives beside the match kernels, the other users of wave_fix_error: compiled on its own it comes out register for
// register different.
__global__ void fix_error_kernel(DevGroup G, uint32_t q1, uint32_t q2, uint32_t qn, uint32_t qx, uint32_t* out) {
  const uint32_t r = wave_fix_error(G, q1, q2, qn, qx, false);
  if (threadIdx.x == 0) *out = r;
}

// Two-level counting (bc_kernel.h): count = bit + table entry.  Folds the bits into the table (one add per set bit, in
// address order) and clears them, so that everything downstream sees plain u32 counts.
__global__ void fold_bits_kernel(uint32_t* __restrict__ bits, uint64_t n_words, uint32_t* __restrict__ table, uint64_t entries) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; j < n_words; j += step) {
    uint32_t w = bits[j];
    if (!w) continue;
    bits[j] = 0u;
    const uint64_t base = j << 5;
    while (w) {
      const uint32_t b = (uint32_t)__ffs(w) - 1u;
      w &= w - 1u;
      if (base + b < entries) table[base + b] += 1u;
    }
  }
}

// The same for a map with many bits set (a long job): a streaming pass over the table, four entries per lane; eight
// consecutive lanes share one word of the map (same wavefront, so all of them have read it before lane 0 of the eight
// clears it).  Writes only the 16-byte pieces that change.
__global__ void fold_bits_dense_kernel(uint32_t* __restrict__ bits, uint64_t n_words, uint4* __restrict__ table4, uint64_t entries) {
  const uint64_t n4 = entries >> 2;  // (entries of a large dense table: a multiple of 4 is not guaranteed -- tail below)
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;  // a multiple of 64
  for (; i < (n_words << 3); i += step) {
    const uint32_t w = bits[i >> 3];
    const uint32_t four = (w >> ((uint32_t)(i & 7u) * 4u)) & 15u;
    if (four && i < n4) {
      uint4 v = table4[i];
      v.x += four & 1u;
      v.y += (four >> 1) & 1u;
      v.z += (four >> 2) & 1u;
      v.w += (four >> 3) & 1u;
      table4[i] = v;
    } else if (four) {  // the last, partial group of four
      uint32_t* t = reinterpret_cast<uint32_t*>(table4);
      for (uint32_t k = 0; k < 4; ++k)
        if (((four >> k) & 1u) && (i << 2) + k < entries) t[(i << 2) + k] += 1u;
    }
    if ((i & 7u) == 0u && w) bits[i >> 3] = 0u;
  }
}

// bc_engine_reset with a dirty-block map (DevPlan::dirty_off): zeroes the 64-entry blocks of the table that somebody
// added to since the last reset, and the flags.  16 flags (one uint4) per lane and step.
__global__ void sparse_reset_kernel(uint32_t* __restrict__ table, uint4* __restrict__ dirty16, uint64_t n16, uint64_t entries) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  for (; i < n16; i += step) {
    const uint4 v = dirty16[i];
    if ((v.x | v.y | v.z | v.w) == 0u) continue;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) == 0u) continue;
      const uint64_t first = (i * 16 + (uint64_t)k) * 64;  // first table entry of the block
      if (first + 64 <= entries) {
        uint4* b = reinterpret_cast<uint4*>(table + first);
#pragma unroll
        for (int q = 0; q < 16; ++q) b[q] = zero;
      } else {
        for (uint64_t e = first; e < entries; ++e) table[e] = 0u;
      }
    }
    dirty16[i] = zero;
  }
}

}  // namespace bc

using namespace bc;

int bc::upload(bc_engine* e, const void* src, size_t bytes, uint64_t* out) {
  void* d = nullptr;
  HIP_TRY(hipMalloc(&d, bytes ? bytes : 16));
  e->allocs.push_back(d);
  if (bytes) HIP_TRY(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
  *out = (uint64_t)(uintptr_t)d;
  return BC_OK;
}

static void engine_free(bc_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (auto& ev : e->events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  for (int s = 0; s < bc_engine::kStages; ++s) {
    if (e->pin[s]) (void)hipHostFree(e->pin[s]);
    if (e->dev[s]) (void)hipFree(e->dev[s]);
    if (e->copied[s]) (void)hipEventDestroy(e->copied[s]);
    if (e->consumed[s]) (void)hipEventDestroy(e->consumed[s]);
  }
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->own_table && e->d_table) (void)hipFree(e->d_table);
  if (e->d_bits) (void)hipFree(e->d_bits);
  if (e->d_log) (void)hipFree(e->d_log);
  if (e->d_grouped) (void)hipFree(e->d_grouped);
  if (e->d_fold_meta) (void)hipFree(e->d_fold_meta);
  if (e->d_slots) (void)hipFree(e->d_slots);
  if (e->d_vals) (void)hipFree(e->d_vals);
  if (e->d_ready) (void)hipFree(e->d_ready);
  e->sums.drop();
  e->raw_rows.drop();
  e->wide_rows.drop();
  for (RawEnrichSegs& r : e->raw_enrich) r.drop();
  if (e->d_counters) (void)hipFree(e->d_counters);
  strand_free(e);
  if (e->d_plan) (void)hipFree(e->d_plan);
  if (e->reset_stream) (void)hipStreamSynchronize(e->reset_stream);
  if (e->reset_fork) (void)hipEventDestroy(e->reset_fork);
  if (e->reset_join) (void)hipEventDestroy(e->reset_join);
  if (e->reset_stream) (void)hipStreamDestroy(e->reset_stream);
  if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
  if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

static int engine_init(bc_engine* e, const bc_plan* p, int device_id, void* hip_stream, void* table_mem) {
  e->src_plan = p;
  // BC_WIDE_LANE=1: a plan with wide keys whose groups, budgets and format are within the lane kernel's widths is
  // lowered for that kernel (bc_plan::lower, allow_wide); default 0: such a plan runs on the wave-per-read kernel
  const char* wl_env = getenv("BC_WIDE_LANE");
  const bool allow_wide = wl_env && atoi(wl_env) != 0;
  if (p->lower(e->h, allow_wide)) {
    if (e->h.plan.wide) {
      // the key layout of rows, renderers and exchange is read from the wave-per-read plan: lowered now (host side),
      // uploaded when a batch above 320 bases needs that kernel (ensure_long)
      if (!p->lower_long(e->lh)) return BC_ERR_UNSUPPORTED;
      if (!e->lh.plan.wide || e->lh.plan.key_words != e->h.plan.key_words || e->lh.plan.rnd_bit != e->h.plan.rnd_bit) {
        set_error("bc_engine_create: the two kernels' key layouts differ");  // (cannot happen: one helper lays out both)
        return BC_ERR_STATE;
      }
      e->long_lowered = true;
      e->key_words = e->h.plan.key_words;
    }
  } else {
    // not a plan for the lane-per-read kernel (a group or a known barcode above 32 bases, more than 31 constant errors
    // allowed, a format above 320 bases): the wave-per-read kernel takes every batch
    const std::string why = get_error();
    if (!p->lower_long(e->lh)) {
      set_error(why);
      return BC_ERR_UNSUPPORTED;
    }
    e->long_only = true;
    e->long_lowered = true;
    // the fields of the lane plan that results, keys and rows are read from
    DevPlan& P = e->h.plan;
    memset(&P, 0, sizeof(P));
    const LongPlan& Q = e->lh.plan;
    P.L = Q.L;
    P.RL = Q.RL;
    P.n_groups = Q.n_groups;
    P.max_const = Q.max_const;
    P.quality_on = Q.quality_on;
    P.discard_counts = Q.discard_counts;
    P.has_random = Q.has_random;
    P.rnd_off = Q.rnd_off;
    P.rnd_len = Q.rnd_len;
    P.rspace = Q.rspace;
    P.sparse = Q.sparse;
    e->key_words = Q.wide ? Q.key_words : 1u;
    for (uint32_t g = 0; g < Q.n_groups; ++g) {
      P.groups[g].type = Q.groups[g].type;
      P.groups[g].off = Q.groups[g].off;
      P.groups[g].len = Q.groups[g].len;
      P.groups[g].n_refs = Q.groups[g].n_refs;
      P.groups[g].max_err = Q.groups[g].max_err;
      P.groups[g].table_stride = Q.groups[g].table_stride;
      P.groups[g].mode = Q.groups[g].n_refs ? kSetScan : kSetNone;
      P.groups[g].index = g;
    }
    e->h.table_entries = e->lh.table_entries;
    e->h.n_samples = e->lh.n_samples;
    e->h.sets.assign(Q.n_groups, HostSet());
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) {
    set_error("bc_engine_create: no HIP device " + std::to_string(device_id) + " (the engine has no CPU path)");
    return BC_ERR_HIP;
  }
  e->device = device_id;
  HIP_TRY(hipSetDevice(device_id));
  if (hip_stream) {
    e->stream = (hipStream_t)hip_stream;
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->own_stream = true;
  }
  HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device_id));
  e->lds_limit = (uint32_t)prop.maxSharedMemoryPerMultiProcessor;
  e->n_cus = (uint32_t)prop.multiProcessorCount;
  e->barcode_num = p->barcode_num;
  e->has_sample_group = p->sample_barcode;
  {
    // groups are ordered sample first, then counted barcodes (bc_plan::lower)
    if (p->sample_barcode) e->set_seqs.push_back(p->samples.seqs);
    for (uint32_t b = 0; b < p->barcode_num; ++b) e->set_seqs.push_back(p->counted[b].seqs);
  }

  DevPlan& P = e->h.plan;
  // the plan edits and bit-map layout an ahead-of-time build applies too
  const PlanSetup ps = plan_setup(e->h, e->long_only, table_mem == nullptr);
  e->lhash_mode = ps.lhash_mode;
  e->n_bit_words = ps.n_bit_words;
  e->dirty_bytes = ps.dirty_bytes;
  e->table_entries = P.sparse ? 0 : e->h.table_entries;
  if (const char* jm = getenv("BC_JIT"))
    e->jit_mode = !strcmp(jm, "force") ? 2 : (!strcmp(jm, "0") ? 0 : (!strcmp(jm, "cached") ? 3 : 1));
  for (uint32_t g = 0; g < P.n_groups; ++g) {
    DevGroup& G = P.groups[g];
    HostSet& H = e->h.sets[g];
    e->n_sets[g] = G.n_refs;
    int rc;
    if ((rc = upload(e, H.r1.data(), H.r1.size() * 4, &G.r1_a))) return rc;
    if ((rc = upload(e, H.r2.data(), H.r2.size() * 4, &G.r2_a))) return rc;
    if ((rc = upload(e, H.rn.data(), H.rn.size() * 4, &G.rn_a))) return rc;
    if ((rc = upload(e, H.rlen.data(), H.rlen.size(), &G.rlen_a))) return rc;
    if (G.mode == kSetHash) {
      if ((rc = upload(e, H.hkeys.data(), H.hkeys.size() * 8, &G.hkeys_a))) return rc;
      if ((rc = upload(e, H.hvals.data(), H.hvals.size() * 4, &G.hvals_a))) return rc;
      if (G.seed_nb) {
        if ((rc = upload(e, H.seed_off.data(), H.seed_off.size() * 4, &G.seed_off_a))) return rc;
        if ((rc = upload(e, H.seed_list.data(), H.seed_list.size() * 4, &G.seed_list_a))) return rc;
        if ((rc = upload(e, H.odd_list.data(), H.odd_list.size() * 4, &G.odd_list_a))) return rc;
        if (G.seed2_nb) {
          if ((rc = upload(e, H.seed2_off.data(), H.seed2_off.size() * 4, &G.seed2_off_a))) return rc;
          if ((rc = upload(e, H.seed2_list.data(), H.seed2_list.size() * 4, &G.seed2_list_a))) return rc;
        }
        if (G.seed3_nb) {
          if ((rc = upload(e, H.seed3_off.data(), H.seed3_off.size() * 4, &G.seed3_off_a))) return rc;
          if ((rc = upload(e, H.seed3_list.data(), H.seed3_list.size() * 4, &G.seed3_list_a))) return rc;
        }
        if (G.tier_blen) {
          if ((rc = upload(e, H.tier_off.data(), H.tier_off.size() * 4, &G.tier_off_a))) return rc;
          if ((rc = upload(e, H.tier_list.data(), H.tier_list.size() * 4, &G.tier_list_a))) return rc;
          if ((rc = upload(e, H.tier_bkt.data(), H.tier_bkt.size() * 4, &G.tier_bkt_a))) return rc;
        }
      }
    }
    if (G.mode == kSetDirect) {
      void* d = nullptr;
      HIP_TRY(hipMalloc(&d, (size_t)4 << (2 * G.len)));
      e->allocs.push_back(d);
      G.dtable_a = (uint64_t)(uintptr_t)d;
    }
  }
  e->strand = p->strand;
  if (const char* sc = getenv("BC_STRAND_CHUNK")) {
    const uint64_t c = strtoull(sc, nullptr, 0) & ~255ull;
    if (c) e->strand_chunk = std::min<uint64_t>(c, 1ull << 30);  // (select numbers a chunk's reads in 32 bits)
  }
  if (const char* cl = getenv("BC_COUNT_LOG")) e->count_log = strcmp(cl, "auto") == 0 ? 2 : atoi(cl);
  if (const char* ch = getenv("BC_COUNT_LOG_HOT")) e->log_hot = atoi(ch) != 0;
  if (const char* cd = getenv("BC_COUNT_LOG_DEFER_RESET")) e->defer_reset = atoi(cd) != 0;
  if (const char* cf = getenv("BC_COUNT_LOG_FRESH")) e->fold_fresh = atoi(cf) != 0;
  if (const char* cm = getenv("BC_COUNT_LOG_MIN_READS")) e->log_min_reads = strtoull(cm, nullptr, 0);
  if (const char* cc = getenv("BC_COUNT_LOG_CHUNK")) {
    const uint64_t c = strtoull(cc, nullptr, 0) & ~63ull;
    // (a log-mode specialised kernel numbers its tiles in 32 bits: bc_kernel.h tile_t)
    static_assert(kLogChunkMax <= (1ull << 37), "tile_t: tile number + waves of the grid must not wrap");
    if (c) e->log_chunk = std::min<uint64_t>(c, kLogChunkMax);
  }
  if (P.lhash_vec) {
    const int rc = upload(e, e->h.lhash.data(), e->h.lhash.size() * 4, &P.lhash_a);
    if (rc) return rc;
  }
#ifdef BC_EXPERIMENT
  if (const char* pm = getenv("BC_PIPE")) e->pipe = atoi(pm) != 0;
#endif
  e->qshare = qual_region_shared();
  HIP_TRY(hipMalloc((void**)&e->d_plan, sizeof(DevPlan)));
  HIP_TRY(hipMemcpy(e->d_plan, &P, sizeof(DevPlan), hipMemcpyHostToDevice));
  for (uint32_t g = 0; g < P.n_groups; ++g) {
    const DevGroup& G = P.groups[g];
    if (G.mode != kSetDirect) continue;
    const uint32_t nq = 1u << (2 * G.len);
    hipLaunchKernelGGL(build_dtable_kernel, dim3((nq + 255) / 256), dim3(256), 0, e->stream, e->d_plan, g,
                       reinterpret_cast<uint32_t*>((uintptr_t)G.dtable_a));
    HIP_TRY(hipGetLastError());
  }
  if (P.sparse) {
    if (table_mem) {
      set_error("bc_engine_create: the plan keeps raw captures (no dense table); pass table_mem = NULL");
      return BC_ERR_INVALID;
    }
  } else if (table_mem) {
    e->d_table = (uint32_t*)table_mem;
    e->table_all_dirty = true;  // (the caller may write it too: a reset zeroes all of it)
  } else {
    HIP_TRY(hipMalloc((void**)&e->d_table, e->table_entries * 4));
    e->own_table = true;
    HIP_TRY(hipMemsetAsync(e->d_table, 0, e->table_entries * 4, e->stream));
  }
  if (e->n_bit_words) {
    const size_t bytes = P.dirty_off ? (size_t)(P.dirty_off * 4 + e->dirty_bytes) : (size_t)(e->n_bit_words * 4);
    HIP_TRY(hipMalloc((void**)&e->d_bits, bytes));
    HIP_TRY(hipMemsetAsync(e->d_bits, 0, bytes, e->stream));
  }
  HIP_TRY(hipMalloc((void**)&e->d_counters, BC_NCOUNTERS * 8));
  HIP_TRY(hipMemsetAsync(e->d_counters, 0, BC_NCOUNTERS * 8, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BC_OK;
}

#ifdef BC_PROFILE
extern "C" __device__ unsigned long long bc_g_profile[16] = {};
// perf experiments (BC_PROFILE builds only): sums the tick counters of the generic and specialised kernels
extern "C" int bc_internal_profile_read(bc_engine* e, unsigned long long* out) {
  unsigned long long a[16];
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpyFromSymbol(a, HIP_SYMBOL(bc_g_profile), sizeof(a)));
  for (int k = 0; k < 16; ++k) out[k] = a[k];
  for (auto& kv : e->jit.slots) {
    if (!kv.second->fn) continue;
    hipDeviceptr_t p = nullptr;
    size_t sz = 0;
    if (hipModuleGetGlobal(&p, &sz, kv.second->mod, "bc_g_profile") != hipSuccess) continue;
    HIP_TRY(hipMemcpy(a, p, sizeof(a), hipMemcpyDeviceToHost));
    for (int k = 0; k < 16; ++k) out[k] += a[k];
  }
  return BC_OK;
}
#endif

// log mode applies to dense plans with a bit map whose indexes fit a u32 below the kLogNone sentinel
static bool log_mode_for(const bc_engine* e, uint64_t n_reads) {
  const DevPlan& P = e->h.plan;
  if (e->count_log == 0 || !e->d_bits || P.sparse || P.has_random || P.discard_counts || e->table_entries == 0 ||
      e->table_entries >= (uint64_t)kLogNone)
    return false;
  return e->count_log == 1 || n_reads >= e->log_min_reads;
}

// the log and its grouped copy: allocated once per engine, grown to the largest chunk seen (at most log_chunk)
static int ensure_log(bc_engine* e, uint64_t entries) {
  if (!e->d_fold_meta) {
    // (a fifth section: the saved bucket counts of the BC_FOLD_REUSE_CNT experiment)
    HIP_TRY(hipMalloc((void**)&e->d_fold_meta, 5 * (kFoldMaxBuckets + 1) * 4));
    HIP_TRY(hipMemsetAsync(e->d_fold_meta, 0, 5 * (kFoldMaxBuckets + 1) * 4, e->stream));
  }
  if (entries <= e->log_cap) return BC_OK;
  entries = (entries + 63) & ~63ull;
  if (e->d_log) {
    HIP_TRY(hipStreamSynchronize(e->stream));  // the last fold may still read them
    HIP_TRY(hipFree(e->d_log));
    HIP_TRY(hipFree(e->d_grouped));
    e->d_log = e->d_grouped = nullptr;
    e->log_cap = 0;
  }
  HIP_TRY(hipMalloc((void**)&e->d_log, entries * 4));
  HIP_TRY(hipMalloc((void**)&e->d_grouped, entries * 4));
  e->log_cap = entries;
  return BC_OK;
}

// the fold of the log's first n entries into bit map + table (bc_fold.h), on the engine's stream; fresh: onto a bit map
// that is owed its zeroing (the fold writes every word of it instead)
static int fold_log(bc_engine* e, uint64_t n, bool fresh) {
  const uint32_t nb = (uint32_t)((e->table_entries + (1ull << kFoldBucketShift) - 1) >> kFoldBucketShift);
  uint8_t* dirty = e->h.plan.dirty_off ? reinterpret_cast<uint8_t*>(e->d_bits + e->h.plan.dirty_off) : nullptr;
  bool have_cnt = false;
#ifdef BC_EXPERIMENT
  // BC_FOLD_REUSE_CNT=1 (perf experiment, for a benchmark that submits the SAME reads every time): the bucket counts
  // of the engine's first fold are kept and copied back (4 KB) instead of running bc_fold_hist again -- what a step
  // costs when the counts come for free, i.e. the most that counting them inside the match kernel could save
  static const bool reuse_cnt = getenv("BC_FOLD_REUSE_CNT") && atoi(getenv("BC_FOLD_REUSE_CNT")) != 0;
  uint32_t* saved = e->d_fold_meta + 4 * (kFoldMaxBuckets + 1);
  if (reuse_cnt && e->log_folds > 0) {
    HIP_TRY(hipMemcpyAsync(e->d_fold_meta, saved, (kFoldMaxBuckets + 1) * 4, hipMemcpyDeviceToDevice, e->stream));
    have_cnt = true;
  }
#endif
  HIP_TRY(fold_launch(e->stream, (const uint32_t*)e->d_log, n, e->d_grouped, e->d_fold_meta, nb, e->d_bits, e->n_bit_words,
                      e->d_table, dirty, e->n_cus, 0, 0, fresh, have_cnt));
#ifdef BC_EXPERIMENT
  if (reuse_cnt && e->log_folds == 0) {
    // (scan has zeroed cnt by now: count once more, for the copy)
    const uint64_t n4 = n / 4 + 1;
    hipLaunchKernelGGL(bc_fold_hist, dim3((uint32_t)std::min<uint64_t>((n4 + kFoldTPB - 1) / kFoldTPB, 4ull * e->n_cus)), dim3(kFoldTPB), 0,
                       e->stream, (const uint32_t*)e->d_log, n, nb, e->d_fold_meta);
    HIP_TRY(hipMemcpyAsync(saved, e->d_fold_meta, (kFoldMaxBuckets + 1) * 4, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_fold_meta, 0, (kFoldMaxBuckets + 1) * 4, e->stream));
  }
#endif
  ++e->log_folds;
  return BC_OK;
}


// The two parts of an owed reset (bc_engine::owed_*), enqueued on `st`; each clears its flag once it is enqueued.
static int settle_table_on(bc_engine* e, hipStream_t st) {
  if (!e->owed_table) return BC_OK;
  const uint64_t dirty_off = e->h.plan.dirty_off;
  if (!e->owed_table_all) {
    // two-level counting: after a short job the table is almost all zeros -- first occurrences live in the bit map --
    // and every add to it flagged its 256-byte block: zero those blocks and the flags (16.5 GB of memset -> 0.06 GB)
    hipLaunchKernelGGL(sparse_reset_kernel, dim3(grid_for(e->dirty_bytes / 16)), dim3(256), 0, st, e->d_table,
                       reinterpret_cast<uint4*>(e->d_bits + dirty_off), e->dirty_bytes / 16, e->table_entries);
    HIP_TRY(hipGetLastError());
  } else {
    if (e->d_table) HIP_TRY(hipMemsetAsync(e->d_table, 0, e->table_entries * 4, st));
    if (e->d_bits && dirty_off) HIP_TRY(hipMemsetAsync(e->d_bits + dirty_off, 0, e->dirty_bytes, st));
  }
  e->owed_table = e->owed_table_all = false;
  return BC_OK;
}
static int settle_bits_on(bc_engine* e, hipStream_t st) {
  if (!e->owed_bits) return BC_OK;
  HIP_TRY(hipMemsetAsync(e->d_bits, 0, e->n_bit_words * 4, st));
  e->owed_bits = false;
  return BC_OK;
}
// Everything owed, on the engine's stream: first thing in every path that reads or writes table, dirty map or bit map.
int bc::settle_owed(bc_engine* e) {
  int rc = settle_table_on(e, e->stream);
  if (rc == BC_OK) rc = settle_bits_on(e, e->stream);
  return rc;
}

// Who pays what a reset owes when a match launch meets it -- the one place that decides it.
//   kOwedMain   on the engine's stream, ahead of the match kernel (what every other path does: settle_owed)
//   kOwedSide   on reset_stream beside the match kernel, joined before the fold (BC_COUNT_LOG_DEFER_RESET)
//   kOwedFresh  never: the first fold takes the bit map as all zero and writes every word of it (BC_COUNT_LOG_FRESH)
// table_untouched: a log-mode launch whose kernel writes neither table nor dirty map.  No log-mode kernel touches the
// bit map, so its part can go aside or stay owed in any log-mode launch.
enum OwedWhere { kOwedMain, kOwedSide, kOwedFresh };
struct OwedPlan {
  OwedWhere table, bits;
};
static OwedPlan owed_plan(const bc_engine* e, bool use_log, bool table_untouched) {
  OwedPlan p;
  p.table = table_untouched && e->defer_reset ? kOwedSide : kOwedMain;
  p.bits = !use_log ? kOwedMain : (e->fold_fresh ? kOwedFresh : (e->defer_reset ? kOwedSide : kOwedMain));
  return p;
}

// A log-mode submit with something owed: the parts that owed_plan() sends aside on reset_stream, after everything
// queued on the engine's stream so far.  *join: the engine's stream has to wait for reset_join before the fold.
// Whatever cannot be forked is settled on the engine's stream instead.
static int fork_owed(bc_engine* e, const OwedPlan& plan, bool* join) {
  *join = false;
  const bool bits_stay_owed = plan.bits != kOwedSide;
  if (plan.table != kOwedSide && e->owed_table) return settle_owed(e);  // (not reached: launch_match settled it)
  if (!e->owed_table && (bits_stay_owed || !e->owed_bits)) return BC_OK;
  if (!e->reset_stream) {
    if (hipStreamCreateWithFlags(&e->reset_stream, hipStreamNonBlocking) != hipSuccess) e->reset_stream = nullptr;
    if (e->reset_stream && (hipEventCreateWithFlags(&e->reset_fork, hipEventDisableTiming) != hipSuccess ||
                            hipEventCreateWithFlags(&e->reset_join, hipEventDisableTiming) != hipSuccess)) {
      (void)hipStreamDestroy(e->reset_stream);
      e->reset_stream = nullptr;
    }
  }
  if (!e->reset_stream || hipEventRecord(e->reset_fork, e->stream) != hipSuccess ||
      hipStreamWaitEvent(e->reset_stream, e->reset_fork, 0) != hipSuccess) {
    (void)hipGetLastError();
    return settle_owed(e);
  }
  int rc = settle_table_on(e, e->reset_stream);
  if (rc == BC_OK && !bits_stay_owed) rc = settle_bits_on(e, e->reset_stream);
  // (joined whatever happened: what did get onto reset_stream must not run on beside a later writer)
  if (hipEventRecord(e->reset_join, e->reset_stream) != hipSuccess) {
    HIP_TRY(hipStreamSynchronize(e->reset_stream));
    return rc;
  }
  *join = true;
  return rc;
}

// Times one launch sequence when bc_engine_timing is on: created and recorded at construction (rc: how that went),
// done() records the end and hands the pair to e->events; a pair that was not handed over is destroyed.
struct LaunchTimer {
  bc_engine* e;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t rc = hipSuccess;
  explicit LaunchTimer(bc_engine* e_) : e(e_) {
    if (!e->timing) return;
    if ((rc = hipEventCreate(&e0)) == hipSuccess && (rc = hipEventCreate(&e1)) == hipSuccess) rc = hipEventRecord(e0, e->stream);
  }
  hipError_t done() {
    if (!e1) return hipSuccess;
    const hipError_t end = hipEventRecord(e1, e->stream);
    if (end == hipSuccess) {
      e->events.emplace_back(e0, e1);
      e0 = e1 = nullptr;
    }
    return end;
  }
  ~LaunchTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

static uint64_t slot_mask(const bc_engine* e) { return e->n_slots ? e->n_slots - 1 : 0; }

// the flags word of a match kernel, generic or specialised: `tables` and `hot` are that kernel's fields of the MatchShape
static uint32_t match_flags(const MatchShape& s, bool tables, bool hot) {
  return (s.pipe ? 1u : 0u) | (tables ? 2u : 0u) | (hot ? 4u : 0u);
}

// s: match_shape() of the batch; NW = s.generic_nw
template <int NW, int NWW>
static int launch_match(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens, uint32_t stride,
                        uint32_t read_len, uint32_t nd, uint64_t n_reads, uint8_t* trace_outcome, uint64_t* trace_idx,
                        const MatchShape& s) {
  // log mode (bc_fold.h): the batch goes through in chunks of at most log_chunk reads, each matched into the log and
  // folded before the next one overwrites it.  (The same code object with the hot-counter cache on or off: the kernel
  // lays out its LDS from the flag, so a launch without the cache does not ask for its bytes.)
  const bool use_log = log_mode_for(e, n_reads);
  const bool hot_on = !use_log || e->log_hot;
  const uint32_t lds = hot_on ? s.lds : s.lds_cold, lds_jit = hot_on ? s.lds_jit : s.lds_jit_cold;
  // In log mode the kernel reads and writes only the reads, the log and the outcome counters -- unless the hot-counter
  // cache flushes to the table or the plan's search queue adds to it directly (neither touches the bit map): what a
  // reset owes can then wait for the fold (owed_plan).  Everyone else settles first.
  const bool table_untouched = use_log && !hot_on && !e->h.plan.defer_search();
  const OwedPlan owed = owed_plan(e, use_log, table_untouched);
  if (owed.table == kOwedMain) {
    const int rc = settle_table_on(e, e->stream);
    if (rc != BC_OK) return rc;
  }
  if (owed.bits == kOwedMain) {
    const int rc = settle_bits_on(e, e->stream);
    if (rc != BC_OK) return rc;
  }
  const uint32_t flags = match_flags(s, s.tables_generic, s.hot_generic && hot_on);
  if (s.lds + 64 > e->lds_limit) {
    set_error("read stride too large for one LDS tile");
    return BC_ERR_UNSUPPORTED;
  }
  const bool wide = e->h.plan.wide != 0;  // (a sparse plan: no bit map, no log, no hot-counter cache)
  const void* kern = wide ? (const void*)match_count_wide_kernel<NW, NWW> : (const void*)match_count_kernel<NW, NWW>;
  if (s.lds > 48 * 1024) HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds));
  // persistent grid: as many workgroups as the chip holds at once (or fewer for a small batch), at the LDS this launch
  // asks for
  int per_cu = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kTPB, lds));
  if (per_cu < 1) per_cu = 1;
  const uint64_t resident = (uint64_t)per_cu * e->n_cus;
  const uint64_t blocks = std::min<uint64_t>((n_reads + kTPB - 1) / kTPB, resident);
  uint64_t blocks_jit = blocks, resident_jit = resident;
  LaunchTimer timer(e);
  HIP_TRY(timer.rc);
  hipFunction_t jit_fn = nullptr;
  e->reads_seen += n_reads;
  // (a log-mode specialised kernel numbers its tiles in 32 bits, bc_kernel.h tile_t: log_chunk is 2^27 reads at most)
  if (NW <= 8 && NWW <= 4 && e->jit_mode != 0) {  // reads up to 256 bases; longer ones stay on the generic kernel
    int per_cu_jit = 1;
    jit_fn = e->jit.function(e->h.plan, e->device, e->jit_mode, e->reads_seen, s, jit_variant(s, use_log, hot_on), &per_cu_jit);
    resident_jit = (uint64_t)per_cu_jit * e->n_cus;
    if (jit_fn) blocks_jit = std::min<uint64_t>((n_reads + kTPB - 1) / kTPB, resident_jit);
  }
  if (use_log) {
    const int rc = ensure_log(e, std::min<uint64_t>(n_reads, e->log_chunk));
    if (rc != BC_OK) return rc;
  }
  const uint64_t chunk = use_log ? e->log_chunk : n_reads;
  bool join = false;
  if (use_log) {
    const int rc = fork_owed(e, owed, &join);
    if (rc != BC_OK) {
      if (join) (void)hipStreamWaitEvent(e->stream, e->reset_join, 0);
      (void)settle_owed(e);
      return rc;
    }
  }
  // (an error below leaves through here: the side stream joined, and what is still owed stays owed for the next comer)
  struct JoinGuard {
    bc_engine* e;
    bool* join;
    ~JoinGuard() {
      if (*join) (void)hipStreamWaitEvent(e->stream, e->reset_join, 0);
    }
  } join_guard{e, &join};
  for (uint64_t c0 = 0; c0 < n_reads; c0 += chunk) {
    const uint64_t n_c = std::min<uint64_t>(chunk, n_reads - c0);
    const uint8_t* a_seq = (const uint8_t*)d_seq + c0 * stride;
    const uint8_t* a_qual = d_qual ? (const uint8_t*)d_qual + c0 * stride : nullptr;
    const uint16_t* a_lens = d_lens ? (const uint16_t*)d_lens + c0 : nullptr;
    const uint16_t* a_qlens = d_qlens ? (const uint16_t*)d_qlens + c0 : nullptr;
    uint8_t* a_to = trace_outcome ? trace_outcome + c0 : nullptr;
    uint64_t* a_ti = trace_idx ? trace_idx + c0 : nullptr;
    uint32_t* a_log = use_log ? e->d_log : nullptr;
    uint64_t a_n = n_c, a_smask = slot_mask(e);
    uint32_t a_region = s.region;
    if (jit_fn) {
      uint32_t a_flags = match_flags(s, s.tables_jit, s.hot_jit && hot_on);
      void* args[] = {&a_seq, &a_qual, &a_lens, &a_qlens, &stride, &read_len, &nd, &a_n, &a_region, &e->d_table, &e->d_bits, &e->d_slots,
                      &e->d_vals, &a_smask, &e->d_counters, &a_to, &a_ti, &a_flags, &a_log,
                      &e->d_ready};  // (the last one: the kernel of a wide-key plan only, bc_jit.hip jit_source)
      const uint64_t grid = std::min<uint64_t>(blocks_jit, (n_c + kTPB - 1) / kTPB);
      HIP_TRY(hipModuleLaunchKernel(jit_fn, (uint32_t)grid, 1, 1, kTPB, 1, 1, lds_jit, e->stream, args, nullptr));
    } else {
      const uint64_t grid = std::min<uint64_t>(blocks, (n_c + kTPB - 1) / kTPB);
      if (wide)
        hipLaunchKernelGGL((match_count_wide_kernel<NW, NWW>), dim3((uint32_t)grid), dim3(kTPB), lds, e->stream, e->d_plan, a_seq, a_qual,
                           a_lens, a_qlens, stride, read_len, nd, a_n, a_region, e->d_slots, e->d_vals, e->d_ready, a_smask,
                           e->d_counters, a_to, a_ti, flags);
      else
        hipLaunchKernelGGL((match_count_kernel<NW, NWW>), dim3((uint32_t)grid), dim3(kTPB), lds, e->stream, e->d_plan, a_seq, a_qual, a_lens,
                           a_qlens, stride, read_len, nd, a_n, a_region, e->d_table, e->d_bits, e->d_slots, e->d_vals, a_smask,
                           e->d_counters, a_to, a_ti, flags, a_log);
    }
    HIP_TRY(hipGetLastError());
    if (use_log) {
      if (join) {
        HIP_TRY(hipStreamWaitEvent(e->stream, e->reset_join, 0));
        join = false;
      }
      const bool fresh = e->owed_bits;  // (kOwedFresh, and only the first chunk after a reset)
      const int rc = fold_log(e, n_c, fresh);
      if (rc != BC_OK) return rc;  // (a fresh fold that failed: the map stays owed its zeros)
      e->owed_bits = false;
    }
  }
  if (e->d_bits) {
    e->bits_dirty = true;
    e->reads_since_fold += n_reads;
  }
  e->last_kernel = std::string(jit_fn ? "bc_jit_match_count<" : "match_count_kernel<") +
                   std::to_string(jit_fn ? s.jit.NW : NW) + "," + std::to_string(jit_fn ? s.jit.NWW : NWW) + ">";
  if (wide) e->wide_lane_reads += n_reads;
  e->last_key = jit_fn ? s.key : 0;
  e->last_lds = jit_fn ? lds_jit : lds;
  e->last_grid = (uint32_t)std::min<uint64_t>(jit_fn ? blocks_jit : blocks, (std::min<uint64_t>(chunk, n_reads) + kTPB - 1) / kTPB);
  e->last_resident = (uint32_t)(jit_fn ? resident_jit : resident);
  HIP_TRY(timer.done());
  return BC_OK;
}

// the wave-per-read plan on the device (once per engine)
static int ensure_long(bc_engine* e) {
  if (e->long_ready) return BC_OK;
  if (!e->long_lowered && !e->src_plan->lower_long(e->lh)) return BC_ERR_UNSUPPORTED;
  e->long_lowered = true;
  LongPlan& Q = e->lh.plan;
  int rc;
  if ((rc = upload(e, e->lh.const_pos.data(), e->lh.const_pos.size() * 4, &Q.const_pos_a))) return rc;
  if ((rc = upload(e, e->lh.const_chr.data(), e->lh.const_chr.size(), &Q.const_chr_a))) return rc;
  if ((rc = upload(e, e->lh.fmtn_pos.data(), e->lh.fmtn_pos.size() * 4, &Q.fmtn_pos_a))) return rc;
  for (uint32_t g = 0; g < Q.n_groups; ++g) {
    if (!Q.groups[g].n_refs) continue;
    if ((rc = upload(e, e->lh.ref_text[g].data(), e->lh.ref_text[g].size(), &Q.groups[g].ref_text_a))) return rc;
    if ((rc = upload(e, e->lh.ref_off[g].data(), e->lh.ref_off[g].size() * 4, &Q.groups[g].ref_off_a))) return rc;
  }
  HIP_TRY(hipMalloc((void**)&e->d_long, sizeof(LongPlan)));
  e->allocs.push_back(e->d_long);
  HIP_TRY(hipMemcpy(e->d_long, &Q, sizeof(LongPlan), hipMemcpyHostToDevice));
  e->long_ready = true;
  return BC_OK;
}

static int launch_long(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens,
                       uint32_t stride, uint32_t read_len, uint64_t n_reads, uint8_t* trace_outcome, uint64_t* trace_idx) {
  int rc = ensure_long(e);
  if (rc != BC_OK) return rc;
  if ((rc = settle_owed(e)) != BC_OK) return rc;
  LaunchTimer timer(e);
  HIP_TRY(timer.rc);
  // four wavefronts per workgroup, one read per wavefront and step; enough workgroups to fill the chip
  const uint64_t blocks = std::min<uint64_t>((n_reads + 3) / 4, (uint64_t)e->n_cus * 8);
  hipLaunchKernelGGL(long_match_kernel, dim3((uint32_t)blocks), dim3(256), 0, e->stream, e->d_long, (const uint8_t*)d_seq,
                     (const uint8_t*)d_qual, (const uint16_t*)d_lens, (const uint16_t*)d_qlens, stride, read_len, n_reads,
                     e->d_table, e->d_slots, e->d_vals, e->d_ready, slot_mask(e), e->d_counters,
                     trace_outcome, trace_idx);
  HIP_TRY(hipGetLastError());
  e->table_all_dirty = true;  // (this kernel adds to the table without flagging blocks)
  e->last_kernel = "long_match_kernel";
  e->reads_seen += n_reads;
  HIP_TRY(timer.done());
  return BC_OK;
}

uint32_t bc::grid_for(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + 255) / 256, 256ull * 32); }

void bc::fix_error_launch(const DevGroup& G, uint32_t q1, uint32_t q2, uint32_t qn, uint32_t qx, uint32_t* d_out) {
  hipLaunchKernelGGL(fix_error_kernel, dim3(1), dim3(64), 0, 0, G, q1, q2, qn, qx, d_out);
}

// what every submit checks first
static int submit_check(const bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, uint32_t stride, uint32_t read_len) {
  if (!d_seq || stride == 0) {
    set_error("submit: null sequence buffer or zero stride");
    return BC_ERR_INVALID;
  }
  if (e->h.plan.quality_on && !d_qual) {
    set_error("submit: the quality filter is on (--min-quality > 0) but no quality buffer was given");
    return BC_ERR_INVALID;
  }
  if (((uintptr_t)d_seq & 15) || ((uintptr_t)d_qual & 15)) {
    set_error("submit: buffers must be 16-byte aligned");
    return BC_ERR_INVALID;
  }
  const uint32_t maxlen = d_lens ? stride : read_len;
  if (maxlen > stride) {
    set_error("submit: read_len exceeds stride");
    return BC_ERR_INVALID;
  }
  return BC_OK;
}

int bc::submit_forward(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens, uint32_t stride,
                       uint32_t read_len, uint64_t n_reads, uint8_t* trace_outcome, uint64_t* trace_idx) {
  const uint32_t maxlen = d_lens ? stride : read_len;
  const uint32_t nd = (maxlen + 3) / 4;
  HIP_TRY(hipSetDevice(e->device));
  e->table_materialized = false;
  counts_changed(e);
  {
    const int rc = set_reserve(e, n_reads);
    if (rc != BC_OK) return rc;
  }
  // plans or reads beyond the lane-per-read kernel's widths: the wave-per-read kernel (bc_long.h)
  if (e->long_only || maxlen > 320u) return launch_long(e, d_seq, d_qual, d_lens, d_qlens, stride, read_len, n_reads, trace_outcome, trace_idx);
  MatchShape s = match_shape(e->h.plan, e->table_entries, stride, read_len, d_lens != nullptr, trace_outcome != nullptr,
                             e->lds_limit, e->pipe, e->qshare, e->lhash_mode);
  // With the quality filter on, the pipelined fetch keeps two tile regions per wave: from 315 bases on (four waves x
  // two regions of 64 x 315 bytes and their slack) they no longer fit the LDS.  Such a batch is fetched on demand
  // into one region per wave -- the path every partial tile takes -- instead of being refused.
  if (s.pipe && s.lds + 64 > e->lds_limit)
    s = match_shape(e->h.plan, e->table_entries, stride, read_len, d_lens != nullptr, trace_outcome != nullptr, e->lds_limit, false,
                    e->qshare, e->lhash_mode);
  const int nww = s.jit.NWW;  // words of candidate offsets: the exact count; the instantiations round it up
#define BC_LAUNCH(NW_, NWW_) \
  return launch_match<NW_, NWW_>(e, d_seq, d_qual, d_lens, d_qlens, stride, read_len, nd, n_reads, trace_outcome, trace_idx, s)
  if (s.generic_nw == 4) {
    if (nww <= 1) BC_LAUNCH(4, 1);
    if (nww <= 2) BC_LAUNCH(4, 2);
    BC_LAUNCH(4, 4);
  }
  if (s.generic_nw == 8) {
    if (nww <= 2) BC_LAUNCH(8, 2);
    if (nww <= 4) BC_LAUNCH(8, 4);
    BC_LAUNCH(8, 8);
  }
  if (nww <= 4) BC_LAUNCH(10, 4);  // (up to 320 bases: longer reads went to the wave-per-read kernel)
  BC_LAUNCH(10, 10);
#undef BC_LAUNCH
}

// A plan's strand setting decides here, once, who counts the batch: as it stands (the engine's only path until a plan
// asks otherwise), or through bc_strand.hip.
static int submit_device_impl(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens, uint32_t stride,
                              uint32_t read_len, uint64_t n_reads, uint64_t trace_off) {
  if (n_reads == 0) return BC_OK;
  const int rc = submit_check(e, d_seq, d_qual, d_lens, stride, read_len);
  if (rc != BC_OK) return rc;
  if (e->strand != BC_STRAND_FORWARD) return submit_strand(e, d_seq, d_qual, d_lens, d_qlens, stride, read_len, n_reads, trace_off);
  return submit_forward(e, d_seq, d_qual, d_lens, d_qlens, stride, read_len, n_reads,
                        e->trace_outcome ? e->trace_outcome + trace_off : nullptr, e->trace_idx ? e->trace_idx + trace_off : nullptr);
}

extern "C" {

bc_engine* bc_engine_create(const bc_plan* p, int device_id, void* hip_stream, void* table_mem) {
  if (!p) {
    set_error("bc_engine_create: null plan");
    return nullptr;
  }
  bc_engine* e = new bc_engine();
  const int rc = engine_init(e, p, device_id, hip_stream, table_mem);
  if (rc != BC_OK) {
    const std::string msg = get_error();
    engine_free(e);
    set_error(msg);
    return nullptr;
  }
  return e;
}

void bc_engine_destroy(bc_engine* e) { engine_free(e); }

int bc_engine_submit_device(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, uint32_t stride,
                            uint32_t read_len, uint64_t n_reads) {
  return submit_device_impl(e, d_seq, d_qual, d_lens, nullptr, stride, read_len, n_reads, 0);
}

int bc_engine_submit_device_q(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens,
                              uint32_t stride, uint64_t n_reads) {
  if (!d_lens || !d_qlens) {
    set_error("bc_engine_submit_device_q: both length arrays are required");
    return BC_ERR_INVALID;
  }
  return submit_device_impl(e, d_seq, d_qual, d_lens, d_qlens, stride, stride, n_reads, 0);
}

void* bc_engine_hip_stream(bc_engine* e) { return (void*)e->stream; }
int bc_engine_device(const bc_engine* e) { return e->device; }
uint32_t bc_engine_key_words(const bc_engine* e) { return e->key_words; }
const bc_plan* bc_engine_plan(const bc_engine* e) { return e->src_plan; }

}  // extern "C"

// staging copy pageable -> pinned, cut into slices for a few threads: one core moves ~10 GB/s, the link takes ~50
void bc::staged_copy(void* dst, const void* src, size_t n) {
  static const int threads = []() {
    const char* t = getenv("BC_STAGE_THREADS");
    const int v = t ? atoi(t) : 4;
    return v < 1 ? 1 : (v > 16 ? 16 : v);
  }();
  if (threads == 1 || n < (8u << 20)) {
    memcpy(dst, src, n);
    return;
  }
  const size_t slice = ((n / threads) + 4095) & ~(size_t)4095;
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; ++t) {
    const size_t off = (size_t)t * slice;
    if (off >= n) break;
    const size_t len = std::min(slice, n - off);
    pool.emplace_back([=]() { memcpy((uint8_t*)dst + off, (const uint8_t*)src + off, len); });
  }
  memcpy(dst, src, std::min(slice, n));
  for (auto& th : pool) th.join();
}

extern "C" {

int bc_engine_submit_host(bc_engine* e, const void* seq, const void* qual, const uint16_t* lens, uint32_t stride,
                          uint32_t read_len, uint64_t n_reads) {
  if (n_reads == 0) return BC_OK;
  if (!seq || stride == 0) {
    set_error("submit: null sequence buffer or zero stride");
    return BC_ERR_INVALID;
  }
  const bool with_qual = e->h.plan.quality_on != 0;
  if (with_qual && !qual) {
    set_error("submit: the quality filter is on (--min-quality > 0) but no quality buffer was given");
    return BC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(e->device));
  // chunk = a multiple of 256 reads so that every chunk's arrays stay 16-byte aligned
  const uint64_t chunk = std::max<uint64_t>(256, ((64ull << 20) / (stride * (with_qual ? 2 : 1) + 2)) & ~255ull);
  const size_t seq_bytes = (size_t)chunk * stride;
  const size_t need = seq_bytes * (with_qual ? 2 : 1) + chunk * 2 + 64;
  if (e->stage_bytes < need) {
    for (int s = 0; s < bc_engine::kStages; ++s) {
      if (e->pin[s]) (void)hipHostFree(e->pin[s]);
      if (e->dev[s]) (void)hipFree(e->dev[s]);
      e->pin[s] = nullptr;
      e->dev[s] = nullptr;
      HIP_TRY(hipHostMalloc((void**)&e->pin[s], need, hipHostMallocDefault));
      HIP_TRY(hipMalloc((void**)&e->dev[s], need));
      if (!e->copied[s]) HIP_TRY(hipEventCreateWithFlags(&e->copied[s], hipEventDisableTiming));
      if (!e->consumed[s]) HIP_TRY(hipEventCreateWithFlags(&e->consumed[s], hipEventDisableTiming));
      HIP_TRY(hipEventRecord(e->consumed[s], e->stream));
    }
    e->stage_bytes = need;
  }
  uint64_t done = 0;
  int s = 0;
  while (done < n_reads) {
    const uint64_t n = std::min(chunk, n_reads - done);
    // the pinned buffer is free once its previous H2D copy is done, the device buffer once the
    // kernel that read it has finished
    HIP_TRY(hipEventSynchronize(e->copied[s]));
    uint8_t* hp = e->pin[s];
    const size_t sb = (size_t)n * stride;
    const size_t q_off = with_qual ? ((sb + 15) & ~(size_t)15) : 0;
    const size_t l_off = q_off + (with_qual ? ((sb + 15) & ~(size_t)15) : ((sb + 15) & ~(size_t)15));
    staged_copy(hp, (const uint8_t*)seq + done * stride, sb);
    if (with_qual) staged_copy(hp + q_off, (const uint8_t*)qual + done * stride, sb);
    if (lens) memcpy(hp + l_off, lens + done, n * 2);
    const size_t total = l_off + (lens ? n * 2 : 0);
    HIP_TRY(hipStreamWaitEvent(e->copy_stream, e->consumed[s], 0));
    HIP_TRY(hipMemcpyAsync(e->dev[s], hp, total, hipMemcpyHostToDevice, e->copy_stream));
    HIP_TRY(hipEventRecord(e->copied[s], e->copy_stream));
    HIP_TRY(hipStreamWaitEvent(e->stream, e->copied[s], 0));
    const int rc = submit_device_impl(e, e->dev[s], with_qual ? e->dev[s] + q_off : nullptr,
                                      lens ? e->dev[s] + l_off : nullptr, nullptr, stride, read_len, n, done);
    if (rc != BC_OK) return rc;
    HIP_TRY(hipEventRecord(e->consumed[s], e->stream));
    done += n;
    s ^= 1;
  }
  // the caller may reuse its buffers on return: they were copied into pinned memory above
  return BC_OK;
}

// two-level counting: the bits into the table, the map cleared (enqueued on the engine's stream)
static int fold_bits(bc_engine* e) {
  const int owed_rc = settle_owed(e);
  if (owed_rc != BC_OK) return owed_rc;
  if (!e->bits_dirty) return BC_OK;
  // few bits (under one in sixteen entries): one lane per word of the map, a table access per set bit; many: a
  // streaming pass over the table
  if (e->reads_since_fold * 16 < e->table_entries || ((uintptr_t)e->d_table & 15))
    hipLaunchKernelGGL(fold_bits_kernel, dim3(grid_for(e->n_bit_words)), dim3(256), 0, e->stream, e->d_bits, e->n_bit_words,
                       e->d_table, e->table_entries);
  else
    hipLaunchKernelGGL(fold_bits_dense_kernel, dim3(256 * 32), dim3(256), 0, e->stream, e->d_bits, e->n_bit_words,
                       reinterpret_cast<uint4*>(e->d_table), e->table_entries);
  HIP_TRY(hipGetLastError());
  e->bits_dirty = false;
  e->reads_since_fold = 0;
  e->table_all_dirty = true;  // (the fold adds to the table without flagging blocks)
  return BC_OK;
}

int bc_engine_sync(bc_engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  {
    const int rc = settle_owed(e);  // (reset(); sync() costs and means what it always did)
    if (rc != BC_OK) return rc;
  }
  // Two-level counting: a table somebody else can see -- caller-owned memory, or an engine-owned table whose pointer
  // has been handed out (bc_engine_table_ptr) -- holds the whole counts from here on; an engine-owned one nobody has
  // asked for keeps its bits apart: bc_engine_finish reads bits and table as they stand.
  if (e->bits_dirty && (!e->own_table || e->table_exposed)) {
    const int rc = fold_bits(e);
    if (rc != BC_OK) return rc;
  }
  HIP_TRY(hipStreamSynchronize(e->copy_stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BC_OK;
}


static int reset_impl(bc_engine* e, bool counters_too);
int bc_engine_reset(bc_engine* e) { return reset_impl(e, true); }
int bc_engine_reset_results(bc_engine* e) { return reset_impl(e, false); }
static int reset_impl(bc_engine* e, bool counters_too) {
  HIP_TRY(hipSetDevice(e->device));
  counts_changed(e);
  // what an earlier reset still owes goes first: its dirty-block pass is what makes the flags mean what they say
  {
    const int rc = settle_owed(e);
    if (rc != BC_OK) return rc;
  }
  // Nothing is zeroed here: the reset is recorded as owed (bc_engine::owed_*) and paid by whoever needs it.  With a
  // dirty-block map whose flags can be trusted the table's part is the dirty-block pass (sparse_reset_kernel), otherwise
  // table and flags are zeroed whole; the bit map is zeroed either way.
  const uint64_t dirty_off = e->h.plan.dirty_off;
  e->owed_table = e->d_table != nullptr;
  e->owed_table_all = !(e->d_bits && dirty_off && !e->table_all_dirty);
  e->owed_bits = e->d_bits != nullptr;
  if (e->owed_table_all) e->table_all_dirty = !e->own_table || e->table_exposed;  // (whoever holds the pointer may write it again)
  if (!e->own_table || e->table_exposed) {
    // a table somebody else can see: they may order their own work after the reset by the stream alone
    const int rc = settle_table_on(e, e->stream);
    if (rc != BC_OK) return rc;
  }
  e->bits_dirty = false;
  e->reads_since_fold = 0;
  if (counters_too) HIP_TRY(hipMemsetAsync(e->d_counters, 0, BC_NCOUNTERS * 8, e->stream));
  return clear_key_table(e);
}

int bc_engine_counters(bc_engine* e, uint64_t out[BC_NCOUNTERS]) {
  int rc = bc_engine_sync(e);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out, e->d_counters, BC_NCOUNTERS * 8, hipMemcpyDeviceToHost));
  return BC_OK;
}

void* bc_engine_table_ptr(bc_engine* e) {
  // whoever takes the pointer wants plain u32 counts behind it, now and after every later bc_engine_sync (two-level
  // counting: fold what is pending, and wait; from here on every sync folds)
  if (hipSetDevice(e->device) != hipSuccess || settle_owed(e) != BC_OK) {
    set_error(std::string("bc_engine_table_ptr: the pending reset of the table could not be run: ") + get_error());
    return nullptr;
  }
  e->table_exposed = true;
  e->table_all_dirty = true;
  if (e->bits_dirty && hipSetDevice(e->device) == hipSuccess && fold_bits(e) == BC_OK) (void)hipStreamSynchronize(e->stream);
  return e->d_table;
}
// (not part of the documented ABI) the table as plain u32 counts for the engine library's own end-of-run exchange
// (bc_comm.hip): folded like bc_engine_table_ptr, but the pointer does not outlive the call that asked for it, so the
// table is not marked as exposed for good -- only the next reset has to zero all of it (the exchange writes the sum
// into the root's table without flagging blocks).
void* bc_internal_table_folded(bc_engine* e) {
  if (hipSetDevice(e->device) != hipSuccess || settle_owed(e) != BC_OK) {
    set_error(std::string("the pending reset of the table could not be run: ") + get_error());
    return nullptr;
  }
  if (e->bits_dirty && hipSetDevice(e->device) == hipSuccess && fold_bits(e) == BC_OK) (void)hipStreamSynchronize(e->stream);
  e->table_all_dirty = true;
  counts_changed(e);
  return e->d_table;
}
// ... or as it stands, with the bit map beside it (*bits: NULL when nothing is pending there): the exchange packs
// table + bit itself.  The caller says when the table has been overwritten with plain counts (the root: the job's sum).
void* bc_internal_table_unfolded(bc_engine* e, const void** bits) {
  *bits = nullptr;
  if (hipSetDevice(e->device) != hipSuccess || settle_owed(e) != BC_OK) {
    set_error(std::string("the pending reset of the table could not be run: ") + get_error());
    return nullptr;
  }
  *bits = e->bits_dirty ? e->d_bits : nullptr;
  e->table_all_dirty = true;
  counts_changed(e);
  return e->d_table;
}
int bc_internal_table_now_plain(bc_engine* e) {
  counts_changed(e);  // (the exchange has written the job's sum into the table)
  {
    const int rc = settle_owed(e);
    if (rc != BC_OK) return rc;
  }
  if (e->d_bits) HIP_TRY(hipMemsetAsync(e->d_bits, 0, e->n_bit_words * 4, e->stream));
  e->bits_dirty = false;
  e->reads_since_fold = 0;
  return BC_OK;
}
void* bc_engine_counters_ptr(bc_engine* e) { return e->d_counters; }
uint64_t bc_engine_table_entries(const bc_engine* e) { return e->table_entries; }

int bc_engine_trace(bc_engine* e, void* d_outcome_u8, void* d_index_u64) {
  e->trace_outcome = (uint8_t*)d_outcome_u8;
  e->trace_idx = (uint64_t*)d_index_u64;
  return BC_OK;
}

}  // extern "C"

extern "C" {

int bc_engine_timing(bc_engine* e, int enable) {
  e->timing = enable != 0;
  return BC_OK;
}

const char* bc_engine_kernel_name(bc_engine* e) { return e ? e->last_kernel.c_str() : ""; }

// test hook (not part of the documented ABI): the engine's last match launch -- the specialised kernel's shape key (0 when
// the generic kernel ran), the dynamic LDS it asked for, its grid, and the workgroups the device holds of it at once
int bc_internal_last_launch(const bc_engine* e, uint64_t* key, uint32_t* lds_bytes, uint32_t* grid, uint32_t* resident) {
  *key = e->last_key;
  *lds_bytes = e->last_lds;
  *grid = e->last_grid;
  *resident = e->last_resident;
  return BC_OK;
}

int bc_engine_count_log_folds(const bc_engine* e, uint64_t* n) {
  *n = e->log_folds;
  return BC_OK;
}

int bc_engine_wide_lane_reads(const bc_engine* e, uint64_t* n) {
  *n = e->wide_lane_reads;
  return BC_OK;
}

int bc_engine_gz_blocks_inflated(const bc_engine* e, uint64_t* n) {
  *n = e->gz_blocks;
  return BC_OK;
}

int bc_engine_gz_segments_inflated(const bc_engine* e, uint64_t* n) {
  *n = e->gz_segments;
  return BC_OK;
}

// resolves the recorded event pairs into per-launch times (the stream has drained)
static int collect_launch_times(bc_engine* e) {
  int rc = bc_engine_sync(e);
  if (rc) return rc;
  for (auto& ev : e->events) {
    float ms = 0.f;
    const hipError_t he = hipEventElapsedTime(&ms, ev.first, ev.second);
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
    if (he == hipSuccess) e->launch_ms.push_back(ms);
  }
  e->events.clear();
  return BC_OK;
}

int bc_engine_kernel_ms(bc_engine* e, double* total_ms, uint64_t* launches) {
  const int rc = collect_launch_times(e);
  if (rc) return rc;
  double total = 0.0;
  for (float ms : e->launch_ms) total += ms;
  if (total_ms) *total_ms = total;
  if (launches) *launches = e->launch_ms.size();
  e->launch_ms.clear();
  return BC_OK;
}

int bc_engine_kernel_ms_each(bc_engine* e, double* ms_out, uint64_t capacity, uint64_t* launches) {
  const int rc = collect_launch_times(e);
  if (rc) return rc;
  if (launches) *launches = e->launch_ms.size();
  for (uint64_t i = 0; ms_out && i < capacity && i < e->launch_ms.size(); ++i) ms_out[i] = e->launch_ms[i];
  return BC_OK;
}

}  // extern "C"

// the ingest path's count of BGZF blocks inflated for this engine (bc_bgzf.hpp)
namespace bc {
void engine_add_gz_blocks(bc_engine* e, uint64_t n) { e->gz_blocks += n; }
void engine_add_gz_segments(bc_engine* e, uint64_t n) { e->gz_segments += n; }
}  // namespace bc
