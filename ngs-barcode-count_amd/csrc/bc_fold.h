// Log-mode counting (bc_kernel.h, match_count_body with `count_log`): the fold of a count log into the two-level
// counters (first-occurrence bit map + table).
//
// The match kernel leaves one u32 per read: the read's dense tuple index, or kLogNone.  Four kernels then apply it:
//   bc_fold_hist     entries per bucket (a bucket = 2^22 tuples = 512 KB of bit map; at most 1024 buckets)
//   bc_fold_scan     bucket starts, and the fold's work items (bucket x chunk of entries)
//   bc_fold_scatter  the log grouped by bucket: 16384-entry tiles sorted in LDS, then written out as runs
//                    (the tile held in registers meanwhile, the next tile's loads in flight)
//   bc_fold_apply    per item and quarter of its bucket (one such unit per workgroup and step, the four of an item on
//                    four workgroups of one XCD at one time: fold_apply_unit): 128 KB of bit map into LDS, one LDS
//                    atomicOr per entry (a bit that was set already makes the entry a table add), the quarter written back
// A tuple with c entries ends as the atomic path would leave it: bit clear before -> bit set and table + c - 1; bit set
// before -> table + c.  A bucket with more than kFoldChunk entries (a hot library) is split over several items, which
// then meet on the same quarter: there the first entry of a tuple in an item also sets its bit in memory, with a
// returning atomicOr, and a bit another item had set meanwhile was not a first occurrence after all (table + 1).
// Exactly one of them sets each bit; only the sole item of a bucket writes its quarters back whole.
// Neither kernel waits for one memory access at a time: loads go out as 16-byte groups, several together and ahead of
// their use, and a thread's LDS atomics are issued back to back with one wait behind them.  log and grouped are
// therefore 16-byte aligned (fold_launch refuses others), and no load reaches past the 16-byte group that holds the
// last entry of the log or of an item.
//
// A fold onto a map that is known to be all zero but has not been written so (`fresh`: the engine's first fold after a
// reset, bc_engine.hip) reads none of it: the sole item of a bucket starts its quarters from zeroed LDS and writes them
// back whole as ever, and bc_fold_zero_unowned, between scan and apply, writes zeros over the buckets that have no sole
// item -- the empty ones, and the split ones, whose items meet in memory.  Every word of the map is defined afterwards.
#pragma once

#include "bc_intrin.h"

namespace bc {

constexpr uint32_t kFoldTPB = 1024;
constexpr uint32_t kFoldBucketShift = 22;   // tuples per bucket: 2^22
constexpr uint32_t kFoldQuarterShift = 20;  // tuples per apply pass: 2^20 (32768 bit-map words, 128 KB of LDS)
constexpr uint32_t kFoldQuarters = 1u << (kFoldBucketShift - kFoldQuarterShift);
constexpr uint32_t kFoldMaxBuckets = 1024;  // indexes below 2^32
constexpr uint32_t kFoldTile = 16384;       // bc_fold_scatter: entries per LDS tile (two workgroups per CU)
constexpr uint32_t kFoldChunk = 1u << 18;   // entries per apply item at most
constexpr uint32_t kFoldQuarterWords = 1u << (kFoldQuarterShift - 5);
constexpr uint32_t kFoldSpare = 64;          // bc_fold_scatter: bins behind the buckets' for kLogNone entries, one per lane
constexpr uint32_t kFoldScatterLds = kFoldTile * 4u + (3u * kFoldMaxBuckets + 2u * kFoldSpare) * 4u;
constexpr uint32_t kFoldApplyLds = kFoldQuarterWords * 4u;
constexpr uint32_t kFoldXcds = 8;            // bc_fold_apply: workgroups b and b + 8 are observed to share an L2

// bc_fold_apply's unit of work is one quarter of one item's bucket; a workgroup walks the units of step 0, 1, ... until
// one is not valid (the items of a workgroup rise with the step).  Over the blocks of a grid and their steps every
// (item < n_items, quarter < kFoldQuarters) comes up exactly once, for every grid >= 1.  A grid that is a multiple of
// 32 puts the four quarters of an item on blocks 8 apart, which are observed to be dealt to one XCD, and in the same
// step.  The intent is that the four read the item's entries at about the same time, so that one reading comes from
// HBM and three can be served by that XCD's L2 (what the counters say of it: DESIGN.md 8).  That is a matter of speed
// alone: the four exchange nothing and write disjoint quarters.
struct FoldUnit {
  uint32_t item, quarter;
  bool valid;
};
BC_HD FoldUnit fold_apply_unit(uint32_t block, uint32_t grid, uint32_t step, uint32_t n_items) {
  uint64_t item;
  uint32_t quarter;
  if (grid % (kFoldXcds * kFoldQuarters) == 0u) {
    const uint32_t xcd = block % kFoldXcds, slot = block / kFoldXcds;
    quarter = slot % kFoldQuarters;
    item = (uint64_t)(slot / kFoldQuarters) * kFoldXcds + xcd + (uint64_t)step * (grid / kFoldQuarters);
  } else {
    const uint64_t u = block + (uint64_t)step * grid;
    quarter = (uint32_t)(u % kFoldQuarters);
    item = u / kFoldQuarters;
  }
  FoldUnit r;
  r.valid = item < n_items;
  r.item = r.valid ? (uint32_t)item : 0u;
  r.quarter = quarter;
  return r;
}

#if defined(__HIPCC__)

// A workgroup barrier that orders LDS alone: loads, stores and atomics to global memory that are in flight stay in
// flight across it (__syncthreads waits for them).  Scatter and apply place every wait for memory themselves: both
// request entries well ahead of their use.
__device__ __forceinline__ void fold_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// exclusive prefix sum over the 1024 threads of a workgroup; tmp: 16 words of LDS.  Returns the total in `total`.
__device__ __forceinline__ uint32_t fold_block_scan(uint32_t v, uint32_t* tmp, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63u) tmp[wave] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < kFoldTPB / 64u; ++w) {
    const uint32_t t = tmp[w];
    before += w < wave ? t : 0u;
    all += t;
  }
  __syncthreads();
  total = all;
  return before + x - v;
}

__global__ __launch_bounds__(kFoldTPB) void bc_fold_hist(const uint32_t* __restrict__ log, uint64_t n, uint32_t nb,
                                                        uint32_t* __restrict__ cnt) {
  __shared__ uint32_t h[kFoldMaxBuckets];
  for (uint32_t i = threadIdx.x; i < nb; i += kFoldTPB) h[i] = 0;
  __syncthreads();
  const uint64_t n4 = n / 4u, step = (uint64_t)gridDim.x * kFoldTPB;
  const uint4* log4 = reinterpret_cast<const uint4*>(log);
  for (uint64_t i = (uint64_t)blockIdx.x * kFoldTPB + threadIdx.x; i < n4; i += step) {
    const uint4 v = log4[i];
    if (v.x != kLogNone) atomicAdd(&h[v.x >> kFoldBucketShift], 1u);
    if (v.y != kLogNone) atomicAdd(&h[v.y >> kFoldBucketShift], 1u);
    if (v.z != kLogNone) atomicAdd(&h[v.z >> kFoldBucketShift], 1u);
    if (v.w != kLogNone) atomicAdd(&h[v.w >> kFoldBucketShift], 1u);
  }
  if (blockIdx.x == 0 && threadIdx.x < (uint32_t)(n & 3u)) {
    const uint32_t v = log[n4 * 4u + threadIdx.x];
    if (v != kLogNone) atomicAdd(&h[v >> kFoldBucketShift], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nb; i += kFoldTPB)
    if (h[i]) atomicAdd(&cnt[i], h[i]);
}

// one workgroup: start[0..nb] (bucket starts in the grouped log), cursor[b] = start[b], item_off[0..nb] (first apply
// item of every bucket; item_off[nb] = the number of items); cnt is left zeroed for the next fold
__global__ __launch_bounds__(kFoldTPB) void bc_fold_scan(uint32_t* __restrict__ cnt, uint32_t nb, uint32_t* __restrict__ start,
                                                        uint32_t* __restrict__ cursor, uint32_t* __restrict__ item_off) {
  __shared__ uint32_t tmp[kFoldTPB / 64u];
  const uint32_t b = threadIdx.x;
  const uint32_t c = b < nb ? cnt[b] : 0u;
  const uint32_t items = (c + kFoldChunk - 1u) / kFoldChunk;
  uint32_t total_c, total_i;
  const uint32_t s = fold_block_scan(c, tmp, total_c);
  const uint32_t it = fold_block_scan(items, tmp, total_i);
  if (b < nb) {
    start[b] = s;
    cursor[b] = s;
    item_off[b] = it;
    cnt[b] = 0u;
  }
  if (b == 0) {
    start[nb] = total_c;
    item_off[nb] = total_i;
  }
}

// A tile's entries are read once, as four 16-byte loads per thread that are all in flight together, and stay in
// registers from the ranking to the placement; the loads of the workgroup's next tile are requested before the current
// tile is written out.  Every tile but the last takes the loads without a bounds test; in the last, what lies past n
// counts as kLogNone (no load reaches beyond the 16-byte group of the log's last entry: the log is 16-byte aligned).
// A kLogNone entry takes its rank from a spare bin and is placed on that bin, so neither pass branches around its
// LDS operation and the sixteen of a thread are issued back to back.
__global__ __launch_bounds__(kFoldTPB) void bc_fold_scatter(const uint32_t* __restrict__ log, uint64_t n, uint32_t nb,
                                                           uint32_t* __restrict__ cursor, uint32_t* __restrict__ out) {
  extern __shared__ uint32_t fold_smem[];
  uint32_t* sorted = fold_smem;
  uint32_t* h = sorted + kFoldTile;
  uint32_t* lstart = h + kFoldMaxBuckets + kFoldSpare;
  uint32_t* base = lstart + kFoldMaxBuckets + kFoldSpare;
  __shared__ uint32_t tmp[kFoldTPB / 64u];
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t kPer = kFoldTile / kFoldTPB, kPer4 = kPer / 4u;
  const uint64_t n_tiles = (n + kFoldTile - 1u) / kFoldTile, n_full = n / kFoldTile;
  const uint4* log4 = reinterpret_cast<const uint4*>(log);
  const uint32_t spare = kFoldMaxBuckets + (tid & (kFoldSpare - 1u));  // one per lane: no two lanes of a wave meet there
  uint32_t x[kPer];
  auto request = [&](uint64_t t) {
    const uint4* p = log4 + t * (kFoldTile / 4u) + tid;
    if (t < n_full) {
#pragma unroll
      for (uint32_t k = 0; k < kPer4; ++k) {
        const uint4 v = p[k * kFoldTPB];
        x[4 * k + 0] = v.x, x[4 * k + 1] = v.y, x[4 * k + 2] = v.z, x[4 * k + 3] = v.w;
      }
    } else {
      const uint32_t n_t = (uint32_t)(n - t * kFoldTile);
#pragma unroll
      for (uint32_t k = 0; k < kPer4; ++k) {
        const uint32_t e = (k * kFoldTPB + tid) * 4u;
        const uint4 v = e < n_t ? p[k * kFoldTPB] : make_uint4(kLogNone, kLogNone, kLogNone, kLogNone);
        x[4 * k + 0] = e + 0u < n_t ? v.x : kLogNone;
        x[4 * k + 1] = e + 1u < n_t ? v.y : kLogNone;
        x[4 * k + 2] = e + 2u < n_t ? v.z : kLogNone;
        x[4 * k + 3] = e + 3u < n_t ? v.w : kLogNone;
      }
    }
  };
  uint64_t t = blockIdx.x;
  if (t < n_tiles) request(t);
  // the run of a spare bin is the bin itself (h follows sorted): where the placement puts a kLogNone entry
  if (tid < kFoldSpare) lstart[kFoldMaxBuckets + tid] = kFoldTile + kFoldMaxBuckets + tid;
  for (; t < n_tiles; t += gridDim.x) {
    // (the last tile's write-out reads none of h, so no barrier stands between it and these stores)
    for (uint32_t i = tid; i < kFoldMaxBuckets + kFoldSpare; i += kFoldTPB) h[i] = 0;
    fold_lds_barrier();
    // the entries' ranks within their bucket, two per register (below 2^15)
    uint32_t r[kPer / 2];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t rk = atomicAdd(&h[x[k] != kLogNone ? x[k] >> kFoldBucketShift : spare], 1u);  // (a load-free select)
      if (k & 1u) r[k / 2] |= rk << 16; else r[k / 2] = rk;
    }
    fold_lds_barrier();
    // one bucket per thread (nb <= 1024): the tile's runs, and their places in the grouped log
    const uint32_t hc = tid < nb ? h[tid] : 0u;
    uint32_t valid;
    const uint32_t ls = fold_block_scan(hc, tmp, valid);
    uint32_t reserved = 0;
    if (tid < nb) {
      lstart[tid] = ls;
      if (hc) reserved = atomicAdd(&cursor[tid], hc);
    }
    fold_lds_barrier();
    // the placement needs lstart alone: the reservation is in flight beside it.  Eight runs are read before the eight
    // entries go to their places (reads and writes of the one LDS array are not reordered by the compiler)
#pragma unroll
    for (uint32_t k0 = 0; k0 < kPer; k0 += 8u) {
      uint32_t at[8];
#pragma unroll
      for (uint32_t k = k0; k < k0 + 8u; ++k) {
        const uint32_t rk = (r[k / 2] >> (16u * (k & 1u))) & 0xFFFFu;
        const bool some = x[k] != kLogNone;
        at[k - k0] = lstart[some ? x[k] >> kFoldBucketShift : spare] + (some ? rk : 0u);
      }
#pragma unroll
      for (uint32_t k = k0; k < k0 + 8u; ++k) sorted[at[k - k0]] = x[k];
    }
    if (tid < nb && hc) base[tid] = reserved;
    if (t + gridDim.x < n_tiles) request(t + gridDim.x);
    fold_lds_barrier();
    // sixteen entries per thread again, without a branch around their LDS reads: a thread whose place lies past the
    // tile's last valid entry writes that entry once more (the same word to the same place)
    if (valid) {
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t i = k * kFoldTPB + tid < valid ? k * kFoldTPB + tid : valid - 1u;
        const uint32_t v = sorted[i];
        const uint32_t bk = v >> kFoldBucketShift;
        out[base[bk] + (i - lstart[bk])] = v;
      }
    }
  }
}

// a fresh fold: zeroes the bit-map words (clipped to n_words) of every bucket that does not have exactly one apply item;
// one (bucket, quarter) per workgroup and step
__global__ __launch_bounds__(kFoldTPB) void bc_fold_zero_unowned(uint32_t nb, const uint32_t* __restrict__ item_off,
                                                                uint32_t* __restrict__ bits, uint64_t n_words) {
  constexpr uint32_t kPer = kFoldQuarterWords / 4u / kFoldTPB;
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (uint32_t p = blockIdx.x; p < nb * kFoldQuarters; p += gridDim.x) {
    const uint32_t b = p / kFoldQuarters, quarter = p % kFoldQuarters;
    if (item_off[b + 1] - item_off[b] == 1u) continue;
    const uint64_t w0 = ((uint64_t)b << (kFoldBucketShift - 5)) + (uint64_t)quarter * kFoldQuarterWords;
    if (w0 >= n_words) continue;
    const uint64_t nw = n_words - w0 < kFoldQuarterWords ? n_words - w0 : kFoldQuarterWords;
    uint32_t* gw = bits + w0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t w = (k * kFoldTPB + threadIdx.x) * 4u;
      if (w + 4u <= nw) {
        reinterpret_cast<uint4*>(gw)[w / 4u] = zero;
      } else {
        if (w + 0u < nw) gw[w + 0u] = 0u;
        if (w + 1u < nw) gw[w + 1u] = 0u;
        if (w + 2u < nw) gw[w + 2u] = 0u;
      }
    }
  }
}

// n_words: bit-map words in use (ceil(entries / 32)); dirty: the table's dirty-block map, or null; fresh: the map counts
// as all zero whatever memory holds (the owner of a bucket does not load it; bc_fold_zero_unowned has run).
// A workgroup works on one unit at a time, a quarter of an item's bucket (fold_apply_unit), and reads the item's entries
// for it; the units of the other quarters read the same entries elsewhere, in the same step of their workgroups.
// The entries arrive in batches of sixteen per thread, and a batch is requested before the one ahead of it is
// processed: the next batch of the unit, else the first batch of the workgroup's next unit -- neither of which depends
// on what LDS holds, so they stay in flight across the barriers (fold_lds_barrier).  Every request is clipped to its
// item.
__global__ __launch_bounds__(kFoldTPB) void bc_fold_apply(const uint32_t* __restrict__ grouped, uint32_t nb,
                                                         const uint32_t* __restrict__ start, const uint32_t* __restrict__ item_off,
                                                         uint32_t* __restrict__ bits, uint64_t n_words, uint32_t* __restrict__ table,
                                                         uint8_t* __restrict__ dirty, uint32_t fresh) {
  static_assert(kFoldMaxBuckets <= kFoldTPB, "one bucket per thread");
  extern __shared__ uint32_t fold_smem[];
  uint4* q4 = reinterpret_cast<uint4*>(fold_smem);
  // the item of the unit in turn and of the workgroup's next one: bucket, sole item of its bucket, first entry, end of its entries
  __shared__ uint32_t s_item[2][4];
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t kPer = kFoldQuarterWords / 4u / kFoldTPB;  // uint4 per thread
  constexpr uint32_t kIn4 = 4;                                   // 16-byte loads per thread and batch
  constexpr uint32_t kBatch = kIn4 * 4u * kFoldTPB;
  const uint4 none4 = make_uint4(kLogNone, kLogNone, kLogNone, kLogNone);
  const uint32_t n_items = item_off[nb];
  FoldUnit u = fold_apply_unit(blockIdx.x, gridDim.x, 0u, n_items);
  if (!u.valid) return;
  auto add = [&](uint32_t idx) {
    table_add(&table[idx]);
    if (dirty) dirty[idx >> 6] = (uint8_t)1;
  };
  // one bucket per thread: the thread whose bucket holds an item says so (a bucket without items holds none)
  uint32_t my_it0 = 0, my_it1 = 0, my_e0 = 0, my_e1 = 0;
  if (tid < nb) my_it0 = item_off[tid], my_it1 = item_off[tid + 1], my_e0 = start[tid], my_e1 = start[tid + 1];
  auto publish = [&](uint32_t item, uint32_t slot) {
    if (item >= my_it0 && item < my_it1) {
      const uint32_t e_lo = my_e0 + (item - my_it0) * kFoldChunk;
      s_item[slot][0] = tid;
      s_item[slot][1] = my_it1 - my_it0 == 1u ? 1u : 0u;
      s_item[slot][2] = e_lo;
      s_item[slot][3] = my_e1 - e_lo < kFoldChunk ? my_e1 : e_lo + kFoldChunk;
    }
  };
  auto item_word = [&](uint32_t slot, uint32_t k) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)s_item[slot][k]); };
  // four 16-byte loads from the aligned-down start, without a branch: a load past the item's end is one of the 16-byte
  // group that holds the item's last entry instead.  What lies outside the item is masked when the batch is processed
  const uint4* g4 = reinterpret_cast<const uint4*>(grouped);
  auto request = [&](uint4 (&d)[kIn4], uint32_t i0, uint32_t e_end) {
    const uint32_t last = (e_end - 1u) / 4u;
#pragma unroll
    for (uint32_t k = 0; k < kIn4; ++k) {
      const uint32_t i4 = i0 / 4u + k * kFoldTPB + tid;
      d[k] = g4[i4 < last ? i4 : last];
    }
  };
  publish(u.item, 0u);
  fold_lds_barrier();
  uint4 cur[kIn4], nxt[kIn4];
  request(cur, item_word(0u, 2u) & ~3u, item_word(0u, 3u));
  for (uint32_t step = 0, slot = 0; u.valid; ++step, slot ^= 1u) {
    const uint32_t b = item_word(slot, 0u), quarter = u.quarter;
    const bool owner = item_word(slot, 1u) != 0u;
    const uint32_t e_lo = item_word(slot, 2u), e_end = item_word(slot, 3u), first = e_lo & ~3u;
    // (the other slot was last read before this unit's predecessor passed its barriers; read again behind this unit's)
    u = fold_apply_unit(blockIdx.x, gridDim.x, step + 1u, n_items);
    const bool more = u.valid;
    if (more) publish(u.item, slot ^ 1u);
    // the bucket's quarters as far as the table reaches (no entry can fall past its end); a unit past them has nothing
    // to do but to request the next one's entries.  Its own first batch, requested one unit ahead, was read for nothing
    // and the next unit's request is not ahead of anything: at most three units of a fold (the last bucket's), which
    // the walk would have to know the table's end to leave out
    const uint64_t wb = (uint64_t)b << (kFoldBucketShift - 5);
    const uint64_t left = n_words - wb;
    const uint32_t n_q = left >= (uint64_t)kFoldQuarters * kFoldQuarterWords
                             ? kFoldQuarters : (uint32_t)((left + kFoldQuarterWords - 1u) / kFoldQuarterWords);
    if (quarter >= n_q) {
      fold_lds_barrier();
      if (more) request(cur, item_word(slot ^ 1u, 2u) & ~3u, item_word(slot ^ 1u, 3u));
      continue;
    }
    const uint64_t w0 = wb + (uint64_t)quarter * kFoldQuarterWords;
    const uint32_t nw = n_words - w0 < kFoldQuarterWords ? (uint32_t)(n_words - w0) : kFoldQuarterWords;
    uint32_t* gw = bits + w0;
    if (fresh && owner) {
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) q4[k * kFoldTPB + tid] = make_uint4(0u, 0u, 0u, 0u);
    } else if (nw == kFoldQuarterWords) {
      // a whole quarter: its loads together, one wait
      uint4 v[kPer];
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) v[k] = reinterpret_cast<const uint4*>(gw)[k * kFoldTPB + tid];
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) q4[k * kFoldTPB + tid] = v[k];
    } else {
      // the table's ragged last quarter
#pragma unroll 1
      for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t w = (k * kFoldTPB + tid) * 4u;
        uint4 v;
        if (w + 4u <= nw) {
          v = reinterpret_cast<const uint4*>(gw)[w / 4u];
        } else {
          v.x = w + 0u < nw ? gw[w + 0u] : 0u;
          v.y = w + 1u < nw ? gw[w + 1u] : 0u;
          v.z = w + 2u < nw ? gw[w + 2u] : 0u;
          v.w = w + 3u < nw ? gw[w + 3u] : 0u;
        }
        q4[w / 4u] = v;
      }
    }
    fold_lds_barrier();
    for (uint32_t i0 = first; i0 < e_end; i0 += kBatch) {
      if (e_end - i0 > kBatch) {
        request(nxt, i0 + kBatch, e_end);
      } else if (more) {
        request(nxt, item_word(slot ^ 1u, 2u) & ~3u, item_word(slot ^ 1u, 3u));
      } else {
#pragma unroll
        for (uint32_t k = 0; k < kIn4; ++k) nxt[k] = none4;
      }
      // the batch's sixteen LDS atomics back to back, one wait: an entry of another quarter, or outside the item, ORs
      // nothing into a word of the thread's own (no two lanes of a wave meet there)
      const uint32_t x[kIn4 * 4] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w,
                                    cur[2].x, cur[2].y, cur[2].z, cur[2].w, cur[3].x, cur[3].y, cur[3].z, cur[3].w};
      uint32_t old[kIn4 * 4], mine = 0;
#pragma unroll
      for (uint32_t k = 0; k < kIn4 * 4; ++k) {
        const uint32_t i = i0 + ((k / 4u) * kFoldTPB + tid) * 4u + (k & 3u);
        const bool on = i >= e_lo && i < e_end && ((x[k] >> kFoldQuarterShift) & (kFoldQuarters - 1u)) == quarter;
        mine |= (on ? 1u : 0u) << k;
        old[k] = atomicOr(&fold_smem[on ? (x[k] >> 5) & (kFoldQuarterWords - 1u) : tid], on ? 1u << (x[k] & 31u) : 0u);
      }
      // the two rare follow-ups, one entry at a time: a bit that was set already makes the entry a table add.  A split
      // bucket: the first of the item's entries claims the bit in memory at once; another item may have been first (a
      // repeat after all)
      uint32_t again = 0;
#pragma unroll
      for (uint32_t k = 0; k < kIn4 * 4; ++k) again |= ((old[k] >> (x[k] & 31u)) & 1u) << k;
      again &= mine;
      uint32_t todo = owner ? again : mine;
      while (todo) {
        const uint32_t k = (uint32_t)__builtin_ctz(todo);
        todo &= todo - 1u;
        uint32_t v = x[0];
#pragma unroll
        for (uint32_t j = 1; j < kIn4 * 4; ++j) v = k == j ? x[j] : v;
        const uint32_t m = 1u << (v & 31u);
        if (((again >> k) & 1u) || (atomicOr(&gw[(v >> 5) & (kFoldQuarterWords - 1u)], m) & m)) add(v);
      }
#pragma unroll
      for (uint32_t k = 0; k < kIn4; ++k) cur[k] = nxt[k];
    }
    fold_lds_barrier();
    // the owner writes its quarter back as it is now (nearly every line of it changed for a sparse batch), with
    // non-temporal stores: nobody reads these 128 KB again soon, and the L2 they pass through holds the entries that
    // the units of the other quarters are still reading
    if (owner && nw == kFoldQuarterWords) {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) {
        const uint4 c = q4[k * kFoldTPB + tid];
        const u32x4 cv = {c.x, c.y, c.z, c.w};
        __builtin_nontemporal_store(cv, reinterpret_cast<u32x4*>(gw) + k * kFoldTPB + tid);
      }
    } else if (owner) {
#pragma unroll 1
      for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t w = (k * kFoldTPB + tid) * 4u;
        const uint4 c = q4[w / 4u];
        if (w + 4u <= nw) {
          reinterpret_cast<uint4*>(gw)[w / 4u] = c;
        } else {
          if (w + 0u < nw) gw[w + 0u] = c.x;
          if (w + 1u < nw) gw[w + 1u] = c.y;
          if (w + 2u < nw) gw[w + 2u] = c.z;
        }
      }
    }
    fold_lds_barrier();
  }
}

// The fold's launch sequence, on `stream`: the engine's fold_log() and the tests' harness (tests/fold) both call it.
// log: n entries; grouped: room for n; meta: [cnt | start | cursor | item_off], kFoldMaxBuckets + 1 words each, with
// cnt all zero (the fold leaves it so); nb: buckets (ceil(entries / 2^22), at most kFoldMaxBuckets); n_words: bit-map
// words in use; dirty: the table's dirty-block map, or null.  scatter_grid / apply_grid: 0 = sized from n_cus as the
// engine does; tests force other counts to vary how tiles and items interleave.  fresh: the bit map counts as all zero
// and is not read (see the top of the file); every one of its n_words words is written.  have_cnt: cnt already holds
// the entries per bucket (whoever wrote the log counted them): bc_fold_hist is skipped.  log and grouped are 16-byte
// aligned: hipErrorInvalidValue otherwise, and nothing is launched.
inline hipError_t fold_launch(hipStream_t stream, const uint32_t* log, uint64_t n, uint32_t* grouped, uint32_t* meta,
                              uint32_t nb, uint32_t* bits, uint64_t n_words, uint32_t* table, uint8_t* dirty, uint32_t n_cus,
                              uint32_t scatter_grid = 0, uint32_t apply_grid = 0, bool fresh = false,
                              bool have_cnt = false) {
  if ((reinterpret_cast<uintptr_t>(log) | reinterpret_cast<uintptr_t>(grouped)) & 15u) return hipErrorInvalidValue;
  uint32_t* cnt = meta;
  uint32_t* start = cnt + kFoldMaxBuckets + 1;
  uint32_t* cursor = start + kFoldMaxBuckets + 1;
  uint32_t* item_off = cursor + kFoldMaxBuckets + 1;
  const uint64_t hist_cap = 4ull * n_cus, hist_want = (n / 4 + kFoldTPB - 1) / kFoldTPB + 1;
  const uint64_t hist_grid = hist_want < hist_cap ? hist_want : hist_cap;
  if (!have_cnt) hipLaunchKernelGGL(bc_fold_hist, dim3((uint32_t)hist_grid), dim3(kFoldTPB), 0, stream, log, n, nb, cnt);
  hipLaunchKernelGGL(bc_fold_scan, dim3(1), dim3(kFoldTPB), 0, stream, cnt, nb, start, cursor, item_off);
  hipError_t rc = hipFuncSetAttribute((const void*)bc_fold_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFoldScatterLds);
  if (rc != hipSuccess) return rc;
  rc = hipFuncSetAttribute((const void*)bc_fold_apply, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFoldApplyLds);
  if (rc != hipSuccess) return rc;
  const uint64_t tiles = (n + kFoldTile - 1) / kFoldTile, scatter_cap = 2ull * n_cus;
  if (!scatter_grid) scatter_grid = (uint32_t)(tiles < scatter_cap ? tiles : scatter_cap);
  hipLaunchKernelGGL(bc_fold_scatter, dim3(scatter_grid), dim3(kFoldTPB), kFoldScatterLds, stream, log, n, nb, cursor, grouped);
  if (fresh) {
    const uint32_t pairs = nb * kFoldQuarters, zero_cap = 4u * n_cus;
    hipLaunchKernelGGL(bc_fold_zero_unowned, dim3(pairs < zero_cap ? pairs : zero_cap), dim3(kFoldTPB), 0, stream, nb,
                       (const uint32_t*)item_off, bits, n_words);
  }
  const uint64_t items_max = (n + kFoldChunk - 1) / kFoldChunk + nb;
  if (!apply_grid) {
    // one workgroup per CU, in whole sibling groups where the device has that many CUs (fold_apply_unit)
    const uint64_t units_max = items_max * kFoldQuarters, group = kFoldXcds * kFoldQuarters;
    const uint64_t cus = n_cus >= group ? n_cus - n_cus % group : n_cus;
    apply_grid = (uint32_t)(units_max < cus ? units_max : cus);
  }
  hipLaunchKernelGGL(bc_fold_apply, dim3(apply_grid), dim3(kFoldTPB), kFoldApplyLds, stream, (const uint32_t*)grouped, nb,
                     (const uint32_t*)start, (const uint32_t*)item_off, bits, n_words, table, dirty, fresh ? 1u : 0u);
  return hipGetLastError();
}

#endif  // __HIPCC__

}  // namespace bc
