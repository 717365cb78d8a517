// Log-mode counting (bc_kernel.h, match_count_body with `count_log`): the fold of a count log into the two-level
// counters (first-occurrence bit map + table).
//
// The match kernel leaves one u32 per read: the read's dense tuple index, or kLogNone.  Four kernels then apply it:
//   bc_fold_hist     entries per bucket (a bucket = 2^22 tuples = 512 KB of bit map; at most 1024 buckets)
//   bc_fold_scan     bucket starts, and the fold's work items (bucket x chunk of entries)
//   bc_fold_scatter  the log grouped by bucket: 16384-entry tiles sorted in LDS, then written out as runs
//   bc_fold_apply    per item and quarter of its bucket: 128 KB of bit map into LDS, one LDS atomicOr per entry (a bit
//                    that was set already makes the entry a table add), the quarter written back
// A tuple with c entries ends as the atomic path would leave it: bit clear before -> bit set and table + c - 1; bit set
// before -> table + c.  A bucket with more than kFoldChunk entries (a hot library) is split over several items, which
// then meet on the same quarter: there the first entry of a tuple in an item also sets its bit in memory, with a
// returning atomicOr, and a bit another item had set meanwhile was not a first occurrence after all (table + 1).
// Exactly one of them sets each bit; only the sole item of a bucket writes its quarters back whole.
//
// A fold onto a map that is known to be all zero but has not been written so (`fresh`: the engine's first fold after a
// reset, bc_engine.hip) reads none of it: the sole item of a bucket starts its quarters from zeroed LDS and writes them
// back whole as ever, and bc_fold_zero_unowned, between scan and apply, writes zeros over the buckets that have no sole
// item -- the empty ones, and the split ones, whose items meet in memory.  Every word of the map is defined afterwards.
#pragma once

namespace bc {

constexpr uint32_t kFoldTPB = 1024;
constexpr uint32_t kFoldBucketShift = 22;   // tuples per bucket: 2^22
constexpr uint32_t kFoldQuarterShift = 20;  // tuples per apply pass: 2^20 (32768 bit-map words, 128 KB of LDS)
constexpr uint32_t kFoldQuarters = 1u << (kFoldBucketShift - kFoldQuarterShift);
constexpr uint32_t kFoldMaxBuckets = 1024;  // indexes below 2^32
constexpr uint32_t kFoldTile = 16384;       // bc_fold_scatter: entries per LDS tile (two workgroups per CU)
constexpr uint32_t kFoldChunk = 1u << 18;   // entries per apply item at most
constexpr uint32_t kFoldQuarterWords = 1u << (kFoldQuarterShift - 5);
constexpr uint32_t kFoldScatterLds = kFoldTile * 4u + 3u * kFoldMaxBuckets * 4u;
constexpr uint32_t kFoldApplyLds = kFoldQuarterWords * 4u;

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

__global__ __launch_bounds__(kFoldTPB) void bc_fold_scatter(const uint32_t* __restrict__ log, uint64_t n, uint32_t nb,
                                                           uint32_t* __restrict__ cursor, uint32_t* __restrict__ out) {
  extern __shared__ uint32_t fold_smem[];
  uint32_t* sorted = fold_smem;
  uint32_t* h = sorted + kFoldTile;
  uint32_t* lstart = h + kFoldMaxBuckets;
  uint32_t* base = lstart + kFoldMaxBuckets;
  __shared__ uint32_t tmp[kFoldTPB / 64u];
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t kPer = kFoldTile / kFoldTPB;
  const uint64_t n_tiles = (n + kFoldTile - 1u) / kFoldTile;
  for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const uint64_t t0 = t * kFoldTile;
    for (uint32_t i = tid; i < kFoldMaxBuckets; i += kFoldTPB) h[i] = 0;
    __syncthreads();
    // the entries' ranks within their bucket, two per register (below 2^15); the entries themselves are read again
    // below (from the L2) rather than held in registers
    uint32_t r[kPer / 2];
    const uint32_t* tl = log + t0 + tid;
    const uint32_t n_t = n - t0 < kFoldTile ? (uint32_t)(n - t0) : kFoldTile;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t v = k * kFoldTPB + tid < n_t ? tl[k * kFoldTPB] : kLogNone;
      const uint32_t rk = v != kLogNone ? atomicAdd(&h[v >> kFoldBucketShift], 1u) : 0u;
      if (k & 1u) r[k / 2] |= rk << 16; else r[k / 2] = rk;
    }
    __syncthreads();
    // one bucket per thread (nb <= 1024): the tile's runs, and their places in the grouped log
    const uint32_t hc = tid < nb ? h[tid] : 0u;
    uint32_t valid;
    const uint32_t ls = fold_block_scan(hc, tmp, valid);
    if (tid < nb) {
      lstart[tid] = ls;
      if (hc) base[tid] = atomicAdd(&cursor[tid], hc);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t v = k * kFoldTPB + tid < n_t ? tl[k * kFoldTPB] : kLogNone;
      if (v != kLogNone) sorted[lstart[v >> kFoldBucketShift] + ((r[k / 2] >> (16u * (k & 1u))) & 0xFFFFu)] = v;
    }
    __syncthreads();
    for (uint32_t i = tid; i < valid; i += kFoldTPB) {
      const uint32_t x = sorted[i];
      const uint32_t bk = x >> kFoldBucketShift;
      out[base[bk] + (i - lstart[bk])] = x;
    }
    __syncthreads();
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
// as all zero whatever memory holds (the owner of a bucket does not load it; bc_fold_zero_unowned has run)
__global__ __launch_bounds__(kFoldTPB) void bc_fold_apply(const uint32_t* __restrict__ grouped, uint32_t nb,
                                                         const uint32_t* __restrict__ start, const uint32_t* __restrict__ item_off,
                                                         uint32_t* __restrict__ bits, uint64_t n_words, uint32_t* __restrict__ table,
                                                         uint8_t* __restrict__ dirty, uint32_t fresh) {
  extern __shared__ uint32_t fold_smem[];
  uint4* q4 = reinterpret_cast<uint4*>(fold_smem);
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t kPer = kFoldQuarterWords / 4u / kFoldTPB;  // uint4 per thread
  const uint32_t n_items = item_off[nb];
  auto add = [&](uint32_t idx) {
    table_add(&table[idx]);
    if (dirty) dirty[idx >> 6] = (uint8_t)1;
  };
  for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
    // the item's bucket: the last b with item_off[b] <= it
    uint32_t lo_b = 0, hi_b = nb;
    while (hi_b - lo_b > 1u) {
      const uint32_t mid = (lo_b + hi_b) >> 1;
      if (item_off[mid] <= it) lo_b = mid; else hi_b = mid;
    }
    const uint32_t b = lo_b;
    const uint32_t chunk = it - item_off[b];
    const bool owner = item_off[b + 1] - item_off[b] == 1u;
    // the bucket's four quarters one after the other: the chunk's entries are read four times, from the L2
    for (uint32_t quarter = 0; quarter < kFoldQuarters; ++quarter) {
      const uint64_t w0 = ((uint64_t)b << (kFoldBucketShift - 5)) + (uint64_t)quarter * kFoldQuarterWords;
      if (w0 >= n_words) break;  // past the table's end: no entry can fall here
      const uint64_t nw = n_words - w0 < kFoldQuarterWords ? n_words - w0 : kFoldQuarterWords;
      uint32_t* gw = bits + w0;
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t w = (k * kFoldTPB + tid) * 4u;
        uint4 v;
        if (fresh && owner) {
          v = make_uint4(0u, 0u, 0u, 0u);
        } else if (w + 4u <= nw) {
          v = reinterpret_cast<const uint4*>(gw)[w / 4u];
        } else {
          v.x = w + 0u < nw ? gw[w + 0u] : 0u;
          v.y = w + 1u < nw ? gw[w + 1u] : 0u;
          v.z = w + 2u < nw ? gw[w + 2u] : 0u;
          v.w = w + 3u < nw ? gw[w + 3u] : 0u;
        }
        q4[w / 4u] = v;
      }
      __syncthreads();
      const uint32_t e_lo = start[b] + chunk * kFoldChunk;
      const uint32_t e_end = start[b + 1] - e_lo < kFoldChunk ? start[b + 1] : e_lo + kFoldChunk;
      // 16 entries in flight per thread (four 16-byte loads from the aligned-down start; what lies outside the chunk
      // is skipped) before any of them is used: one round trip per 16 K entries
      constexpr uint32_t kIn4 = 4;
      const uint4* g4 = reinterpret_cast<const uint4*>(grouped);
      for (uint32_t i0 = e_lo & ~3u; i0 < e_end; i0 += kIn4 * 4u * kFoldTPB) {
        uint32_t x[kIn4 * 4];
#pragma unroll
        for (uint32_t k = 0; k < kIn4; ++k) {
          const uint32_t i = i0 + (k * kFoldTPB + tid) * 4u;
          const uint4 v = i < e_end ? g4[i / 4u] : make_uint4(kLogNone, kLogNone, kLogNone, kLogNone);
          x[4 * k + 0] = i + 0u >= e_lo && i + 0u < e_end ? v.x : kLogNone;
          x[4 * k + 1] = i + 1u >= e_lo && i + 1u < e_end ? v.y : kLogNone;
          x[4 * k + 2] = i + 2u >= e_lo && i + 2u < e_end ? v.z : kLogNone;
          x[4 * k + 3] = i + 3u >= e_lo && i + 3u < e_end ? v.w : kLogNone;
        }
#pragma unroll
        for (uint32_t k = 0; k < kIn4 * 4; ++k) {
          if (x[k] == kLogNone || ((x[k] >> kFoldQuarterShift) & (kFoldQuarters - 1u)) != quarter) continue;
          const uint32_t m = 1u << (x[k] & 31u);
          const uint32_t wq = (x[k] >> 5) & (kFoldQuarterWords - 1u);
          const uint32_t old = atomicOr(&fold_smem[wq], m);
          // a split bucket: the first of the item's entries claims the bit in memory at once; another item may have
          // been first (a repeat after all)
          if ((old & m) || (!owner && (atomicOr(&gw[wq], m) & m))) add(x[k]);
        }
      }
      __syncthreads();
      // the owner writes its quarter back as it is now (nearly every line of it changed for a sparse batch)
      if (owner) {
#pragma unroll
        for (uint32_t k = 0; k < kPer; ++k) {
          const uint32_t w = (k * kFoldTPB + tid) * 4u;
          const uint4 cur = q4[w / 4u];
          if (w + 4u <= nw) {
            reinterpret_cast<uint4*>(gw)[w / 4u] = cur;
          } else {
            if (w + 0u < nw) gw[w + 0u] = cur.x;
            if (w + 1u < nw) gw[w + 1u] = cur.y;
            if (w + 2u < nw) gw[w + 2u] = cur.z;
          }
        }
      }
      __syncthreads();
    }
  }
}

// The fold's launch sequence, on `stream`: the engine's fold_log() and the tests' harness (tests/fold) both call it.
// log: n entries; grouped: room for n; meta: [cnt | start | cursor | item_off], kFoldMaxBuckets + 1 words each, with
// cnt all zero (the fold leaves it so); nb: buckets (ceil(entries / 2^22), at most kFoldMaxBuckets); n_words: bit-map
// words in use; dirty: the table's dirty-block map, or null.  scatter_grid / apply_grid: 0 = sized from n_cus as the
// engine does; tests force other counts to vary how tiles and items interleave.  fresh: the bit map counts as all zero
// and is not read (see the top of the file); every one of its n_words words is written.  have_cnt: cnt already holds
// the entries per bucket (whoever wrote the log counted them): bc_fold_hist is skipped.
inline hipError_t fold_launch(hipStream_t stream, const uint32_t* log, uint64_t n, uint32_t* grouped, uint32_t* meta,
                              uint32_t nb, uint32_t* bits, uint64_t n_words, uint32_t* table, uint8_t* dirty, uint32_t n_cus,
                              uint32_t scatter_grid = 0, uint32_t apply_grid = 0, bool fresh = false,
                              bool have_cnt = false) {
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
  if (!apply_grid) apply_grid = (uint32_t)(items_max < n_cus ? items_max : n_cus);
  hipLaunchKernelGGL(bc_fold_apply, dim3(apply_grid), dim3(kFoldTPB), kFoldApplyLds, stream, (const uint32_t*)grouped, nb,
                     (const uint32_t*)start, (const uint32_t*)item_off, bits, n_words, table, dirty, fresh ? 1u : 0u);
  return hipGetLastError();
}

}  // namespace bc
