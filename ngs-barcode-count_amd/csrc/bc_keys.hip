// bc_keys.hip -- the key tables of the engine (include/barcode_count_hip.h): the hash set of (tuple, random barcode)
// keys and the (key -> count) map of raw-capture plans, narrow (one u64 per key, bc_kernel.h) and wide (bc_long.h).
// Growing and clearing them, exporting their pairs for the rows and the renderers, the per-tuple distinct counts of a
// random-barcode plan, and the import / export of keys and counts that the multi-GPU exchange runs on.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/barcode_count_hip.h"
#include "bc_kernel.h"
#include "bc_long.h"
#include "bc_engine_impl.h"

namespace bc {

// ---- tables of wide keys (bc_long.h): W words per slot + a ready flag; ONE lane of a wavefront inserts at a time ----
// keys[i * W ..] (+ vals[i], or 1 for every key when vals is null and count_ones, or nothing) into the table; *n_new
// counts the keys that were not there.  zero_from / zero_bits: payload bits cleared before the insert (with the
// fingerprint recomputed) -- the random barcode's planes, when the table being built is the per-tuple aggregate.
__global__ void wide_insert_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ src_ready,
                                   const uint32_t* __restrict__ src_vals, uint64_t n, uint32_t W,
                                   unsigned long long* __restrict__ slots, uint32_t* __restrict__ ready, uint32_t* __restrict__ vals,
                                   uint64_t mask, int add_one, uint32_t zero_from, uint32_t zero_bits,
                                   unsigned long long* __restrict__ n_new) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  uint32_t fresh = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += step) {
    const uint64_t i = base + threadIdx.x;
    const bool have = i < n && (!src_ready || src_ready[i] != 0u);  // (a source table: only its published slots)
    unsigned long long todo = __ballot(have);
    while (todo) {
      const unsigned l = (unsigned)__ffsll((long long)todo) - 1u;
      todo &= todo - 1ull;
      if (__lane_id() == l) {
        uint64_t key[kMaxKeyWords];
        for (uint32_t w = 0; w < W; ++w) key[w] = keys[i * W + w];
        if (zero_bits) {
          for (uint32_t b = zero_from; b < zero_from + zero_bits; ++b) key[1u + (b >> 6)] &= ~(1ull << (b & 63u));
          key[0] = wide_fingerprint(key, W);
        }
        bool is_new;
        const uint64_t slot = wide_find_or_insert(slots, ready, mask, W, key, is_new);
        fresh += is_new ? 1u : 0u;
        if (vals) atomicAdd(&vals[slot], src_vals ? src_vals[i] : (add_one ? 1u : 0u));
      }
    }
  }
  if (n_new && fresh) atomicAdd(n_new, (unsigned long long)fresh);
}

// the published slots of a table, densely: keys (W words each) and counts
__global__ void wide_export_kernel(const unsigned long long* __restrict__ slots, const uint32_t* __restrict__ ready,
                                   const uint32_t* __restrict__ vals, uint64_t n, uint32_t W, unsigned long long* cursor,
                                   unsigned long long* __restrict__ out_keys, uint32_t* __restrict__ out_vals, uint64_t capacity) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    if (ready[i] == 0u) continue;
    if (vals && out_vals && vals[i] == 0u) continue;  // (a key whose count was discarded never shows)
    const unsigned long long p = atomicAdd(cursor, 1ull);
    if (p < capacity) {
      if (out_keys)
        for (uint32_t w = 0; w < W; ++w) out_keys[p * W + w] = slots[i * W + w];
      if (out_vals) out_vals[p] = vals ? vals[i] : 1u;
    }
  }
}

__global__ void set_fill_kernel(unsigned long long* slots, uint64_t n) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) slots[i] = kEmptyKey;
}

// re-inserts every key of `src` (n slots, or n plain keys when `dense`) into dst; counts the new ones
__global__ void set_insert_kernel(const unsigned long long* __restrict__ src, uint64_t n, unsigned long long* dst,
                                  uint64_t dmask, unsigned long long* n_new) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  uint32_t c = 0;
  for (; i < n; i += step) {
    const unsigned long long k = src[i];
    if (k != kEmptyKey && set_insert(dst, dmask, k)) ++c;
  }
  if (n_new) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if (__lane_id() == 0 && c) atomicAdd(n_new, (unsigned long long)c);
  }
}

// moves (key, value) pairs into a larger map
__global__ void map_rehash_kernel(const unsigned long long* __restrict__ src, const uint32_t* __restrict__ src_vals,
                                  uint64_t n, unsigned long long* dst, uint32_t* dst_vals, uint64_t dmask) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = src[i];
    if (k != kEmptyKey) atomicAdd(&dst_vals[map_slot(dst, dmask, k)], src_vals[i]);
  }
}

// raw captures + random barcode: count of a tuple = number of its distinct (tuple, random) keys
__global__ void set_to_map_kernel(const unsigned long long* __restrict__ slots, uint64_t n, uint64_t rspace,
                                  unsigned long long* dst, uint32_t* dst_vals, uint64_t dmask) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = slots[i];
    if (k != kEmptyKey) atomicAdd(&dst_vals[map_slot(dst, dmask, k / rspace)], 1u);
  }
}

__global__ void map_export_kernel(const unsigned long long* __restrict__ slots, const uint32_t* __restrict__ vals,
                                  uint64_t n, unsigned long long* cursor, uint64_t* __restrict__ out_key,
                                  uint32_t* __restrict__ out_cnt) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = slots[i];
    if (k != kEmptyKey) {
      const unsigned long long p = atomicAdd(cursor, 1ull);
      out_key[p] = k;
      out_cnt[p] = vals[i];
    }
  }
}

// adds (key, count) pairs into a map
__global__ void map_add_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ cnts, uint64_t n,
                               unsigned long long* dst, uint32_t* dst_vals, uint64_t dmask) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = keys[i];
    if (k != kEmptyKey && cnts[i]) atomicAdd(&dst_vals[map_slot(dst, dmask, k)], cnts[i]);
  }
}

// counts the occupied slots with a non-zero value / writes them out (capacity-checked)
__global__ void map_export_checked_kernel(const unsigned long long* __restrict__ slots, const uint32_t* __restrict__ vals,
                                          uint64_t n, unsigned long long* cursor, unsigned long long* __restrict__ out_key,
                                          uint32_t* __restrict__ out_cnt, uint64_t capacity) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = slots[i];
    if (k != kEmptyKey && vals[i]) {
      const unsigned long long p = atomicAdd(cursor, 1ull);
      if (p < capacity) {
        out_key[p] = k;
        out_cnt[p] = vals[i];
      }
    }
  }
}

// compacts the keys of a set into out[0 .. *cursor)
__global__ void set_export_kernel(const unsigned long long* __restrict__ slots, uint64_t n, unsigned long long* cursor,
                                  unsigned long long* __restrict__ out, uint64_t capacity) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = slots[i];
    if (k != kEmptyKey) {
      const unsigned long long p = atomicAdd(cursor, 1ull);
      if (p < capacity) out[p] = k;
    }
  }
}

// final counts with a random barcode = number of distinct random barcodes per tuple (output.rs:265-270)
__global__ void set_to_table_kernel(const unsigned long long* __restrict__ slots, uint64_t n, uint64_t rspace,
                                    uint32_t* __restrict__ table) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = slots[i];
    if (k != kEmptyKey) atomicAdd(&table[k / rspace], 1u);
  }
}

}  // namespace bc

using namespace bc;

int bc::set_reserve(bc_engine* e, uint64_t more) {
  const DevPlan& P = e->h.plan;
  if (!P.has_random && !P.sparse) return BC_OK;
  const bool with_vals = P.sparse && !P.has_random;
  const uint32_t W = e->key_words;
  e->key_bound += more;
  uint64_t want = 1ull << 20;
  while (want < 2 * e->key_bound) want <<= 1;
  if (want <= e->n_slots) return BC_OK;
  unsigned long long* fresh = nullptr;
  uint32_t* fresh_vals = nullptr;
  uint32_t* fresh_ready = nullptr;
  ScratchGuard g;  // (what is allocated here is released on an early return, and handed over at the end)
  HIP_TRY(g.dmalloc(&fresh, want * W * 8));
  hipLaunchKernelGGL(set_fill_kernel, dim3(grid_for(want * W)), dim3(256), 0, e->stream, fresh, want * W);
  if (with_vals) {
    HIP_TRY(g.dmalloc(&fresh_vals, want * 4));
    HIP_TRY(hipMemsetAsync(fresh_vals, 0, want * 4, e->stream));
  }
  if (W > 1) {
    HIP_TRY(g.dmalloc(&fresh_ready, want * 4));
    HIP_TRY(hipMemsetAsync(fresh_ready, 0, want * 4, e->stream));
  }
  if (e->d_slots) {
    if (W > 1)
      hipLaunchKernelGGL(wide_insert_kernel, dim3(grid_for(e->n_slots)), dim3(256), 0, e->stream, e->d_slots, e->d_ready, e->d_vals,
                         e->n_slots, W, fresh, fresh_ready, fresh_vals, want - 1, 0, 0u, 0u, (unsigned long long*)nullptr);
    else if (with_vals)
      hipLaunchKernelGGL(map_rehash_kernel, dim3(grid_for(e->n_slots)), dim3(256), 0, e->stream, e->d_slots, e->d_vals,
                         e->n_slots, fresh, fresh_vals, want - 1);
    else
      hipLaunchKernelGGL(set_insert_kernel, dim3(grid_for(e->n_slots)), dim3(256), 0, e->stream, e->d_slots, e->n_slots,
                         fresh, want - 1, (unsigned long long*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    (void)hipFree(e->d_slots);
    if (e->d_vals) (void)hipFree(e->d_vals);
    if (e->d_ready) (void)hipFree(e->d_ready);
  }
  HIP_TRY(hipGetLastError());
  g.dev.clear();  // kept: the engine owns them now
  e->d_slots = fresh;
  e->d_vals = fresh_vals;
  e->d_ready = fresh_ready;
  e->n_slots = want;
  return BC_OK;
}

int bc::export_pairs(bc_engine* e, const char* who, ScratchGuard& g, uint64_t** d_key, uint32_t** d_cnt, uint64_t* n_out) {
  unsigned long long* keys = e->d_slots;
  uint32_t* vals = e->d_vals;
  const uint64_t n_slots = e->n_slots;
  if (e->h.plan.has_random) {
    // count of a tuple = number of its distinct random barcodes (output.rs:265-270)
    unsigned long long* agg_keys = nullptr;
    uint32_t* agg_vals = nullptr;
    HIP_TRY(g.dmalloc(&agg_keys, n_slots * 8));
    HIP_TRY(g.dmalloc(&agg_vals, n_slots * 4));
    hipLaunchKernelGGL(set_fill_kernel, dim3(grid_for(n_slots)), dim3(256), 0, e->stream, agg_keys, n_slots);
    HIP_TRY(hipMemsetAsync(agg_vals, 0, n_slots * 4, e->stream));
    hipLaunchKernelGGL(set_to_map_kernel, dim3(grid_for(n_slots)), dim3(256), 0, e->stream, e->d_slots, n_slots,
                       e->h.plan.rspace, agg_keys, agg_vals, n_slots - 1);
    HIP_TRY(hipGetLastError());
    keys = agg_keys;
    vals = agg_vals;
  }
  unsigned long long* d_n = nullptr;
  HIP_TRY(g.dmalloc(&d_n, 8));
  HIP_TRY(hipMemsetAsync(d_n, 0, 8, e->stream));
  // upper bound on the rows: the keys held
  const uint64_t cap = std::min<uint64_t>(n_slots, e->key_bound ? e->key_bound : 1);
  HIP_TRY(g.dmalloc(d_key, cap * 8));
  HIP_TRY(g.dmalloc(d_cnt, cap * 4));
  hipLaunchKernelGGL(map_export_kernel, dim3(grid_for(n_slots)), dim3(256), 0, e->stream, keys, vals, n_slots, d_n, *d_key,
                     *d_cnt);
  HIP_TRY(hipGetLastError());
  unsigned long long n = 0;
  HIP_TRY(hipMemcpyAsync(&n, d_n, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (n > cap) {  // (cannot happen: key_bound counts every insert)
    set_error(std::string(who) + ": the key map holds more keys than its bound");
    return BC_ERR_STATE;
  }
  *n_out = n;
  return BC_OK;
}

// wide keys (bc_long.h): the two steps of export_pairs on slots of key_words words
int bc::export_wide(bc_engine* e, const char* who, ScratchGuard& g, unsigned long long** d_key, uint32_t** d_cnt,
                    uint64_t* n_out) {
  const DevPlan& P = e->h.plan;
  unsigned long long* keys = e->d_slots;
  uint32_t* vals = e->d_vals;
  const uint64_t n_slots = e->n_slots;
  const uint32_t W = e->key_words;
  const uint32_t* ready = e->d_ready;
  ScratchGuard agg;  // the table of tuples: gone when the rows are out
  if (P.has_random) {
    // count of a tuple = number of its distinct random barcodes (output.rs:265-270): every key, its random
    // barcode's planes cleared, into a map of tuples
    unsigned long long* agg_keys = nullptr;
    uint32_t *agg_vals = nullptr, *agg_ready = nullptr;
    HIP_TRY(agg.dmalloc(&agg_keys, n_slots * W * 8));
    HIP_TRY(agg.dmalloc(&agg_vals, n_slots * 4));
    HIP_TRY(agg.dmalloc(&agg_ready, n_slots * 4));
    hipLaunchKernelGGL(set_fill_kernel, dim3(grid_for(n_slots * W)), dim3(256), 0, e->stream, agg_keys, n_slots * W);
    HIP_TRY(hipMemsetAsync(agg_vals, 0, n_slots * 4, e->stream));
    HIP_TRY(hipMemsetAsync(agg_ready, 0, n_slots * 4, e->stream));
    hipLaunchKernelGGL(wide_insert_kernel, dim3(grid_for(n_slots)), dim3(256), 0, e->stream, e->d_slots, e->d_ready,
                       (const uint32_t*)nullptr, n_slots, W, agg_keys, agg_ready, agg_vals, n_slots - 1, 1, e->lh.plan.rnd_bit,
                       3u * e->lh.plan.rnd_len, (unsigned long long*)nullptr);
    HIP_TRY(hipGetLastError());
    keys = agg_keys;
    vals = agg_vals;
    ready = agg_ready;
  }
  unsigned long long* d_n = nullptr;
  HIP_TRY(agg.dmalloc(&d_n, 8));
  HIP_TRY(hipMemsetAsync(d_n, 0, 8, e->stream));
  const uint64_t cap = std::min<uint64_t>(n_slots, e->key_bound ? e->key_bound : 1);
  HIP_TRY(g.dmalloc(d_key, cap * W * 8));
  HIP_TRY(g.dmalloc(d_cnt, cap * 4));
  hipLaunchKernelGGL(wide_export_kernel, dim3(grid_for(n_slots)), dim3(256), 0, e->stream, keys, ready, vals, n_slots, W, d_n, *d_key,
                     *d_cnt, cap);
  HIP_TRY(hipGetLastError());
  unsigned long long n = 0;
  HIP_TRY(hipMemcpyAsync(&n, d_n, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (n > cap) {  // (cannot happen: key_bound counts every insert)
    set_error(std::string(who) + ": the key map holds more keys than its bound");
    return BC_ERR_STATE;
  }
  *n_out = n;
  return BC_OK;
}

extern "C" {

// Random-barcode plans with a dense table: the count of a tuple is the number of distinct random barcodes seen with it
// (output.rs:265-270).  Writes those counts of the engine's CURRENT key set into its table.  bc_engine_finish does this
// itself for a single-GPU run; a multi-GPU job calls it on every rank after the key exchange (each key then has one
// owner), sums the tables onto the root, and the root's bc_engine_finish compacts the summed table as it stands.
int bc_engine_materialize_table(bc_engine* e) {
  if (!e->h.plan.has_random || e->h.plan.sparse) {
    set_error("bc_engine_materialize_table: the plan has no random barcode with a dense table");
    return BC_ERR_STATE;
  }
  HIP_TRY(hipSetDevice(e->device));
  counts_changed(e);
  {
    const int rc = settle_owed(e);
    if (rc != BC_OK) return rc;
  }
  HIP_TRY(hipMemsetAsync(e->d_table, 0, e->table_entries * 4, e->stream));
  if (e->d_slots) {
    hipLaunchKernelGGL(set_to_table_kernel, dim3(grid_for(e->n_slots)), dim3(256), 0, e->stream, e->d_slots, e->n_slots,
                       e->h.plan.rspace, e->d_table);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->table_materialized = true;
  return BC_OK;
}

int bc_engine_key_count(bc_engine* e, uint64_t* n) {
  *n = 0;
  if (!e->h.plan.has_random || !e->d_slots) return BC_OK;
  return bc_engine_export_keys(e, nullptr, 0, n);
}

int bc_engine_export_keys(bc_engine* e, void* d_keys, uint64_t capacity, uint64_t* n) {
  *n = 0;
  if (!e->h.plan.has_random) {
    set_error("bc_engine_export_keys: the plan has no random barcode");
    return BC_ERR_STATE;
  }
  int rc = bc_engine_sync(e);
  if (rc) return rc;
  if (!e->d_slots) return BC_OK;
  ScratchGuard g;
  unsigned long long* d_n = nullptr;
  HIP_TRY(g.dmalloc(&d_n, 8));
  HIP_TRY(hipMemsetAsync(d_n, 0, 8, e->stream));
  if (e->key_words > 1)
    hipLaunchKernelGGL(wide_export_kernel, dim3(grid_for(e->n_slots)), dim3(256), 0, e->stream, e->d_slots, e->d_ready,
                       (const uint32_t*)nullptr, e->n_slots, e->key_words, d_n, (unsigned long long*)d_keys, (uint32_t*)nullptr,
                       d_keys ? capacity : 0);
  else
    hipLaunchKernelGGL(set_export_kernel, dim3(grid_for(e->n_slots)), dim3(256), 0, e->stream, e->d_slots, e->n_slots, d_n,
                       (unsigned long long*)d_keys, d_keys ? capacity : 0);
  HIP_TRY(hipGetLastError());
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, d_n, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *n = cnt;
  if (d_keys && cnt > capacity) {
    set_error("bc_engine_export_keys: buffer too small");
    return BC_ERR_INVALID;
  }
  return BC_OK;
}

int bc_engine_import_keys(bc_engine* e, const void* d_keys, uint64_t n, uint64_t* n_new) {
  if (n_new) *n_new = 0;
  if (!e->h.plan.has_random) {
    set_error("bc_engine_import_keys: the plan has no random barcode");
    return BC_ERR_STATE;
  }
  if (n == 0) return BC_OK;
  HIP_TRY(hipSetDevice(e->device));
  e->table_materialized = false;
  counts_changed(e);
  int rc = set_reserve(e, n);
  if (rc) return rc;
  ScratchGuard g;
  unsigned long long* d_n = nullptr;
  HIP_TRY(g.dmalloc(&d_n, 8));
  HIP_TRY(hipMemsetAsync(d_n, 0, 8, e->stream));
  if (e->key_words > 1)
    hipLaunchKernelGGL(wide_insert_kernel, dim3(grid_for(n)), dim3(256), 0, e->stream, (const unsigned long long*)d_keys,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, n, e->key_words, e->d_slots, e->d_ready, (uint32_t*)nullptr,
                       e->n_slots - 1, 0, 0u, 0u, d_n);
  else
    hipLaunchKernelGGL(set_insert_kernel, dim3(grid_for(n)), dim3(256), 0, e->stream, (const unsigned long long*)d_keys, n,
                       e->d_slots, e->n_slots - 1, d_n);
  HIP_TRY(hipGetLastError());
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, d_n, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (n_new) *n_new = cnt;
  return BC_OK;
}

// ---- raw-key plans without a random barcode: the counts live in a (key -> count) map -------------
static int need_count_map(bc_engine* e, const char* who) {
  if (!e->h.plan.sparse || e->h.plan.has_random) {
    set_error(std::string(who) + ": the plan does not keep its counts in a key map (it has a dense table or a random barcode)");
    return BC_ERR_STATE;
  }
  return BC_OK;
}

int bc_engine_export_counts(bc_engine* e, void* d_keys, void* d_counts, uint64_t capacity, uint64_t* n) {
  *n = 0;
  int rc = need_count_map(e, "bc_engine_export_counts");
  if (rc) return rc;
  if ((rc = bc_engine_sync(e))) return rc;
  if (!e->d_slots) return BC_OK;
  const bool write = d_keys && d_counts;
  ScratchGuard g;
  unsigned long long* d_n = nullptr;
  HIP_TRY(g.dmalloc(&d_n, 8));
  HIP_TRY(hipMemsetAsync(d_n, 0, 8, e->stream));
  if (e->key_words > 1)
    hipLaunchKernelGGL(wide_export_kernel, dim3(grid_for(e->n_slots)), dim3(256), 0, e->stream, e->d_slots, e->d_ready, e->d_vals,
                       e->n_slots, e->key_words, d_n, (unsigned long long*)(write ? d_keys : nullptr),
                       (uint32_t*)(write ? d_counts : nullptr), write ? capacity : 0);
  else
    hipLaunchKernelGGL(map_export_checked_kernel, dim3(grid_for(e->n_slots)), dim3(256), 0, e->stream, e->d_slots, e->d_vals,
                       e->n_slots, d_n, (unsigned long long*)d_keys, (uint32_t*)d_counts, write ? capacity : 0);
  HIP_TRY(hipGetLastError());
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, d_n, 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *n = cnt;
  if (write && cnt > capacity) {
    set_error("bc_engine_export_counts: buffers too small");
    return BC_ERR_INVALID;
  }
  return BC_OK;
}

int bc_engine_import_counts(bc_engine* e, const void* d_keys, const void* d_counts, uint64_t n) {
  int rc = need_count_map(e, "bc_engine_import_counts");
  if (rc) return rc;
  if (n == 0) return BC_OK;
  if (!d_keys || !d_counts) {
    set_error("bc_engine_import_counts: null buffer");
    return BC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(e->device));
  counts_changed(e);
  if ((rc = set_reserve(e, n))) return rc;
  if (e->key_words > 1)
    hipLaunchKernelGGL(wide_insert_kernel, dim3(grid_for(n)), dim3(256), 0, e->stream, (const unsigned long long*)d_keys,
                       (const uint32_t*)nullptr, (const uint32_t*)d_counts, n, e->key_words, e->d_slots, e->d_ready, e->d_vals,
                       e->n_slots - 1, 0, 0u, 0u, (unsigned long long*)nullptr);
  else
    hipLaunchKernelGGL(map_add_kernel, dim3(grid_for(n)), dim3(256), 0, e->stream, (const unsigned long long*)d_keys,
                       (const uint32_t*)d_counts, n, e->d_slots, e->d_vals, e->n_slots - 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BC_OK;
}

int bc_engine_clear_keys(bc_engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  counts_changed(e);
  return clear_key_table(e);
}

}  // extern "C"

int bc::clear_key_table(bc_engine* e) {
  if (e->d_slots) {
    hipLaunchKernelGGL(set_fill_kernel, dim3(grid_for(e->n_slots * e->key_words)), dim3(256), 0, e->stream, e->d_slots,
                       e->n_slots * e->key_words);
    HIP_TRY(hipGetLastError());
    if (e->d_vals) HIP_TRY(hipMemsetAsync(e->d_vals, 0, e->n_slots * 4, e->stream));
    if (e->d_ready) HIP_TRY(hipMemsetAsync(e->d_ready, 0, e->n_slots * 4, e->stream));
  }
  e->key_bound = 0;
  e->table_materialized = false;
  return BC_OK;
}
