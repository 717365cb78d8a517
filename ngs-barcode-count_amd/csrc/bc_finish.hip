// bc_finish.hip -- the counts out of the engine (include/barcode_count_hip.h): the dense table compacted into sparse
// rows in bounded memory, the rows of a key map, rows as indices or text, and the dense enrichment sums.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "../../include/barcode_count_hip.h"
#include "bc_engine_impl.h"

namespace bc {

// Compaction of the dense table into sparse rows (bc_engine_finish), in two bounded passes.  bits may be NULL; with
// two-level counting the count of entry i is table[i] + bit i: read here as they stand, so an engine-owned table never
// needs the fold pass.
// Pass 1: non-zero entries per block of `block` consecutive entries (one workgroup per block, grid-stride).
__global__ void count_blocks_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ bits, uint64_t n,
                                    uint64_t block, uint64_t n_blocks, uint32_t* __restrict__ per_block) {
  __shared__ uint32_t part[4];
  for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const uint64_t lo = b * block, hi = (lo + block < n) ? lo + block : n;
    uint32_t c = 0;
    for (uint64_t i = lo + threadIdx.x; i < hi; i += blockDim.x)
      c += (table[i] | (bits ? (bits[i >> 5] >> (i & 31)) & 1u : 0u)) != 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) per_block[b] = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
  }
}

// Pass 2: the rows of entries [lo, hi) into a staging buffer the host has sized from pass 1 (one cursor add per
// wavefront; the rows of one range come out in no particular order).
__global__ void compact_range_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ bits, uint64_t lo,
                                     uint64_t hi, unsigned long long* cursor, uint64_t capacity,
                                     uint64_t* __restrict__ out_idx, uint32_t* __restrict__ out_cnt) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  // (every lane of a wavefront runs the same number of rounds: the ballot below needs them all)
  for (uint64_t base = lo + (uint64_t)blockIdx.x * blockDim.x; base < hi; base += step) {
    const uint64_t i = base + threadIdx.x;
    uint32_t v = 0;
    if (i < hi) v = table[i] + (bits ? (bits[i >> 5] >> (i & 31)) & 1u : 0u);
    const unsigned long long m = __ballot(v != 0u);
    if (m == 0ull) continue;
    unsigned long long first = 0;
    if (__lane_id() == 0) first = atomicAdd(cursor, (unsigned long long)__popcll(m));
    first = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(first >> 32)) << 32) |
            (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)first);
    if (v) {
      const unsigned long long p = first + __popcll(m & ((1ull << __lane_id()) - 1ull));
      if (p < capacity) {  // (cannot fail while pass 1 and pass 2 see the same table; a guard, not a path)
        out_idx[p] = i;
        out_cnt[p] = v;
      }
    }
  }
}

}  // namespace bc

using namespace bc;

extern "C" {

// rows of a sparse plan: (tuple key, count) pairs straight out of the hash map
static int finish_sparse(bc_engine* e, uint64_t* n_rows) {
  e->row_idx.clear();
  e->row_cnt.clear();
  if (n_rows) *n_rows = 0;
  e->row_wide.clear();
  if (!e->d_slots) return BC_OK;
  ScratchGuard g;
  // W words per row: a narrow key into row_idx, a wide one (bc_long.h) into row_wide
  const uint32_t W = e->key_words;
  std::vector<uint64_t>& row_key = W > 1 ? e->row_wide : e->row_idx;
  uint64_t* d_key = nullptr;
  uint32_t* d_cnt = nullptr;
  uint64_t n = 0;
  const int rc = W > 1 ? export_wide(e, "bc_engine_finish", g, reinterpret_cast<unsigned long long**>(&d_key), &d_cnt, &n)
                       : export_pairs(e, "bc_engine_finish", g, &d_key, &d_cnt, &n);
  if (rc != BC_OK) return rc;
  try {
    row_key.resize(n * W);
    e->row_cnt.resize(n);
  } catch (const std::bad_alloc&) {
    row_key = std::vector<uint64_t>();
    e->row_cnt = std::vector<uint32_t>();
    set_error("bc_engine_finish: out of host memory for " + std::to_string(n) + " rows");
    return BC_ERR_NOMEM;
  }
  if (n) {
    HIP_TRY(hipMemcpy(row_key.data(), d_key, n * W * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(e->row_cnt.data(), d_cnt, n * 4, hipMemcpyDeviceToHost));
  }
  if (n_rows) *n_rows = n;
  return BC_OK;
}

// Pass 1 of the compaction: the non-zero entries of each block of `block` table entries (bits: the bit map to read
// alongside, or NULL) and their sum.  The device scratch is g's; the stream has drained on return.
static int count_blocks(bc_engine* e, ScratchGuard& g, const uint32_t* bits, uint64_t block, std::vector<uint32_t>* per_block,
                        uint64_t* total) {
  const uint64_t entries = e->table_entries, n_blocks = (entries + block - 1) / block;
  uint32_t* d_per_block = nullptr;
  HIP_TRY(g.dmalloc(&d_per_block, n_blocks * 4));
  hipLaunchKernelGGL(count_blocks_kernel, dim3((uint32_t)std::min<uint64_t>(n_blocks, 256ull * 8)), dim3(256), 0, e->stream,
                     e->d_table, bits, entries, block, n_blocks, d_per_block);
  HIP_TRY(hipGetLastError());
  try {
    per_block->resize(n_blocks);
  } catch (const std::bad_alloc&) {
    set_error("bc_engine_finish: out of host memory");
    return BC_ERR_NOMEM;
  }
  HIP_TRY(hipMemcpyAsync(per_block->data(), d_per_block, n_blocks * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *total = 0;
  for (uint32_t c : *per_block) *total += c;
  return BC_OK;
}

// Dense table -> sparse rows in bounded memory: pass 1 counts the non-zero entries per block of the table, the host
// groups consecutive blocks into ranges of at most `cap` rows, pass 2 compacts range after range into one of two
// staging buffers (device + pinned) while the host takes the previous range's rows.  Device memory: 2 x cap x 12 bytes
// + 4 bytes per block, whatever the table holds (cap: 2^22 rows, BC_FINISH_CHUNK_ROWS).
static int finish_dense(bc_engine* e, const std::function<int(uint64_t)>& on_total,
                        const std::function<int(const uint64_t*, const uint32_t*, uint64_t)>& on_rows, uint64_t* n_rows) {
  if (n_rows) *n_rows = 0;
  const uint64_t entries = e->table_entries;
  if (entries == 0) return on_total(0);
  uint64_t cap = 1ull << 22;
  if (const char* ev = getenv("BC_FINISH_CHUNK_ROWS")) cap = std::max<uint64_t>(256, strtoull(ev, nullptr, 0));
  uint64_t block = 256;
  while (block * 2 <= cap && block < (1ull << 20)) block *= 2;
  const uint64_t n_blocks = (entries + block - 1) / block;
  const uint32_t* bits = e->bits_dirty ? e->d_bits : nullptr;  // two-level counting, not folded: read as they stand
  ScratchGuard g;
  std::vector<uint32_t> per_block;
  uint64_t total = 0;
  int rc = count_blocks(e, g, bits, block, &per_block, &total);
  if (rc != BC_OK) return rc;
  rc = on_total(total);
  if (rc != BC_OK) return rc;
  if (n_rows) *n_rows = total;
  if (total == 0) return BC_OK;

  const uint64_t slot_rows = std::min(cap, total);
  uint64_t* d_idx[2] = {nullptr, nullptr};
  uint32_t* d_cnt[2] = {nullptr, nullptr};
  uint64_t* h_idx[2] = {nullptr, nullptr};
  uint32_t* h_cnt[2] = {nullptr, nullptr};
  hipEvent_t landed[2] = {nullptr, nullptr};
  unsigned long long* d_cursor = nullptr;
  HIP_TRY(g.dmalloc(&d_cursor, 16));
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(g.dmalloc(&d_idx[k], slot_rows * 8));
    HIP_TRY(g.dmalloc(&d_cnt[k], slot_rows * 4));
    HIP_TRY(g.hmalloc(&h_idx[k], slot_rows * 8));
    HIP_TRY(g.hmalloc(&h_cnt[k], slot_rows * 4));
    HIP_TRY(g.event(&landed[k]));
    if (total <= cap) break;  // one range: one slot
  }
  uint64_t pending_rows[2] = {0, 0};
  auto consume = [&](int k) -> int {
    HIP_TRY(hipEventSynchronize(landed[k]));
    return pending_rows[k] ? on_rows(h_idx[k], h_cnt[k], pending_rows[k]) : BC_OK;
  };
  uint64_t b0 = 0;
  int64_t seg = 0;
  while (b0 < n_blocks) {
    // the longest run of blocks from b0 on whose rows fit one slot (a single block always does: block <= cap)
    uint64_t rows = 0, b1 = b0;
    while (b1 < n_blocks && rows + per_block[b1] <= slot_rows) rows += per_block[b1++];
    const int k = (int)(seg & 1);
    if (rows) {
      const uint64_t lo = b0 * block, hi = std::min(entries, b1 * block);
      HIP_TRY(hipMemsetAsync(d_cursor + k, 0, 8, e->stream));
      const uint32_t grid = (uint32_t)std::min<uint64_t>((hi - lo + 255) / 256, 256ull * 32);
      hipLaunchKernelGGL(compact_range_kernel, dim3(grid), dim3(256), 0, e->stream, e->d_table, bits, lo, hi, d_cursor + k,
                         slot_rows, d_idx[k], d_cnt[k]);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(h_idx[k], d_idx[k], rows * 8, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipMemcpyAsync(h_cnt[k], d_cnt[k], rows * 4, hipMemcpyDeviceToHost, e->stream));
    }
    pending_rows[k] = rows;
    HIP_TRY(hipEventRecord(landed[k], e->stream));
    if (seg >= 1 && (rc = consume(k ^ 1)) != BC_OK) {
      (void)hipStreamSynchronize(e->stream);  // nothing of ours may still be writing the staging buffers when they go
      return rc;
    }
    b0 = b1;
    ++seg;
  }
  rc = consume((int)((seg - 1) & 1));
  (void)hipStreamSynchronize(e->stream);
  return rc;
}

// how many rows bc_engine_finish would produce for a dense plan right now (pass 1 alone: one sweep of the table)
int bc_engine_nonzero_entries(bc_engine* e, uint64_t* n) {
  *n = 0;
  if (e->h.plan.sparse || e->h.plan.has_random) {
    set_error("bc_engine_nonzero_entries: only for plans that count into a dense table directly");
    return BC_ERR_STATE;
  }
  int rc = bc_engine_sync(e);
  if (rc) return rc;
  if (!e->table_entries) return BC_OK;
  ScratchGuard g;
  std::vector<uint32_t> per_block;
  return count_blocks(e, g, e->bits_dirty ? e->d_bits : nullptr, 1ull << 20, &per_block, n);
}

}  // extern "C"

int bc::dense_counts_ready(bc_engine* e) {
  int rc = bc_engine_sync(e);
  if (rc) return rc;
  if (e->h.plan.has_random && !e->table_materialized) return bc_engine_materialize_table(e);
  return BC_OK;
}

extern "C" {

// rows of either kind of plan, chunk by chunk (bc_engine_finish_stream); for sparse plans the chunks are cut from the
// exported map
static int finish_any(bc_engine* e, const std::function<int(uint64_t)>& on_total,
                      const std::function<int(const uint64_t*, const uint32_t*, uint64_t)>& on_rows, uint64_t* n_rows) {
  int rc;
  if (e->h.plan.sparse) {
    if ((rc = bc_engine_sync(e)) != BC_OK) return rc;
    uint64_t n = 0;
    if ((rc = finish_sparse(e, &n)) != BC_OK) return rc;
    if (n_rows) *n_rows = n;
    return BC_OK;  // (finish_sparse leaves the rows in e->row_idx / row_cnt; the callers below hand them on)
  }
  if ((rc = dense_counts_ready(e)) != BC_OK) return rc;
  return finish_dense(e, on_total, on_rows, n_rows);
}

int bc_engine_finish(bc_engine* e, uint64_t* n_rows) {
  if (n_rows) *n_rows = 0;
  e->row_idx.clear();
  e->row_cnt.clear();
  uint64_t at = 0;
  auto on_total = [&](uint64_t total) -> int {
    try {
      e->row_idx.resize(total);
      e->row_cnt.resize(total);
    } catch (const std::bad_alloc&) {
      e->row_idx = std::vector<uint64_t>();
      e->row_cnt = std::vector<uint32_t>();
      set_error("bc_engine_finish: out of host memory for " + std::to_string(total) +
                " rows (bc_engine_finish_stream hands the rows over in chunks instead)");
      return BC_ERR_NOMEM;
    }
    return BC_OK;
  };
  auto on_rows = [&](const uint64_t* idx, const uint32_t* cnt, uint64_t n) -> int {
    staged_copy(e->row_idx.data() + at, idx, n * 8);
    staged_copy(e->row_cnt.data() + at, cnt, n * 4);
    at += n;
    return BC_OK;
  };
  const int rc = finish_any(e, on_total, on_rows, n_rows);
  if (rc != BC_OK) {
    e->row_idx.clear();
    e->row_cnt.clear();
    if (n_rows) *n_rows = 0;
  }
  return rc;
}

int bc_engine_finish_stream(bc_engine* e, bc_rows_fn fn, void* user, uint64_t* n_rows) {
  if (!fn) {
    set_error("bc_engine_finish_stream: null callback");
    return BC_ERR_INVALID;
  }
  if (n_rows) *n_rows = 0;
  e->row_idx.clear();
  e->row_cnt.clear();
  auto on_total = [&](uint64_t) -> int { return BC_OK; };
  auto on_rows = [&](const uint64_t* idx, const uint32_t* cnt, uint64_t n) -> int {
    if (fn(idx, cnt, n, user) != 0) {
      set_error("bc_engine_finish_stream: stopped by the callback");
      return BC_ERR_STATE;
    }
    return BC_OK;
  };
  uint64_t n = 0;
  int rc = finish_any(e, on_total, on_rows, &n);
  if (rc != BC_OK) return rc;
  if (e->h.plan.sparse && e->key_words > 1) {
    e->row_wide.clear();
    e->row_cnt.clear();
    set_error("bc_engine_finish_stream: the plan's keys are " + std::to_string(e->key_words) +
              " words wide; read its rows with bc_engine_finish + bc_engine_row_text");
    return BC_ERR_UNSUPPORTED;
  }
  if (e->h.plan.sparse) {
    // a key map's rows are already on the host (finish_sparse): hand them on in slices, then drop them
    const uint64_t slice = 1ull << 20;
    for (uint64_t a = 0; a < n && rc == BC_OK; a += slice)
      rc = on_rows(e->row_idx.data() + a, e->row_cnt.data() + a, std::min(slice, n - a));
    e->row_idx.clear();
    e->row_cnt.clear();
  }
  if (rc == BC_OK && n_rows) *n_rows = n;
  return rc;
}

int bc_engine_decode_index(const bc_engine* e, uint64_t dense_index, uint32_t* sample_idx, uint32_t* barcode_idx) {
  const DevPlan& P = e->h.plan;
  if (P.sparse) {
    set_error("bc_engine_decode_index: the plan keeps raw captures, whose keys are not indices");
    return BC_ERR_STATE;
  }
  const uint32_t g0 = e->has_sample_group ? 1u : 0u;
  uint64_t di = dense_index;
  for (int b = (int)e->barcode_num - 1; b >= 0; --b) {
    const uint32_t nr = P.groups[g0 + b].n_refs;
    if (barcode_idx) barcode_idx[b] = (uint32_t)(di % nr);
    di /= nr;
  }
  if (sample_idx) *sample_idx = (uint32_t)di;
  return BC_OK;
}

}  // extern "C"

bool bc::enrich_shape(const bc_engine* e, const char* who, EnrichShape* sh, uint64_t* n_samples) {
  const DevPlan& P = e->h.plan;
  if (P.sparse) {
    set_error(std::string(who) + ": the plan keeps raw captures, whose keys are sequences, not indices: enrich its rows "
              "(bc_engine_row_text) on the host");
    return false;
  }
  if (e->barcode_num > (uint32_t)kEnrichMaxG) {  // (cannot happen: a plan has at most kMaxGroups groups)
    set_error(std::string(who) + ": more counted barcodes than the enrichment kernel takes");
    return false;
  }
  memset(sh, 0, sizeof(*sh));
  sh->G = e->barcode_num;
  const uint32_t g0 = e->has_sample_group ? 1u : 0u;
  sh->inner = 1;
  for (uint32_t g = 0; g < sh->G; ++g) {
    sh->n[g] = P.groups[g0 + g].n_refs;
    sh->single_off[g] = sh->sum_n;
    sh->sum_n += sh->n[g];
    sh->inner *= sh->n[g];
  }
  if (sh->G >= 3)  // (the reference writes Double files only then, output.rs:176, 349)
    for (uint32_t g = 0; g + 1 < sh->G; ++g)
      for (uint32_t h = g + 1; h < sh->G; ++h) {
        sh->pair_off[enrich_pair_index((int)sh->G, (int)g, (int)h)] = sh->pairs;
        sh->pairs += (uint64_t)sh->n[g] * sh->n[h];
      }
  *n_samples = sh->inner ? e->table_entries / sh->inner : 0;
  return true;
}

extern "C" {

int bc_engine_enrich_entries(const bc_engine* e, uint64_t* single_entries, uint64_t* double_entries) {
  EnrichShape sh;
  uint64_t S = 0;
  if (!enrich_shape(e, "bc_engine_enrich_entries", &sh, &S)) return BC_ERR_UNSUPPORTED;
  if (single_entries) *single_entries = S * sh.sum_n;
  if (double_entries) *double_entries = S * sh.pairs;
  return BC_OK;
}

// Single and pair counts as marginal sums of the dense table, in one pass over it on the device (bc_enrich.hip).  The
// table, the bit map and the rows stay as they are.
int bc_engine_enrich(bc_engine* e, uint64_t* single_counts, uint64_t* double_counts) {
  EnrichShape sh;
  uint64_t S = 0;
  if (!enrich_shape(e, "bc_engine_enrich", &sh, &S)) return BC_ERR_UNSUPPORTED;
  const uint64_t n_single = S * sh.sum_n, n_double = double_counts ? S * sh.pairs : 0;
  if (n_single && !single_counts) {
    set_error("bc_engine_enrich: single_counts is NULL");
    return BC_ERR_INVALID;
  }
  int rc = dense_counts_ready(e);
  if (rc) return rc;
  if (n_single == 0) return BC_OK;
  ScratchGuard g;
  unsigned long long *d_single = nullptr, *d_double = nullptr;
  HIP_TRY(g.dmalloc(&d_single, n_single * 8));
  if (n_double) HIP_TRY(g.dmalloc(&d_double, n_double * 8));
  HIP_TRY(hipMemsetAsync(d_single, 0, n_single * 8, e->stream));
  if (n_double) HIP_TRY(hipMemsetAsync(d_double, 0, n_double * 8, e->stream));
  HIP_TRY(bc_enrich_launch(sh, e->d_table, e->bits_dirty ? e->d_bits : nullptr, e->table_entries, d_single, d_double,
                           e->stream));
  HIP_TRY(hipMemcpyAsync(single_counts, d_single, n_single * 8, hipMemcpyDeviceToHost, e->stream));
  if (n_double) HIP_TRY(hipMemcpyAsync(double_counts, d_double, n_double * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return BC_OK;
}

int bc_engine_rows(bc_engine* e, uint64_t first, uint64_t n, uint32_t* sample_idx, uint32_t* barcode_idx,
                   uint64_t* count) {
  if (first + n > e->row_idx.size()) {
    set_error("bc_engine_rows: range outside the compacted rows (call bc_engine_finish first)");
    return BC_ERR_STATE;
  }
  const DevPlan& P = e->h.plan;
  if (P.sparse) {
    set_error("bc_engine_rows: the plan keeps raw captures, which have no index; use bc_engine_row_text");
    return BC_ERR_STATE;
  }
  const uint32_t nb = e->barcode_num ? e->barcode_num : 1;
  const uint32_t g0 = e->has_sample_group ? 1u : 0u;  // groups[0] is the sample group when present
  for (uint64_t r = 0; r < n; ++r) {
    uint64_t di = e->row_idx[first + r];
    for (int b = (int)e->barcode_num - 1; b >= 0; --b) {
      const uint32_t nr = P.groups[g0 + b].n_refs;
      barcode_idx[r * nb + b] = (uint32_t)(di % nr);
      di /= nr;
    }
    sample_idx[r] = (uint32_t)di;
    count[r] = e->row_cnt[first + r];
  }
  return BC_OK;
}

int bc_engine_row_text(bc_engine* e, uint64_t row, char* sample, size_t sample_cap, char* tuple, size_t tuple_cap,
                       uint64_t* count) {
  if (row >= e->row_cnt.size() || (e->key_words == 1 && row >= e->row_idx.size())) {
    set_error("bc_engine_row_text: row outside the compacted rows (call bc_engine_finish first)");
    return BC_ERR_STATE;
  }
  const DevPlan& P = e->h.plan;
  std::string s_out = "barcode", t_out;  // parse.rs:473: the sample key without a sample group
  std::vector<std::string> parts(P.n_groups);
  if (e->key_words > 1) {
    // wide key (bc_long.h): every group's field read back from the payload bits
    const uint64_t* key = &e->row_wide[row * e->key_words];
    auto bit = [&](uint32_t at) { return (uint32_t)((key[1u + (at >> 6)] >> (at & 63u)) & 1ull); };
    for (uint32_t g = 0; g < P.n_groups; ++g) {
      const LongGroup& G = e->lh.plan.groups[g];
      if (G.n_refs) {
        uint32_t idx = 0;
        for (uint32_t b = 0; b < 32u; ++b) idx |= bit(G.key_bit + b) << b;
        parts[g] = idx < e->set_seqs[g].size() ? e->set_seqs[g][idx] : std::string("?");
      } else {
        std::string v;
        for (uint32_t i = 0; i < G.len; ++i) {
          const uint32_t b1 = bit(G.key_bit + i), b2 = bit(G.key_bit + G.len + i), bn = bit(G.key_bit + 2u * G.len + i);
          v.push_back(bn ? 'N' : "ACTG"[b1 | (b2 << 1)]);
        }
        parts[g] = v;
      }
    }
  }
  uint64_t key = e->key_words > 1 ? 0 : e->row_idx[row];
  for (int g = (int)P.n_groups - 1; g >= 0 && e->key_words == 1; --g) {
    const DevGroup& G = P.groups[g];
    std::string v;
    if (G.mode == kSetNone) {
      uint64_t radix = 1;
      for (uint32_t k = 0; k < G.len; ++k) radix *= 5;
      uint64_t code = key % radix;
      key /= radix;
      for (uint32_t k = 0; k < G.len; ++k) {
        v.push_back("ACTGN"[code % 5]);
        code /= 5;
      }
    } else {
      const uint32_t idx = (uint32_t)(key % G.n_refs);
      key /= G.n_refs;
      v = e->set_seqs[g][idx];
    }
    parts[g] = v;
  }
  for (uint32_t g = 0; g < P.n_groups; ++g) {
    if (P.groups[g].type == kGroupSample)
      s_out = parts[g];
    else
      t_out += (t_out.empty() ? "" : ",") + parts[g];
  }
  if (s_out.size() + 1 > sample_cap || t_out.size() + 1 > tuple_cap) {
    set_error("bc_engine_row_text: buffer too small");
    return BC_ERR_INVALID;
  }
  memcpy(sample, s_out.c_str(), s_out.size() + 1);
  memcpy(tuple, t_out.c_str(), t_out.size() + 1);
  if (count) *count = e->row_cnt[row];
  return BC_OK;
}

}  // extern "C"
