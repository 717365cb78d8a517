// bc_text.hip -- the output files written as CSV text on the device, five renderers:
//   counts of a dense plan        bc_engine_render_counts / _merged            bc_render.h
//   counts of a raw-key plan      bc_engine_render_raw_counts / _merged        bc_raw_render.h, bc_sort.h
//   counts of a wide-key plan     bc_engine_render_wide_counts / _merged       bc_wide_render.h, bc_sort.h
//   Single / Double, dense plan   bc_engine_render_enriched / _merged          bc_enrich_render.h
//   Single / Double, raw-key plan bc_engine_render_raw_enriched / _merged      bc_raw_enrich_render.h, bc_sort.h, bc_reduce.h
// A renderer is a view struct with lane code (written with bc_line.h) and a front end here that checks the request,
// has what the view reads made or served from the engine (the structs of bc_engine_impl.h, kept under the counts
// epoch) and fills the view.  What the front ends share comes first: the label pool, the host loop around the kernels
// of bc_text_kernels.h (stream_text; both templates over the view), the refusals, the description of a sparse plan's
// counted groups, the longest line, and the closing call (render_lines).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "bc_engine_impl.h"
#include "bc_enrich_render.h"
#include "bc_raw_enrich_render.h"
#include "bc_raw_render.h"
#include "bc_reduce.h"
#include "bc_render.h"
#include "bc_sort.h"
#include "bc_text_kernels.h"
#include "bc_wide_render.h"

using namespace bc;

// ---- what the renderers share ----

// The IDs of the counted sets on the device, once per engine: per group N_g + 1 offsets, and the bytes back to back.
static int ensure_render_pool(bc_engine* e, const char* who) {
  if (e->labels.ready) return BC_OK;
  const uint32_t G = e->barcode_num;
  std::vector<uint32_t> off;
  std::string bytes;
  try {
    for (uint32_t g = 0; g < G; ++g) {
      e->labels.off_start[g] = (uint32_t)off.size();
      e->labels.max_len[g] = 0;
      const uint32_t n = bc_plan_n_counted(e->src_plan, g);
      for (uint32_t i = 0; i < n; ++i) {
        const char* id = bc_plan_counted_id(e->src_plan, g, i);
        const size_t len = id ? strlen(id) : 0;
        if (bytes.size() + len > 0xFFFFFFF0ull || off.size() > 0xFFFFFFF0ull) {
          set_error(std::string(who) + ": the IDs of the counted barcodes pass 4 GB");
          return BC_ERR_UNSUPPORTED;
        }
        off.push_back((uint32_t)bytes.size());
        if (len) bytes.append(id, len);
        e->labels.max_len[g] = std::max<uint32_t>(e->labels.max_len[g], (uint32_t)len);
      }
      off.push_back((uint32_t)bytes.size());
    }
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return BC_ERR_NOMEM;
  }
  HIP_TRY(hipSetDevice(e->device));
  // both parts in one allocation (offsets first: the bytes need no alignment), so a failure leaves nothing behind
  const size_t off_bytes = off.size() * 4;
  std::string image;
  try {
    image.assign((const char*)off.data(), off_bytes);
    image += bytes;
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return BC_ERR_NOMEM;
  }
  void* d_pool = nullptr;
  HIP_TRY(hipMalloc(&d_pool, image.size() ? image.size() : 16));
  if (!image.empty()) {
    const hipError_t hrc = hipMemcpy(d_pool, image.data(), image.size(), hipMemcpyHostToDevice);
    if (hrc != hipSuccess) {
      (void)hipFree(d_pool);
      HIP_TRY(hrc);
    }
  }
  try {
    e->allocs.push_back(d_pool);
  } catch (const std::bad_alloc&) {
    (void)hipFree(d_pool);
    set_error(std::string(who) + ": out of host memory");
    return BC_ERR_NOMEM;
  }
  e->labels.d_off = (uint32_t*)d_pool;
  e->labels.d_bytes = (uint8_t*)d_pool + off_bytes;
  e->labels.ready = true;
  return BC_OK;
}

// The lines of the keys [0, n_keys) that have one, in ascending key order, handed to `fn` in chunks that end with a
// line.  Pass 1 sizes every block of the key space, the host scans the sizes and cuts the space into ranges whose text
// fits one staging buffer, pass 2 writes range after range into one of two buffers (device + pinned) while the host hands
// on the range before.  A block whose text passes the buffer is cut between its lines from their lengths.  Device
// memory: 2 x buffer + 12 bytes per block of 1024 keys.  max_line: no line is longer.
template <class View>
static int stream_text(bc_engine* e, const char* who, const View& v, uint64_t max_line, bc_text_fn fn, void* user,
                       uint64_t* n_rows) {
  const uint64_t n_keys = text_keys(v);
  uint64_t cap = 64ull << 20;
  if (const char* ev = getenv("BC_RENDER_CHUNK_BYTES")) {  // (a value that does not parse, or 0, leaves the default)
    char* end = nullptr;
    const unsigned long long x = strtoull(ev, &end, 0);
    if (end != ev && *end == '\0' && x > 0) cap = x;
  }
  cap = std::max(cap, max_line);  // never smaller than the longest possible line: every line fits some chunk

  ScratchGuard g;
  const uint64_t n_blocks = (n_keys + kRenderBlock - 1) / kRenderBlock;
  uint32_t* d_rows = nullptr;
  unsigned long long* d_bytes = nullptr;
  HIP_TRY(g.dmalloc(&d_rows, n_blocks * 4));
  HIP_TRY(g.dmalloc(&d_bytes, (n_blocks + 1) * 8));
  HIP_TRY(hipMemsetAsync(d_rows, 0, n_blocks * 4, e->stream));
  HIP_TRY(hipMemsetAsync(d_bytes, 0, (n_blocks + 1) * 8, e->stream));
  HIP_TRY(text_sizes_launch(v, n_blocks, d_rows, d_bytes, e->stream));
  std::vector<uint32_t> rows;
  std::vector<unsigned long long> prefix;
  try {
    rows.resize(n_blocks);
    prefix.resize(n_blocks + 1);
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return BC_ERR_NOMEM;
  }
  HIP_TRY(hipMemcpyAsync(rows.data(), d_rows, n_blocks * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemcpyAsync(prefix.data(), d_bytes, n_blocks * 8, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  uint64_t total_rows = 0, total_bytes = 0;
  for (uint64_t b = 0; b < n_blocks; ++b) {  // sizes -> exclusive scan, in place
    const uint64_t x = prefix[b];
    prefix[b] = total_bytes;
    total_bytes += x;
    total_rows += rows[b];
  }
  prefix[n_blocks] = total_bytes;
  if (total_rows == 0) return BC_OK;
  HIP_TRY(hipMemcpyAsync(d_bytes, prefix.data(), (n_blocks + 1) * 8, hipMemcpyHostToDevice, e->stream));

  const uint64_t slot = std::min(cap, total_bytes);
  const size_t slot_alloc = (size_t)((slot + 3) & ~3ull);
  uint8_t* d_text[2] = {nullptr, nullptr};
  uint8_t* h_text[2] = {nullptr, nullptr};
  hipEvent_t landed[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(g.dmalloc(&d_text[k], slot_alloc));
    HIP_TRY(g.hmalloc(&h_text[k], slot_alloc));
    HIP_TRY(g.event(&landed[k]));
    if (total_bytes <= cap) break;  // one range: one slot
  }
  uint32_t *d_len = nullptr, *h_len = nullptr;  // a block's line lengths, when one has to be cut inside
  uint64_t pending[2] = {0, 0};
  auto consume = [&](int k) -> int {
    HIP_TRY(hipEventSynchronize(landed[k]));
    if (pending[k] && fn((const char*)h_text[k], (size_t)pending[k], user) != 0) {
      set_error(std::string(who) + ": stopped by the callback");
      return BC_ERR_STATE;
    }
    return BC_OK;
  };
  int64_t seg = 0;
  // one range: the lines of tuples [lo, hi) inside blocks [b0, b1), `bytes` of text that starts at scan position `sub`
  auto emit = [&](uint64_t b0, uint64_t b1, uint64_t lo, uint64_t hi, uint64_t sub, uint64_t bytes) -> int {
    const int k = (int)(seg & 1);
    if (bytes) {
      HIP_TRY(text_write_launch(v, b0, b1 - b0, lo, hi, d_rows, d_bytes, sub, d_text[k], slot, e->stream));
      HIP_TRY(hipMemcpyAsync(h_text[k], d_text[k], bytes, hipMemcpyDeviceToHost, e->stream));
    }
    pending[k] = bytes;
    HIP_TRY(hipEventRecord(landed[k], e->stream));
    int r2 = BC_OK;
    if (seg >= 1) r2 = consume(k ^ 1);
    ++seg;
    return r2;
  };
  auto run = [&]() -> int {
    uint64_t b0 = 0;
    while (b0 < n_blocks) {
      uint64_t b1 = b0;
      while (b1 < n_blocks && prefix[b1 + 1] - prefix[b0] <= slot) ++b1;
      int r2;
      if (b1 > b0) {
        if (prefix[b1] == prefix[b0]) {  // (nothing but empty blocks)
          b0 = b1;
          continue;
        }
        r2 = emit(b0, b1, b0 * kRenderBlock, std::min<uint64_t>(n_keys, b1 * kRenderBlock), prefix[b0], prefix[b1] - prefix[b0]);
        if (r2 != BC_OK) return r2;
        b0 = b1;
        continue;
      }
      // block b0 alone passes the buffer: cut it between its lines
      if (!d_len) {
        HIP_TRY(g.dmalloc(&d_len, kRenderBlock * 4));
        HIP_TRY(g.hmalloc(&h_len, kRenderBlock * 4));
      }
      const uint64_t t0 = b0 * kRenderBlock;
      const uint32_t n = (uint32_t)std::min<uint64_t>(kRenderBlock, n_keys - t0);
      HIP_TRY(text_lens_launch(v, t0, n, d_len, e->stream));
      HIP_TRY(hipMemcpyAsync(h_len, d_len, n * 4, hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(hipStreamSynchronize(e->stream));
      uint32_t len[kRenderBlock];  // (a copy: h_len is reused by a later block while ranges are in flight)
      memcpy(len, h_len, n * 4);
      uint32_t i = 0;
      while (i < n) {
        uint64_t bytes = 0;
        uint32_t j = i;
        while (j < n && bytes + len[j] <= slot) bytes += len[j++];  // (a line always fits: slot >= max_line)
        if (bytes && (r2 = emit(b0, b0 + 1, t0 + i, t0 + j, prefix[b0], bytes)) != BC_OK) return r2;
        i = j;
      }
      ++b0;
    }
    return seg ? consume((int)((seg - 1) & 1)) : BC_OK;
  };
  const int rc = run();
  (void)hipStreamSynchronize(e->stream);  // nothing of ours may still be writing the staging buffers when they go
  if (rc == BC_OK && n_rows) *n_rows = total_rows;
  return rc;
}

// What every front end refuses after its plan's shape: no callback, a sample list that is not there, a sample that the
// plan does not have (S of them).
static int check_request(const char* who, const uint32_t* cols, uint32_t n_cols, bc_text_fn fn, uint64_t S) {
  if (!fn || (n_cols && !cols)) {
    set_error(std::string(who) + ": null callback or sample list");
    return BC_ERR_INVALID;
  }
  for (uint32_t c = 0; c < n_cols; ++c)
    if (cols[c] >= S) {
      set_error(std::string(who) + ": sample index " + std::to_string(cols[c]) + " of " + std::to_string(S));
      return BC_ERR_INVALID;
    }
  return BC_OK;
}

static int check_max_line(const char* who, uint64_t max_line) {
  if (max_line > kRenderMaxLine) {
    set_error(std::string(who) + ": a line could be " + std::to_string(max_line) + " bytes long; the renderer takes " +
              std::to_string(kRenderMaxLine));
    return BC_ERR_UNSUPPORTED;
  }
  return BC_OK;
}

// the sample columns on the device, for the render's lifetime
static int upload_cols(bc_engine* e, ScratchGuard& g, const uint32_t* cols, uint32_t n_cols, uint32_t*& d_cols) {
  HIP_TRY(g.dmalloc(&d_cols, (size_t)n_cols * 4));
  HIP_TRY(hipMemcpyAsync(d_cols, cols, (size_t)n_cols * 4, hipMemcpyHostToDevice, e->stream));
  return BC_OK;
}

// What a front end renders, for the refusals below.  (The dense enrichment refuses through enrich_shape.)
enum TextFamily { kDenseCounts, kRawCounts, kWideCounts, kRawEnrich };

// The engine's plan is one of: dense; sparse with one-word keys (raw); sparse with wider keys (wide); and a sparse plan
// may keep its sample barcode raw, which no renderer takes.  BC_OK when `fam` renders that, else its refusal.
static int check_plan_shape(const bc_engine* e, const char* who, TextFamily fam) {
  const DevPlan& P = e->h.plan;
  const bool enrich = fam == kRawEnrich;
  std::string why;
  if (fam == kDenseCounts) {
    if (P.sparse)
      why = "the plan keeps raw captures, whose rows are sequences, not indices: write them from bc_engine_row_text on the host";
  } else if (!P.sparse) {
    why = enrich ? "the plan has a dense table: its Single / Double files come from bc_engine_render_enriched / "
                   "bc_engine_render_enriched_merged"
                 : "the plan has a dense table: its files come from bc_engine_render_counts / bc_engine_render_merged";
  } else if (fam != kWideCounts && e->key_words > 1) {
    why = "the plan's keys are " + std::to_string(e->key_words) + " words wide; " +
          (enrich ? "build its Single / Double files" : "write its rows") + " from bc_engine_finish + bc_engine_row_text on the host";
  } else if (e->has_sample_group && P.groups[0].mode == kSetNone) {
    why = std::string("the sample barcode is kept raw, so a sample is a capture, not an index: ") +
          (enrich ? "build the Single / Double files" : "write the rows") + " from bc_engine_finish + bc_engine_row_text on the host";
  } else if (fam == kWideCounts && e->key_words <= 1) {
    why = "the plan's keys are one word wide: its files come from bc_engine_render_raw_counts / bc_engine_render_raw_merged";
  }
  if (why.empty()) return BC_OK;
  set_error(std::string(who) + ": " + why);
  return BC_ERR_UNSUPPORTED;
}

static int check_kind(const char* who, int kind) {
  if (kind == BC_ENRICH_SINGLE || kind == BC_ENRICH_DOUBLE) return BC_OK;
  set_error(std::string(who) + ": kind " + std::to_string(kind) + " is neither BC_ENRICH_SINGLE nor BC_ENRICH_DOUBLE");
  return BC_ERR_INVALID;
}

// counted set g still has the n entries the table's axes / the key's digits were made for (it cannot be otherwise)
static int check_set_size(const bc_engine* e, const char* who, uint32_t g, uint32_t n) {
  if (bc_plan_n_counted(e->src_plan, g) == n) return BC_OK;
  set_error(std::string(who) + ": the plan's sets changed after the engine was created");
  return BC_ERR_STATE;
}

// The counted groups of a sparse plan, as its views read them.  The caller gives G and, per group, raw_len (bases of a
// raw capture; 0: a known set) and n_ids (the set's size); describe_groups adds the rest once the label pool is ready.
struct CountedGroups {
  uint32_t G;
  uint32_t raw_len[bc::kRenderMaxG];
  uint32_t n_ids[bc::kRenderMaxG];
  uint32_t off_start[bc::kRenderMaxG];  // known set: where its offsets start in the label pool
  uint32_t longest[bc::kRenderMaxG];    // bytes of the group's longest field
  uint64_t radix[bc::kRenderMaxG];      // the set's size, or 5^raw_len (past 27 bases it wraps: wide keys have no radix)
};

static int describe_groups(const bc_engine* e, const char* who, CountedGroups& cg) {
  for (uint32_t g = 0; g < cg.G; ++g) {
    cg.off_start[g] = 0;
    if (cg.raw_len[g]) {
      cg.longest[g] = cg.raw_len[g];
      cg.radix[g] = 1;
      for (uint32_t k = 0; k < cg.raw_len[g]; ++k) cg.radix[g] *= 5;
      continue;
    }
    const int rc = check_set_size(e, who, g, cg.n_ids[g]);
    if (rc != BC_OK) return rc;
    cg.radix[g] = cg.n_ids[g];
    cg.off_start[g] = e->labels.off_start[g];
    cg.longest[g] = e->labels.max_len[g];
  }
  return BC_OK;
}

// a one-word sparse plan's counted groups (they follow the sample group, when there is one): G, raw_len, n_ids
static int raw_plan_groups(const bc_engine* e, const char* who, CountedGroups& cg) {
  const DevPlan& P = e->h.plan;
  const uint32_t g0 = e->has_sample_group ? 1u : 0u;
  memset(&cg, 0, sizeof cg);
  cg.G = e->barcode_num;
  if (cg.G > (uint32_t)bc::kRenderMaxG || g0 + cg.G > P.n_groups) {  // (cannot happen: a plan's groups fit the view)
    set_error(std::string(who) + ": the plan's groups do not fit the view");
    return BC_ERR_STATE;
  }
  for (uint32_t g = 0; g < cg.G; ++g) {
    const DevGroup& Gr = P.groups[g0 + g];
    if (Gr.mode == kSetNone)
      cg.raw_len[g] = Gr.len;
    else
      cg.n_ids[g] = Gr.n_refs;
  }
  return BC_OK;
}

// the longest a counts line can be: every group's longest field, the commas, '\n', and ",4294967295" per column
static uint64_t counts_max_line(uint32_t G, const uint32_t* longest, uint32_t n_cols) {
  uint64_t max_line = 1 + (G ? G - 1 : 0) + 11ull * n_cols;
  for (uint32_t g = 0; g < G; ++g) max_line += longest[g];
  return max_line;
}

// ... and a Single (Double) line: the longest field (the two longest of different groups), G - 1 commas, '\n', and a
// comma and 20 digits per column
static uint64_t enrich_max_line(uint32_t G, const uint32_t* longest, uint32_t n_cols, int kind) {
  uint32_t top[2] = {0, 0};
  for (uint32_t g = 0; g < G; ++g) {
    const uint32_t m = longest[g];
    if (m > top[0]) {
      top[1] = top[0];
      top[0] = m;
    } else if (m > top[1]) {
      top[1] = m;
    }
  }
  return 1 + (G - 1) + 21ull * n_cols + top[0] + (kind == BC_ENRICH_DOUBLE ? top[1] : 0u);
}

// How every front end ends, its view filled but for the columns and the label pool (which is ready): the lines of the
// keys that have one go to `fn` (stream_text).
template <class View>
static int render_lines(bc_engine* e, const char* who, View& v, uint64_t max_line, const uint32_t* cols, uint32_t n_cols,
                        bc_text_fn fn, void* user, uint64_t* n_rows) {
  int rc = check_max_line(who, max_line);
  if (rc != BC_OK) return rc;
  HIP_TRY(hipSetDevice(e->device));
  ScratchGuard g;
  uint32_t* d_cols = nullptr;
  if ((rc = upload_cols(e, g, cols, n_cols, d_cols)) != BC_OK) return rc;
  v.cols = d_cols;
  v.n_cols = n_cols;
  v.label_off = e->labels.d_off;
  v.label_bytes = e->labels.d_bytes;
  return stream_text(e, who, v, max_line, fn, user, n_rows);
}

// ---- counts of a dense plan as text (bc_render.h) ----

// The lines of the tuples for which some listed sample counts, in ascending tuple order (stream_text).
static int render_text(bc_engine* e, const char* who, const uint32_t* cols, uint32_t n_cols, bc_text_fn fn, void* user,
                       uint64_t* n_rows) {
  if (n_rows) *n_rows = 0;
  int rc = check_plan_shape(e, who, kDenseCounts);
  if (rc) return rc;
  static_assert(bc::kRenderMaxG >= kMaxGroups, "a plan's counted barcodes fit the view");
  bc::RenderView v;
  memset(&v, 0, sizeof v);
  v.G = e->barcode_num;
  v.T = 1;
  const uint32_t g0 = e->has_sample_group ? 1u : 0u;
  for (uint32_t g = 0; g < v.G; ++g) {
    v.n[g] = e->h.plan.groups[g0 + g].n_refs;
    v.T *= v.n[g];
  }
  const uint64_t S = v.T ? e->table_entries / v.T : 0;
  if ((rc = check_request(who, cols, n_cols, fn, S)) != BC_OK) return rc;
  if ((rc = dense_counts_ready(e)) != BC_OK) return rc;
  if (n_cols == 0 || v.T == 0 || e->table_entries == 0) return BC_OK;
  if ((rc = ensure_render_pool(e, who)) != BC_OK) return rc;
  for (uint32_t g = 0; g < v.G; ++g) {
    if ((rc = check_set_size(e, who, g, v.n[g])) != BC_OK) return rc;
    v.off_start[g] = e->labels.off_start[g];
  }
  v.table = e->d_table;
  v.bits = e->bits_dirty ? e->d_bits : nullptr;  // two-level counting, not folded: read as they stand
  return render_lines(e, who, v, counts_max_line(v.G, e->labels.max_len, n_cols), cols, n_cols, fn, user, n_rows);
}

extern "C" {

int bc_engine_render_counts(bc_engine* e, uint32_t sample_idx, bc_text_fn fn, void* user, uint64_t* n_rows) {
  return render_text(e, "bc_engine_render_counts", &sample_idx, 1, fn, user, n_rows);
}

int bc_engine_render_merged(bc_engine* e, const uint32_t* sample_idx, uint32_t n_samples, bc_text_fn fn, void* user,
                            uint64_t* n_rows) {
  return render_text(e, "bc_engine_render_merged", sample_idx, n_samples, fn, user, n_rows);
}

}  // extern "C"

// ---- counts of a raw-key plan as text (bc_raw_render.h, bc_sort.h) ----

namespace bc {

// key = s * t_space + T  ->  T * S + s: the same digits, the sample's moved to the least significant place
__global__ __launch_bounds__(256) void raw_rekey_kernel(unsigned long long* __restrict__ keys, uint64_t n, uint64_t t_space,
                                                        uint32_t S) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = keys[i];
    const unsigned long long s = k / t_space;
    keys[i] = (k - s * t_space) * S + s;
  }
}

}  // namespace bc

// keys[i] = s * t_space + T  (the engine's key: the sample group, when there is one, is its most significant digit)
//   ->  T * S + s,  in place; S == 1: nothing to do, and nothing is launched
static hipError_t raw_rekey_launch(uint64_t* d_keys, uint64_t n, uint64_t t_space, uint32_t S, hipStream_t stream) {
  if (n == 0 || S <= 1 || t_space == 0) return hipSuccess;
  hipLaunchKernelGGL(raw_rekey_kernel, dim3(grid_for(n)), dim3(256), 0, stream, (unsigned long long*)d_keys, n, t_space, S);
  return hipGetLastError();
}

// (the enrichment segments are made from the sorted rows: they go together)
static void raw_sorted_drop(bc_engine* e) {
  for (RawEnrichSegs& r : e->raw_enrich) r.drop();
  e->raw_rows.drop();
}

// The pairs of the current counts, sorted into the order of the files, in e->raw_rows: served as they are while the
// counts epoch stands, else exported from the map (export_pairs, as finish_sparse does), re-keyed and sorted.  Device
// memory while it runs: the map's export bound x 12 bytes (kept), the same again for the sort's other buffers and n / 2
// bytes of histograms.
static int ensure_raw_sorted(bc_engine* e, uint64_t t_space, uint32_t S) {
  SortedRows& R = e->raw_rows;
  if (R.epoch == e->counts_epoch) return BC_OK;
  raw_sorted_drop(e);
  if (!e->d_slots) {  // nothing was ever submitted or imported
    R.epoch = e->counts_epoch;
    return BC_OK;
  }
  ScratchGuard g;
  StreamTimer timer;
  HIP_TRY(timer.start(g, e->stream));
  uint64_t* d_key = nullptr;
  uint32_t* d_cnt = nullptr;
  uint64_t n = 0;
  const int rc = export_pairs(e, "raw render", g, &d_key, &d_cnt, &n);
  if (rc != BC_OK) return rc;
  if (n) {
    uint64_t* d_key2 = nullptr;
    uint32_t *d_cnt2 = nullptr, *d_scratch = nullptr;
    HIP_TRY(g.dmalloc(&d_key2, n * 8));
    HIP_TRY(g.dmalloc(&d_cnt2, n * 4));
    HIP_TRY(g.dmalloc(&d_scratch, bc::sort_scratch_words(n) * 4));
    HIP_TRY(raw_rekey_launch(d_key, n, t_space, S, e->stream));
    uint32_t key_bits = 1;  // the bit length of the largest key of the space (the re-keyed digits have the same radices)
    while (key_bits < 64 && ((e->h.table_entries - 1) >> key_bits) != 0) ++key_bits;
    const hipError_t src = bc::sort_pairs_launch(e->stream, d_key, d_cnt, d_key2, d_cnt2, n, key_bits, d_scratch);
    if (src == hipErrorInvalidValue) {
      set_error("raw render: " + std::to_string(n) + " rows pass what one sort takes (2^32); write them from bc_engine_row_text on the host");
      return BC_ERR_UNSUPPORTED;
    }
    HIP_TRY(src);
  }
  HIP_TRY(timer.stop(&R.sort_ms));
  R.d_keys = g.release(d_key);
  R.d_cnts = g.release(d_cnt);
  R.n = n;
  R.epoch = e->counts_epoch;
  ++R.sorts;
  return BC_OK;
}

static int render_raw(bc_engine* e, const char* who, bool merged, const uint32_t* cols, uint32_t n_cols, bc_text_fn fn,
                      void* user, uint64_t* n_rows) {
  if (n_rows) *n_rows = 0;
  int rc = check_plan_shape(e, who, kRawCounts);
  if (rc) return rc;
  const DevPlan& P = e->h.plan;
  const uint32_t g0 = e->has_sample_group ? 1u : 0u;
  const uint32_t S = g0 ? P.groups[0].n_refs : 1u;
  const uint64_t t_space = g0 ? P.groups[0].table_stride : e->h.table_entries;
  if ((rc = check_request(who, cols, n_cols, fn, S)) != BC_OK) return rc;
  CountedGroups cg;
  if ((rc = raw_plan_groups(e, who, cg)) != BC_OK) return rc;
  HIP_TRY(hipSetDevice(e->device));
  if ((rc = bc_engine_sync(e)) != BC_OK) return rc;  // the submits, as bc_engine_finish waits for them
  if ((rc = ensure_raw_sorted(e, t_space, S)) != BC_OK) return rc;
  if (n_cols == 0 || e->raw_rows.n == 0) return BC_OK;
  if ((rc = ensure_render_pool(e, who)) != BC_OK) return rc;
  if ((rc = describe_groups(e, who, cg)) != BC_OK) return rc;
  bc::RawRenderView v;
  memset(&v, 0, sizeof v);
  v.G = cg.G;
  v.S = S;
  v.merged = merged ? 1u : 0u;
  v.sample = cols[0];
  memcpy(v.raw_len, cg.raw_len, sizeof v.raw_len);
  memcpy(v.off_start, cg.off_start, sizeof v.off_start);
  memcpy(v.radix, cg.radix, sizeof v.radix);
  v.keys = e->raw_rows.d_keys;
  v.cnts = e->raw_rows.d_cnts;
  v.n = e->raw_rows.n;
  return render_lines(e, who, v, counts_max_line(cg.G, cg.longest, n_cols), cols, n_cols, fn, user, n_rows);
}

extern "C" {

int bc_engine_render_raw_counts(bc_engine* e, uint32_t sample_idx, bc_text_fn fn, void* user, uint64_t* n_rows) {
  return render_raw(e, "bc_engine_render_raw_counts", false, &sample_idx, 1, fn, user, n_rows);
}

int bc_engine_render_raw_merged(bc_engine* e, const uint32_t* sample_idx, uint32_t n_samples, bc_text_fn fn, void* user,
                                uint64_t* n_rows) {
  return render_raw(e, "bc_engine_render_raw_merged", true, sample_idx, n_samples, fn, user, n_rows);
}

int bc_engine_raw_render_sorts(const bc_engine* e, uint64_t* n) {
  *n = e->raw_rows.sorts;
  return BC_OK;
}

int bc_engine_raw_render_sort_ms(const bc_engine* e, double* ms) {
  *ms = (double)e->raw_rows.sort_ms;
  return BC_OK;
}

}  // extern "C"

// ---- counts of a wide-key plan as text (bc_wide_render.h, bc_sort.h) ----

namespace bc {

// okeys[w * n + i] = word w of the order key of key i (blockIdx.y = w): a lane makes one word of one key
__global__ __launch_bounds__(256) void wide_order_kernel(WideOrder o, const unsigned long long* __restrict__ keys, uint64_t n,
                                                         unsigned long long* __restrict__ okeys) {
  const uint32_t w = blockIdx.y;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
    okeys[(uint64_t)w * n + i] = wide_order_word(o, (const uint64_t*)keys + i * o.W + 1u, w);
}

// the keys (W words each) and counts into file order: entry j comes from perm[j]; a lane moves one word
__global__ __launch_bounds__(256) void wide_gather_kernel(const unsigned long long* __restrict__ keys,
                                                          const uint32_t* __restrict__ cnts, const uint32_t* __restrict__ perm,
                                                          uint64_t n, uint32_t W, unsigned long long* __restrict__ keys_out,
                                                          uint32_t* __restrict__ cnts_out) {
  const uint64_t total = n * W, step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
    const uint64_t j = (t >> 32) == 0 ? (uint64_t)((uint32_t)t / W) : t / W;
    const uint32_t w = (uint32_t)(t - j * W);
    const uint64_t i = perm[j];
    if (i >= n) continue;  // (never: perm is a permutation of 0 .. n-1)
    keys_out[t] = keys[i * W + w];
    if (w == 0) cnts_out[j] = cnts[i];
  }
}

}  // namespace bc

// The keys and counts of the current counts in the order of the files, in e->wide_rows (n x (W x 8 + 4) bytes): served
// as they are while the counts epoch stands, else exported from the map (export_wide, as bc_engine_finish does), given order keys, sorted by them (bc::sort_words_launch) and gathered.  Peak device memory per
// exported row, beside the map: while the sort runs the exported row (W x 8 + 4), its order key (K x 8) and the sort's
// 24.5 bytes -- (W + K) x 8 + 28.5; order keys and sort buffers are released before the gather, which holds the row
// twice and the permutation -- 2 x (W x 8 + 4) + 4.  With K <= W - 1 <= 7 that is at most 148.5 bytes per row.  (A random-
// barcode plan's export holds its table of tuples, slots x (W x 8 + 8) bytes, until the rows are out, before any of it.)
static int ensure_wide_sorted(bc_engine* e, const bc::WideOrder& o) {
  SortedRows& R = e->wide_rows;
  if (R.epoch == e->counts_epoch) return BC_OK;
  R.drop();
  if (!e->d_slots) {  // nothing was ever submitted or imported
    R.epoch = e->counts_epoch;
    return BC_OK;
  }
  ScratchGuard g;
  StreamTimer timer;
  HIP_TRY(timer.start(g, e->stream));
  unsigned long long* d_key = nullptr;
  uint32_t* d_cnt = nullptr;
  uint64_t n = 0;
  const int rc = export_wide(e, "wide render", g, &d_key, &d_cnt, &n);
  if (rc != BC_OK) return rc;
  if (n >= 0xFFFFFFFFull - bc::kSortTile) {
    set_error("wide render: " + std::to_string(n) + " rows pass what one sort takes (2^32); write them from bc_engine_row_text on the host");
    return BC_ERR_UNSUPPORTED;
  }
  const uint32_t W = o.W;
  unsigned long long* d_key2 = nullptr;
  uint32_t* d_cnt2 = nullptr;
  if (n) {
    uint32_t* d_perm = nullptr;
    HIP_TRY(g.dmalloc(&d_perm, n * 4));
    {
      ScratchGuard s;  // order keys and the sort's buffers: gone before the gather's destination is made
      unsigned long long* d_okeys = nullptr;
      uint64_t *d_col = nullptr, *d_col2 = nullptr;
      uint32_t *d_perm2 = nullptr, *d_scratch = nullptr;
      HIP_TRY(s.dmalloc(&d_okeys, n * o.K * 8));
      HIP_TRY(s.dmalloc(&d_col, n * 8));
      HIP_TRY(s.dmalloc(&d_col2, n * 8));
      HIP_TRY(s.dmalloc(&d_perm2, n * 4));
      HIP_TRY(s.dmalloc(&d_scratch, bc::sort_scratch_words(n) * 4));
      hipLaunchKernelGGL(wide_order_kernel, dim3(std::min<uint32_t>(grid_for(n), 2048u), o.K), dim3(256), 0, e->stream, o, d_key, n,
                         d_okeys);
      HIP_TRY(hipGetLastError());
      HIP_TRY(bc::sort_words_launch(e->stream, (const uint64_t*)d_okeys, o.K, n, d_perm, d_col, d_col2, d_perm2, d_scratch));
      HIP_TRY(hipStreamSynchronize(e->stream));
    }
    HIP_TRY(g.dmalloc(&d_key2, n * W * 8));
    HIP_TRY(g.dmalloc(&d_cnt2, n * 4));
    hipLaunchKernelGGL(wide_gather_kernel, dim3(grid_for(n * W)), dim3(256), 0, e->stream, d_key, d_cnt, d_perm, n, W, d_key2, d_cnt2);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(timer.stop(&R.sort_ms));
  R.d_keys = (uint64_t*)g.release(d_key2);
  R.d_cnts = g.release(d_cnt2);
  R.n = n;
  R.epoch = e->counts_epoch;
  ++R.sorts;
  return BC_OK;
}

static int render_wide(bc_engine* e, const char* who, bool merged, const uint32_t* cols, uint32_t n_cols, bc_text_fn fn,
                       void* user, uint64_t* n_rows) {
  if (n_rows) *n_rows = 0;
  int rc = check_plan_shape(e, who, kWideCounts);
  if (rc) return rc;
  const LongPlan& Q = e->lh.plan;  // (a wide-key plan is the wave-per-read kernel's: its groups hold the key layout)
  const uint32_t g0 = e->has_sample_group ? 1u : 0u;
  const uint32_t S = g0 ? Q.groups[0].n_refs : 1u;
  if ((rc = check_request(who, cols, n_cols, fn, S)) != BC_OK) return rc;
  bc::WideRenderView v;
  bc::WideOrder o;
  CountedGroups cg;
  memset(&v, 0, sizeof v);
  memset(&o, 0, sizeof o);
  memset(&cg, 0, sizeof cg);
  v.G = o.G = cg.G = e->barcode_num;
  v.W = o.W = e->key_words;
  v.S = S;
  v.merged = merged ? 1u : 0u;
  v.sample = n_cols ? cols[0] : 0u;
  // (cannot happen: a plan's groups fit the view, its sample group comes first and starts the payload)
  if (v.G > (uint32_t)bc::kRenderMaxG || g0 + v.G > Q.n_groups || v.W > (uint32_t)kMaxKeyWords ||
      (g0 && (Q.groups[0].type != kGroupSample || Q.groups[0].key_bit != 0))) {
    set_error(std::string(who) + ": the plan's groups do not fit the view");
    return BC_ERR_STATE;
  }
  v.sample_bits = o.sample_bits = g0 ? 32u : 0u;
  o.sample_obits = g0 ? bc::wide_bit_length(S - 1u) : 0u;
  const uint32_t pay_bits = 64u * (v.W - 1u);
  for (uint32_t g = 0; g < v.G; ++g) {
    const LongGroup& G = Q.groups[g0 + g];
    v.key_bit[g] = o.key_bit[g] = G.key_bit;
    if (G.n_refs == 0) {
      v.raw_len[g] = o.raw_len[g] = cg.raw_len[g] = G.len;
    } else {
      v.n_ids[g] = cg.n_ids[g] = G.n_refs;
      o.obits[g] = bc::wide_bit_length(G.n_refs - 1u);
    }
    if (G.key_bit + (G.n_refs ? 32u : 3u * G.len) > pay_bits || (G.n_refs == 0 && G.len == 0)) {  // (cannot happen)
      set_error(std::string(who) + ": a group's field lies outside the key");
      return BC_ERR_STATE;
    }
  }
  bc::wide_order_layout(o);
  if (o.K + 1u > v.W) {  // (cannot happen: no field is wider in the order key than in the payload)
    set_error(std::string(who) + ": the order key is wider than the key");
    return BC_ERR_STATE;
  }
  HIP_TRY(hipSetDevice(e->device));
  if ((rc = bc_engine_sync(e)) != BC_OK) return rc;  // the submits, as bc_engine_finish waits for them
  if ((rc = ensure_wide_sorted(e, o)) != BC_OK) return rc;
  if (n_cols == 0 || e->wide_rows.n == 0) return BC_OK;
  if ((rc = ensure_render_pool(e, who)) != BC_OK) return rc;
  if ((rc = describe_groups(e, who, cg)) != BC_OK) return rc;  // (a wide key has bit fields, not digits: no radix)
  memcpy(v.off_start, cg.off_start, sizeof v.off_start);
  v.keys = e->wide_rows.d_keys;
  v.cnts = e->wide_rows.d_cnts;
  v.n = e->wide_rows.n;
  return render_lines(e, who, v, counts_max_line(cg.G, cg.longest, n_cols), cols, n_cols, fn, user, n_rows);
}

extern "C" {

int bc_engine_render_wide_counts(bc_engine* e, uint32_t sample_idx, bc_text_fn fn, void* user, uint64_t* n_rows) {
  return render_wide(e, "bc_engine_render_wide_counts", false, &sample_idx, 1, fn, user, n_rows);
}

int bc_engine_render_wide_merged(bc_engine* e, const uint32_t* sample_idx, uint32_t n_samples, bc_text_fn fn, void* user,
                                 uint64_t* n_rows) {
  return render_wide(e, "bc_engine_render_wide_merged", true, sample_idx, n_samples, fn, user, n_rows);
}

int bc_engine_wide_render_sorts(const bc_engine* e, uint64_t* n) {
  *n = e->wide_rows.sorts;
  return BC_OK;
}

int bc_engine_wide_render_sort_ms(const bc_engine* e, double* ms) {
  *ms = (double)e->wide_rows.sort_ms;
  return BC_OK;
}

}  // extern "C"

// ---- Single / Double enrichment as text (bc_enrich_render.h) ----

namespace {

// One key per lane, grid-stride over S * K entries.  A key that is not canonical moves its sum to the canonical one: an
// entry is either only added to (canonical) or only read and zeroed by its own lane (the others), so no order matters.
__global__ __launch_bounds__(256) void enrich_fold_kernel(bc::EnrichRenderView v, uint64_t n_samples) {
  unsigned long long* sums = const_cast<unsigned long long*>(v.sums);
  const uint64_t total = n_samples * v.K, step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const unsigned long long x = sums[e];
    if (!x) continue;
    const uint64_t s = e / v.K, k = e - s * v.K;
    const uint64_t t = bc::enrich_fold_target(v, k);
    if (t == k) continue;
    atomicAdd(sums + s * v.K + t, x);
    sums[e] = 0ull;
  }
}

}  // namespace

// Folds the sums of one kind for n_samples samples (v.sums writable, v.canon not NULL): every key that is not its own
// enrich_fold_target adds its sum to the target and becomes zero.
static hipError_t enrich_fold_launch(const bc::EnrichRenderView& v, uint64_t n_samples, hipStream_t stream) {
  const uint64_t total = n_samples * v.K;
  if (total == 0 || !v.canon) return hipSuccess;
  hipLaunchKernelGGL(enrich_fold_kernel, dim3(grid_for(total)), dim3(256), 0, stream, v, n_samples);
  return hipGetLastError();
}

// For every counted set, which entries share an ID: canon[off_g + i] = the smallest index of set g whose ID equals i's.
// Built once per engine, next to the label pool; uploaded only when some set does share an ID.
static int ensure_canon(bc_engine* e, const char* who) {
  if (e->labels.canon_ready) return BC_OK;
  std::vector<uint32_t> canon;
  bool shared = false;
  try {
    for (uint32_t g = 0; g < e->barcode_num; ++g) {
      std::unordered_map<std::string, uint32_t> first;
      const uint32_t n = bc_plan_n_counted(e->src_plan, g);
      for (uint32_t i = 0; i < n; ++i) {
        const char* id = bc_plan_counted_id(e->src_plan, g, i);
        const uint32_t c = first.emplace(id ? id : "", i).first->second;
        shared = shared || c != i;
        canon.push_back(c);
      }
    }
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return BC_ERR_NOMEM;
  }
  if (shared) {
    uint64_t d = 0;
    const int rc = upload(e, canon.data(), canon.size() * 4, &d);
    if (rc != BC_OK) return rc;
    e->labels.d_canon = (uint32_t*)(uintptr_t)d;
  }
  e->labels.canon_ready = true;
  return BC_OK;
}

// the view of one kind over the engine's sums (columns and label pool: render_lines)
static bc::EnrichRenderView enrich_view(const bc_engine* e, const EnrichShape& sh, uint64_t S, uint32_t kind) {
  bc::EnrichRenderView v;
  memset(&v, 0, sizeof v);
  v.kind = kind;
  v.G = sh.G;
  v.K = kind == bc::kEnrichSingle ? sh.sum_n : sh.pairs;
  v.sums = e->sums.d + (kind == bc::kEnrichSingle ? 0 : S * sh.sum_n);
  v.canon = e->labels.d_canon;
  for (uint32_t g = 0; g < sh.G; ++g) {
    v.n[g] = sh.n[g];
    v.off_start[g] = e->labels.off_start[g];
  }
  return v;
}

// The folded sums of the counts as they stand, on the device: computed by one pass over the table (bc_enrich_launch) and
// the fold, then kept until the counts may have changed (counts_epoch).
static int ensure_sums(bc_engine* e, const EnrichShape& sh, uint64_t S) {
  const bool keep = e->own_table && !e->table_exposed;  // (nobody else can write the table between two renders)
  if (e->sums.d && keep && e->sums.epoch == e->counts_epoch) return BC_OK;
  HIP_TRY(hipSetDevice(e->device));
  const uint64_t n_single = S * sh.sum_n, n_double = S * sh.pairs;
  e->sums.epoch = 0;
  if (!e->sums.d) HIP_TRY(hipMalloc((void**)&e->sums.d, (size_t)(n_single + n_double) * 8));
  HIP_TRY(hipMemsetAsync(e->sums.d, 0, (size_t)(n_single + n_double) * 8, e->stream));
  HIP_TRY(bc_enrich_launch(sh, e->d_table, e->bits_dirty ? e->d_bits : nullptr, e->table_entries, e->sums.d,
                           n_double ? e->sums.d + n_single : nullptr, e->stream));
  if (e->labels.d_canon) {
    HIP_TRY(enrich_fold_launch(enrich_view(e, sh, S, bc::kEnrichSingle), S, e->stream));
    if (n_double) HIP_TRY(enrich_fold_launch(enrich_view(e, sh, S, bc::kEnrichDouble), S, e->stream));
  }
  ++e->sums.passes;
  if (keep) e->sums.epoch = e->counts_epoch;
  return BC_OK;
}

static int render_enriched(bc_engine* e, const char* who, int kind, const uint32_t* cols, uint32_t n_cols, bc_text_fn fn,
                           void* user, uint64_t* n_rows) {
  if (n_rows) *n_rows = 0;
  EnrichShape sh;
  uint64_t S = 0;
  if (!enrich_shape(e, who, &sh, &S)) return BC_ERR_UNSUPPORTED;
  int rc = check_kind(who, kind);
  if (rc) return rc;
  if ((rc = check_request(who, cols, n_cols, fn, S)) != BC_OK) return rc;
  if ((rc = dense_counts_ready(e)) != BC_OK) return rc;
  const uint64_t K = kind == BC_ENRICH_SINGLE ? sh.sum_n : sh.pairs;  // (no pairs below three counted barcodes)
  if (n_cols == 0 || K == 0 || e->table_entries == 0) return BC_OK;
  if ((rc = ensure_render_pool(e, who)) != BC_OK) return rc;
  if ((rc = ensure_canon(e, who)) != BC_OK) return rc;
  for (uint32_t g = 0; g < sh.G; ++g)
    if ((rc = check_set_size(e, who, g, sh.n[g])) != BC_OK) return rc;
  const uint64_t max_line = enrich_max_line(sh.G, e->labels.max_len, n_cols, kind);
  if ((rc = check_max_line(who, max_line)) != BC_OK) return rc;  // (before the table is passed over for a refused request)
  if ((rc = ensure_sums(e, sh, S)) != BC_OK) return rc;
  bc::EnrichRenderView v = enrich_view(e, sh, S, (uint32_t)kind);
  return render_lines(e, who, v, max_line, cols, n_cols, fn, user, n_rows);
}

extern "C" {

int bc_engine_render_enriched(bc_engine* e, int kind, uint32_t sample_idx, bc_text_fn fn, void* user, uint64_t* n_rows) {
  return render_enriched(e, "bc_engine_render_enriched", kind, &sample_idx, 1, fn, user, n_rows);
}

int bc_engine_render_enriched_merged(bc_engine* e, int kind, const uint32_t* sample_idx, uint32_t n_samples, bc_text_fn fn,
                                     void* user, uint64_t* n_rows) {
  return render_enriched(e, "bc_engine_render_enriched_merged", kind, sample_idx, n_samples, fn, user, n_rows);
}

int bc_engine_enrich_render_passes(const bc_engine* e, uint64_t* n) {
  *n = e->sums.passes;
  return BC_OK;
}

}  // extern "C"

// ---- Single / Double enrichment of a raw-key plan as text (bc_raw_enrich_render.h, bc_sort.h, bc_reduce.h) ----

namespace bc {

// out_keys[i] = the projection of keys[i], out_vals[i] = cnts[i]: one lane per entry
__global__ __launch_bounds__(256) void raw_enrich_project_kernel(RawEnrichProj p, const unsigned long long* __restrict__ keys,
                                                                 const uint32_t* __restrict__ cnts, uint64_t n,
                                                                 unsigned long long* __restrict__ out_keys,
                                                                 uint32_t* __restrict__ out_vals) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    out_keys[i] = raw_enrich_project(p, keys[i]);
    out_vals[i] = cnts[i];
  }
}

}  // namespace bc

// The (projected key, sum) segments of one kind (k = 0: Single, 1: Double) for the sorted pairs as they stand
// (ensure_raw_sorted has run, e->raw_rows.n != 0), in e->raw_enrich[k]: served as they are while the counts epoch stands, else
// made projection by projection -- project, sort over the bits of the projection's bound, reduce the runs, keep the
// runs in an allocation of their own size -- and joined at the end.  Every projection is sorted, the Single of group 0
// too: its input ascends in d_0 already, but entries of one (d_0, s) are not adjacent there (s is the least significant
// digit of every key in between), and a reduction needs them adjacent.
// Device memory while a kind is built, n = raw_rows.n: 12 n (projected pairs) + 12 n (the sort's other buffers, whose keys
// then take the runs' keys) + n / 2 (histograms) + 8 n (sums) = 32.5 n bytes beside the kept 12 n -- one set of buffers,
// allocated once and used by every projection in turn (the stream orders the reuse), released before the segments are
// joined; kept: 16 bytes per (key, sample) with a sum, twice that while the segments are joined.
static int ensure_raw_enrich(bc_engine* e, int k, const bc::RawEnrichProj& base) {
  RawEnrichSegs& R = e->raw_enrich[k];
  if (R.epoch == e->counts_epoch) return BC_OK;
  R.drop();
  const uint64_t n = e->raw_rows.n;
  const uint32_t G = base.G, n_seg = k == 0 ? G : G * (G - 1u) / 2u;
  ScratchGuard segs;  // every projection's runs (keys, then sums) until they are joined
  std::vector<uint64_t> start;
  StreamTimer timer;
  HIP_TRY(timer.start(segs, e->stream));
  try {
    start.reserve(n_seg + 1u);
    segs.dev.reserve(2u * n_seg + 2u);
  } catch (const std::bad_alloc&) {
    set_error("raw enrichment: out of host memory");
    return BC_ERR_NOMEM;
  }
  uint64_t total = 0;
  {
    ScratchGuard s;  // the buffers every projection works in: gone before the segments are joined
    uint64_t *d_pk = nullptr, *d_tk = nullptr, *d_sum = nullptr;
    uint32_t *d_pv = nullptr, *d_tv = nullptr, *d_sort = nullptr, *d_red = nullptr, *d_runs = nullptr;
    HIP_TRY(s.dmalloc(&d_pk, n * 8));
    HIP_TRY(s.dmalloc(&d_pv, n * 4));
    HIP_TRY(s.dmalloc(&d_tk, n * 8));
    HIP_TRY(s.dmalloc(&d_tv, n * 4));
    HIP_TRY(s.dmalloc(&d_sort, bc::sort_scratch_words(n) * 4));
    HIP_TRY(s.dmalloc(&d_sum, n * 8));
    HIP_TRY(s.dmalloc(&d_red, bc::reduce_scratch_words(n) * 4));
    HIP_TRY(s.dmalloc(&d_runs, 4));
    for (uint32_t g = 0; g < G; ++g)
      for (uint32_t h = k == 0 ? g : g + 1u; h < (k == 0 ? g + 1u : G); ++h) {
        bc::RawEnrichProj p = base;
        p.g = g;
        p.h = h;
        const uint64_t bound = bc::raw_enrich_bound(p);
        uint32_t key_bits = 1;
        while (key_bits < 64 && ((bound - 1u) >> key_bits) != 0) ++key_bits;
        hipLaunchKernelGGL(raw_enrich_project_kernel, dim3(grid_for(n)), dim3(256), 0, e->stream, p,
                           (const unsigned long long*)e->raw_rows.d_keys, (const uint32_t*)e->raw_rows.d_cnts, n, (unsigned long long*)d_pk, d_pv);
        HIP_TRY(hipGetLastError());
        HIP_TRY(bc::sort_pairs_launch(e->stream, d_pk, d_pv, d_tk, d_tv, n, key_bits, d_sort));
        HIP_TRY(bc::reduce_runs_launch(e->stream, d_pk, d_pv, n, d_tk, d_sum, d_runs, d_red));
        uint32_t runs = 0;
        HIP_TRY(hipMemcpyAsync(&runs, d_runs, 4, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));  // (the one wait of a projection beside the sort's own)
        if (runs > n) {  // (cannot happen: there are no more runs than pairs)
          set_error("raw enrichment: the reduction reports more runs than pairs");
          return BC_ERR_STATE;
        }
        uint64_t *d_rk = nullptr, *d_rs = nullptr;
        HIP_TRY(segs.dmalloc(&d_rk, (size_t)runs * 8));
        HIP_TRY(segs.dmalloc(&d_rs, (size_t)runs * 8));
        if (runs) {  // (the next projection's kernels come after these copies on the stream)
          HIP_TRY(hipMemcpyAsync(d_rk, d_tk, (size_t)runs * 8, hipMemcpyDeviceToDevice, e->stream));
          HIP_TRY(hipMemcpyAsync(d_rs, d_sum, (size_t)runs * 8, hipMemcpyDeviceToDevice, e->stream));
        }
        start.push_back(total);
        total += runs;
      }
    HIP_TRY(hipStreamSynchronize(e->stream));  // nothing may still read the buffers when they go
  }
  start.push_back(total);
  // keys, sums, segment starts: one allocation
  void* d_all = nullptr;
  HIP_TRY(hipMalloc(&d_all, (size_t)(2u * total + n_seg + 1u) * 8));
  uint64_t* d_keys = (uint64_t*)d_all;
  uint64_t* d_sums = d_keys + total;
  auto join = [&]() -> int {
    for (uint32_t q = 0; q < n_seg; ++q) {
      const uint64_t len = start[q + 1u] - start[q];
      if (!len) continue;
      HIP_TRY(hipMemcpyAsync(d_keys + start[q], segs.dev[2u * q], (size_t)len * 8, hipMemcpyDeviceToDevice, e->stream));
      HIP_TRY(hipMemcpyAsync(d_sums + start[q], segs.dev[2u * q + 1u], (size_t)len * 8, hipMemcpyDeviceToDevice, e->stream));
    }
    HIP_TRY(hipMemcpyAsync(d_sums + total, start.data(), (size_t)(n_seg + 1u) * 8, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(timer.stop(&e->raw_enrich_ms));
    return BC_OK;
  };
  const int rc = join();
  if (rc != BC_OK) {
    (void)hipFree(d_all);
    return rc;
  }
  R.d = d_all;
  R.n = total;
  R.n_seg = n_seg;
  R.epoch = e->counts_epoch;
  ++e->raw_enrich_builds;
  return BC_OK;
}

static int render_raw_enriched(bc_engine* e, const char* who, bool merged, int kind, const uint32_t* cols, uint32_t n_cols,
                               bc_text_fn fn, void* user, uint64_t* n_rows) {
  if (n_rows) *n_rows = 0;
  int rc = check_plan_shape(e, who, kRawEnrich);
  if (rc) return rc;
  if ((rc = check_kind(who, kind)) != BC_OK) return rc;
  const DevPlan& P = e->h.plan;
  const uint32_t g0 = e->has_sample_group ? 1u : 0u;
  const uint32_t S = g0 ? P.groups[0].n_refs : 1u;
  const uint64_t t_space = g0 ? P.groups[0].table_stride : e->h.table_entries;
  if ((rc = check_request(who, cols, n_cols, fn, S)) != BC_OK) return rc;
  CountedGroups cg;
  if ((rc = raw_plan_groups(e, who, cg)) != BC_OK) return rc;
  const uint32_t G = cg.G;
  if (kind == BC_ENRICH_DOUBLE && G < 3) return BC_OK;  // (no pairs below three counted barcodes, as the dense call)
  HIP_TRY(hipSetDevice(e->device));
  if ((rc = bc_engine_sync(e)) != BC_OK) return rc;  // the submits, as bc_engine_finish waits for them
  if ((rc = ensure_raw_sorted(e, t_space, S)) != BC_OK) return rc;
  if (n_cols == 0 || e->raw_rows.n == 0 || G == 0) return BC_OK;
  if ((rc = ensure_render_pool(e, who)) != BC_OK) return rc;
  if ((rc = ensure_canon(e, who)) != BC_OK) return rc;
  if ((rc = describe_groups(e, who, cg)) != BC_OK) return rc;
  bc::RawEnrichProj proj;
  bc::RawEnrichView v;
  memset(&proj, 0, sizeof proj);
  memset(&v, 0, sizeof v);
  proj.canon = e->labels.d_canon;
  proj.S = v.S = S;
  proj.G = v.G = G;
  v.kind = (uint32_t)kind;
  v.merged = merged ? 1u : 0u;
  v.sample = cols[0];
  memcpy(v.raw_len, cg.raw_len, sizeof v.raw_len);
  memcpy(v.off_start, cg.off_start, sizeof v.off_start);
  memcpy(v.radix, cg.radix, sizeof v.radix);
  memcpy(proj.radix, cg.radix, sizeof proj.radix);
  uint32_t canon_off = 0;
  for (uint32_t g = 0; g < G; ++g) {
    proj.known[g] = cg.raw_len[g] ? 0u : 1u;
    proj.canon_off[g] = canon_off;
    canon_off += bc_plan_n_counted(e->src_plan, g);  // (ensure_canon lays the sets out back to back)
  }
  const uint64_t max_line = enrich_max_line(G, cg.longest, n_cols, kind);
  if ((rc = check_max_line(who, max_line)) != BC_OK) return rc;  // (before anything is built for a refused request)
  const RawEnrichSegs& R = e->raw_enrich[kind == BC_ENRICH_SINGLE ? 0 : 1];
  if ((rc = ensure_raw_enrich(e, kind == BC_ENRICH_SINGLE ? 0 : 1, proj)) != BC_OK) return rc;
  if (R.n == 0) return BC_OK;
  v.n = R.n;
  v.n_seg = R.n_seg;
  v.keys = (const uint64_t*)R.d;
  v.sums = v.keys + v.n;
  v.seg_start = v.sums + v.n;
  return render_lines(e, who, v, max_line, cols, n_cols, fn, user, n_rows);
}

extern "C" {

int bc_engine_render_raw_enriched(bc_engine* e, int kind, uint32_t sample_idx, bc_text_fn fn, void* user, uint64_t* n_rows) {
  return render_raw_enriched(e, "bc_engine_render_raw_enriched", false, kind, &sample_idx, 1, fn, user, n_rows);
}

int bc_engine_render_raw_enriched_merged(bc_engine* e, int kind, const uint32_t* sample_idx, uint32_t n_samples, bc_text_fn fn,
                                         void* user, uint64_t* n_rows) {
  return render_raw_enriched(e, "bc_engine_render_raw_enriched_merged", true, kind, sample_idx, n_samples, fn, user, n_rows);
}

int bc_engine_raw_enrich_reduces(const bc_engine* e, uint64_t* n) {
  *n = e->raw_enrich_builds;
  return BC_OK;
}

int bc_engine_raw_enrich_reduce_ms(const bc_engine* e, double* ms) {
  *ms = (double)e->raw_enrich_ms;
  return BC_OK;
}

}  // extern "C"
