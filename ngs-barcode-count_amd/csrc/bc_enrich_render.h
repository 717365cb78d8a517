// bc_enrich_render.h -- the text of a dense plan's Single and Double enrichment files (bc_engine_render_enriched /
// bc_engine_render_enriched_merged): the lane-level pieces, shared by the kernels of bc_text_kernels.h (instantiated in
// bc_text.hip, next to the fold of the sums) and the host harness tests/render/enrich_render_host.cpp (which runs this
// SAME code under AddressSanitizer; never a product path on the host).
//
// A line belongs to one key k of one sample's slice of the marginal sums (bc_engine_enrich's layout; G counted barcodes,
// N_g = size of known set g, SUM = sum N_g, P = sum over pairs g < h of N_g * N_h, pairs in add_double's order):
//     Single  k in [0, SUM)  ->  (g, i)        k = off_g + i
//     Double  k in [0, P)    ->  (g, h, i, j)  k = poff_(g,h) + i * N_h + j
// and to an ordered list of sample columns.  It has G fields joined by commas -- field g holds id_g (and field h id_h),
// every other field is empty, as add_single / add_double build the key (info.rs:840-904) -- then one count per column:
//     ,id,,c_0,c_1,..\n        c_m = sums[cols[m] * K + k], a u64 in decimal
// and exists when some c_m is not zero.  IDs are copied verbatim from the label pool (bc_line.h).
//
// Entries of one known set whose IDs are byte-equal are ONE key of the reference's maps (they are keyed by text): the
// sums are folded before any line is written -- enrich_fold_target names, for every key, the key of the smallest indices
// carrying the same IDs; a key that is not its own target adds its sum there and becomes zero, so it has no line.
// Text that coincides ACROSS groups or pairs (possible only when some ID is empty: ",," is the empty ID of every group)
// is NOT merged: such plans are not for this renderer.
//
// A line is measured and written from its END backwards, digit by digit (bc_line.h).
#ifndef BC_ENRICH_RENDER_H
#define BC_ENRICH_RENDER_H

#include "bc_line.h"

namespace bc {

constexpr uint32_t kEnrichSingle = 1, kEnrichDouble = 2;  // BC_ENRICH_SINGLE / BC_ENRICH_DOUBLE

struct EnrichRenderView {
  const unsigned long long* sums;  // this kind's sums, folded: entry s * K + k
  const uint32_t* cols;            // sample index of every column
  const uint32_t* canon;           // canon[off_g + i]: the smallest index of set g with i's ID; NULL: no set shares an ID
  const uint32_t* label_off;       // the label pool (bc_line.h)
  const uint8_t* label_bytes;
  uint64_t K;                      // keys per sample: SUM or P
  uint32_t n_cols;
  uint32_t G;
  uint32_t kind;                   // kEnrichSingle | kEnrichDouble
  uint32_t n[kRenderMaxG];          // N_g
  uint32_t off_start[kRenderMaxG];  // where group g's N_g + 1 offsets start in label_off
};

struct EnrichKey {
  uint32_t g, h;  // the fields that hold an ID (h = g for a single)
  uint32_t i, j;  // indices into sets g and h
};

// key -> the fields and indices it stands for (k < v.K)
BC_HD EnrichKey enrich_key(const EnrichRenderView& v, uint64_t k) {
  EnrichKey key = {0u, 0u, 0u, 0u};
  if (v.kind == kEnrichSingle) {
    uint32_t g = 0;
    while (g + 1 < v.G && k >= v.n[g]) k -= v.n[g++];
    key.g = key.h = g;
    key.i = key.j = (uint32_t)k;
    return key;
  }
  for (uint32_t g = 0; g + 1 < v.G; ++g)
    for (uint32_t h = g + 1; h < v.G; ++h) {
      const uint64_t sz = (uint64_t)v.n[g] * v.n[h];
      if (k < sz || (g + 2 == v.G)) {  // (the last pair takes what is left)
        key.g = g;
        key.h = h;
        key.j = (uint32_t)take_digit(k, v.n[h]);
        key.i = (uint32_t)k;
        return key;
      }
      k -= sz;
    }
  return key;
}

// off_g = N_0 + .. + N_{g-1}: where set g starts in v.canon (and in a single's key space)
BC_HD uint64_t enrich_set_off(const EnrichRenderView& v, uint32_t g) {
  uint64_t off = 0;
  for (uint32_t x = 0; x < g; ++x) off += v.n[x];
  return off;
}

// the key that k's sum belongs to: the same fields with the smallest indices that carry the same IDs (k itself when it
// is canonical, and always without v.canon)
BC_HD uint64_t enrich_fold_target(const EnrichRenderView& v, uint64_t k) {
  if (!v.canon) return k;
  const EnrichKey key = enrich_key(v, k);
  const uint32_t ci = v.canon[enrich_set_off(v, key.g) + key.i];
  if (v.kind == kEnrichSingle) return k - key.i + ci;
  const uint32_t cj = v.canon[enrich_set_off(v, key.h) + key.j];
  const uint64_t nh = v.n[key.h];
  return k - ((uint64_t)key.i * nh + key.j) + ((uint64_t)ci * nh + cj);
}

BC_HD uint64_t enrich_sum(const EnrichRenderView& v, uint32_t c, uint64_t k) { return v.sums[(uint64_t)v.cols[c] * v.K + k]; }

// bytes of key k's line, '\n' included; 0 when every column is zero (no line)
BC_HD uint32_t enrich_row_len(const EnrichRenderView& v, uint64_t k) {
  uint64_t any = 0;
  uint32_t len = 1u + (v.G ? v.G - 1u : 0u);  // '\n' and the commas between the fields
  for (uint32_t c = 0; c < v.n_cols; ++c) {
    const uint64_t x = enrich_sum(v, c, k);
    any |= x;
    len += 1u + digits_u64(x);  // ",count"
  }
  if (!any) return 0;
  const EnrichKey key = enrich_key(v, k);
  len += label_len(v.label_off, v.off_start[key.g], key.i);
  if (v.kind == kEnrichDouble) len += label_len(v.label_off, v.off_start[key.h], key.j);
  return len;
}

// Writes the part of key k's line (len = enrich_row_len, not 0) that falls into the window dst[0 .. win); the line starts
// at window position `at` (bc_line.h).
template <typename Byte>
BC_HD void enrich_row_write(const EnrichRenderView& v, uint64_t k, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  LineCursor<Byte> c(dst, at, len, win);
  c.put('\n');
  for (uint32_t m = v.n_cols; m-- > 0;) {
    c.put_u64(enrich_sum(v, m, k));
    c.put(',');
  }
  const EnrichKey key = enrich_key(v, k);
  for (uint32_t f = v.G; f-- > 0;) {
    // (for a single h == g: the first test takes it)
    if (f == key.h || f == key.g) {
      const uint32_t* o = v.label_off + v.off_start[f] + (f == key.h ? key.j : key.i);
      c.put_label(v.label_bytes, o[0], o[1] - o[0]);
    }
    if (f) c.put(',');
  }
}

// the names bc_text_kernels.h reaches a view's lane code by
BC_HD uint64_t text_keys(const EnrichRenderView& v) { return v.K; }
BC_HD uint32_t text_line_len(const EnrichRenderView& v, uint64_t k) { return enrich_row_len(v, k); }
template <typename Byte>
BC_HD void text_line_write(const EnrichRenderView& v, uint64_t k, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  enrich_row_write(v, k, len, dst, at, win);
}

}  // namespace bc

#endif
