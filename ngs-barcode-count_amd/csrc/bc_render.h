// bc_render.h -- the text of a dense plan's counts files (bc_engine_render_counts / bc_engine_render_merged): the
// lane-level pieces, shared by the kernels of bc_text_kernels.h (instantiated in bc_text.hip) and the host harness
// tests/render/render_host.cpp (which runs this SAME code under AddressSanitizer; never a product path on the host).
//
// A line belongs to one barcode tuple t in [0, T), T = N_0 * .. * N_{G-1} (the last counted barcode is the innermost
// axis, as bc_engine_decode_index reads it), and to an ordered list of sample columns:
//     id_0,id_1,..,id_{G-1},c_0,c_1,..\n       c_k = the count of (cols[k], t), written in decimal
// and exists when some c_k is not zero.  The per-sample file is the one-column case.  IDs are copied verbatim from the
// label pool: group g's offsets are label_off[off_start[g] .. off_start[g] + N_g], byte positions in label_bytes.
//
// Nothing here indexes a local array: a line is measured and written from its END backwards, in the order the index
// decodes (innermost digit first), so the digits of t never have to be kept.
#ifndef BC_RENDER_H
#define BC_RENDER_H

#include "bc_intrin.h"

namespace bc {

constexpr int kRenderMaxG = 18;                  // counted barcodes: as many as a plan may have groups (kMaxGroups)
constexpr uint32_t kRenderMaxLine = 1u << 25;    // longest line taken: 64 of them stay below 2^31 bytes

struct RenderView {
  const uint32_t* table;       // the dense table: entry s * T + t
  const uint32_t* bits;        // two-level counting, not folded: count = table[i] + bit i; NULL otherwise
  const uint32_t* cols;        // sample index of every column
  const uint32_t* label_off;   // the label pool's offsets (u32 byte positions), all groups back to back
  const uint8_t* label_bytes;  // the IDs, back to back
  uint64_t T;                  // tuples per sample
  uint32_t n_cols;
  uint32_t G;
  uint32_t n[kRenderMaxG];          // N_g
  uint32_t off_start[kRenderMaxG];  // where group g's N_g + 1 offsets start in label_off
};

// decimal digits of x: 1 .. 10
BC_HD uint32_t render_digits(uint32_t x) {
  return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) +
         (x >= 100000000u) + (x >= 1000000000u);
}

// the count of column c for tuple t, as compact_range_kernel reads an entry
BC_HD uint32_t render_count(const RenderView& v, uint32_t c, uint64_t t) {
  const uint64_t i = (uint64_t)v.cols[c] * v.T + t;
  return v.table[i] + (v.bits ? (v.bits[i >> 5] >> (i & 31)) & 1u : 0u);
}

// r = t with the digits of groups above g already taken off -> digit of group g; r loses it.  (One 64-bit division at
// most matters: after the innermost groups r fits 32 bits for every table that fits a GPU.)
BC_HD uint32_t render_take_digit(uint64_t& r, uint32_t n) {
  if ((r >> 32) == 0) {
    const uint32_t r32 = (uint32_t)r, q = r32 / n;
    r = q;
    return r32 - q * n;
  }
  const uint64_t q = r / n;
  const uint32_t d = (uint32_t)(r - q * n);
  r = q;
  return d;
}

// bytes of tuple t's line, '\n' included; 0 when every column is zero (no line)
BC_HD uint32_t render_row_len(const RenderView& v, uint64_t t) {
  uint32_t any = 0, len = 1u + (v.G ? v.G - 1u : 0u);  // '\n' and the commas between the IDs
  for (uint32_t c = 0; c < v.n_cols; ++c) {
    const uint32_t x = render_count(v, c, t);
    any |= x;
    len += 1u + render_digits(x);  // ",count"
  }
  if (!any) return 0;
  uint64_t r = t;
  for (uint32_t g = v.G; g-- > 0;) {
    const uint32_t d = render_take_digit(r, v.n[g]);
    const uint32_t* o = v.label_off + v.off_start[g] + d;
    len += o[1] - o[0];
  }
  return len;
}

// Writes the part of tuple t's line (len = render_row_len, not 0) that falls into the window dst[0 .. win): the line
// starts at window position `at`, which may be negative or beyond the window -- a wavefront stages the text of its 64
// entries window by window, and a long line crosses windows.
template <typename Byte>
BC_HD void render_row_write(const RenderView& v, uint64_t t, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  int64_t p = at + (int64_t)len;  // one past the byte written next (the line is written backwards)
#define BC_RENDER_PUT(ch)                                 \
  do {                                                    \
    --p;                                                  \
    if (p >= 0 && p < (int64_t)win) dst[p] = (Byte)(ch);  \
  } while (0)
  BC_RENDER_PUT('\n');
  for (uint32_t c = v.n_cols; c-- > 0;) {
    uint32_t x = render_count(v, c, t);
    do {
      const uint32_t q = x / 10u;
      BC_RENDER_PUT('0' + (x - q * 10u));
      x = q;
    } while (x);
    BC_RENDER_PUT(',');
  }
  uint64_t r = t;
  for (uint32_t g = v.G; g-- > 0;) {
    const uint32_t d = render_take_digit(r, v.n[g]);
    const uint32_t* o = v.label_off + v.off_start[g] + d;
    const uint32_t a = o[0], n = o[1] - o[0];
    // the label lies at [p - n, p): only its bytes inside the window are touched
    int64_t lo = p - (int64_t)n, hi = p;
    p = lo;
    if (lo < 0) lo = 0;
    if (hi > (int64_t)win) hi = (int64_t)win;
    for (int64_t w = lo; w < hi; ++w) dst[w] = (Byte)v.label_bytes[a + (uint32_t)(w - p)];
    if (g) BC_RENDER_PUT(',');
  }
#undef BC_RENDER_PUT
}

// the names bc_text_kernels.h reaches a view's lane code by
BC_HD uint64_t text_keys(const RenderView& v) { return v.T; }
BC_HD uint32_t text_line_len(const RenderView& v, uint64_t t) { return render_row_len(v, t); }
template <typename Byte>
BC_HD void text_line_write(const RenderView& v, uint64_t t, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  render_row_write(v, t, len, dst, at, win);
}

}  // namespace bc

#endif
