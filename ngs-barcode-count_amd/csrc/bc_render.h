// bc_render.h -- the text of a dense plan's counts files (bc_engine_render_counts / bc_engine_render_merged): the
// lane-level pieces, shared by the kernels of bc_text_kernels.h (instantiated in bc_text.hip) and the host harness
// tests/render/render_host.cpp (which runs this SAME code under AddressSanitizer; never a product path on the host).
//
// A line belongs to one barcode tuple t in [0, T), T = N_0 * .. * N_{G-1} (the last counted barcode is the innermost
// axis, as bc_engine_decode_index reads it), and to an ordered list of sample columns:
//     id_0,id_1,..,id_{G-1},c_0,c_1,..\n       c_k = the count of (cols[k], t), written in decimal
// and exists when some c_k is not zero.  The per-sample file is the one-column case.  IDs are copied verbatim from the
// label pool, and the line is measured and written from its END backwards (bc_line.h).
#ifndef BC_RENDER_H
#define BC_RENDER_H

#include "bc_line.h"

namespace bc {

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

// the count of column c for tuple t, as compact_range_kernel reads an entry
BC_HD uint32_t render_count(const RenderView& v, uint32_t c, uint64_t t) {
  const uint64_t i = (uint64_t)v.cols[c] * v.T + t;
  return v.table[i] + (v.bits ? (v.bits[i >> 5] >> (i & 31)) & 1u : 0u);
}

// bytes of tuple t's line, '\n' included; 0 when every column is zero (no line)
BC_HD uint32_t render_row_len(const RenderView& v, uint64_t t) {
  uint32_t any = 0, len = 1u + (v.G ? v.G - 1u : 0u);  // '\n' and the commas between the IDs
  for (uint32_t c = 0; c < v.n_cols; ++c) {
    const uint32_t x = render_count(v, c, t);
    any |= x;
    len += 1u + digits_u32(x);  // ",count"
  }
  if (!any) return 0;
  uint64_t r = t;
  for (uint32_t g = v.G; g-- > 0;) len += label_len(v.label_off, v.off_start[g], (uint32_t)take_digit(r, v.n[g]));
  return len;
}

// Writes the part of tuple t's line (len = render_row_len, not 0) that falls into the window dst[0 .. win); the line
// starts at window position `at` (bc_line.h).
template <typename Byte>
BC_HD void render_row_write(const RenderView& v, uint64_t t, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  LineCursor<Byte> c(dst, at, len, win);
  c.put('\n');
  for (uint32_t k = v.n_cols; k-- > 0;) {
    c.put_u32(render_count(v, k, t));
    c.put(',');
  }
  uint64_t r = t;
  for (uint32_t g = v.G; g-- > 0;) {
    const uint32_t* o = v.label_off + v.off_start[g] + (uint32_t)take_digit(r, v.n[g]);
    c.put_label(v.label_bytes, o[0], o[1] - o[0]);
    if (g) c.put(',');
  }
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
