// bc_raw_render.h -- the text of a raw-key plan's counts files (bc_engine_render_raw_counts / bc_engine_render_raw_merged):
// the lane-level pieces, shared by the kernels of bc_text_kernels.h (instantiated in bc_text.hip, next to the re-key step)
// and the host harness tests/render/raw_render_host.cpp (which runs this SAME code under AddressSanitizer; never a
// product path on the host).
//
// A raw-key plan (bc_plan_mode() == 2) keeps some capture as it was read, so its rows have no table index; what the
// device holds is a map of (key, count).  A key is a mixed-radix number over the scheme's groups: a known set gives its
// index (radix: the set's size), a raw capture its base-5 code  sum c_k 5^k  with A, C, T, G, N = 0 .. 4 and k the base's
// position (radix 5^len; the FIRST base is the least significant).
//
// The order of the lines.  Lines ascend by the tuple of the counted groups' digits, compared group by group in scheme
// order (Barcode_1 first); a digit is the set index of a known group and the base-5 code above of a raw one.  A per-
// sample file holds the tuples counted for that sample in that order, the merged file every tuple counted for some
// listed sample, once.  (Two raw captures therefore compare by their LAST differing base, in the order A < C < T < G < N.)
//
// How the order is made: the exported keys are re-keyed to  T * S + s  (T: the tuple's mixed-radix number, first counted
// group most significant; s: the sample index, S the number of samples, or S = 1 and s = 0 without a sample group) and
// sorted with their counts (bc_sort.h).  The view below reads that sorted array.  A "key index" of the text kernels is a
// position i in it:
//     per-sample view   position i has a line when its s is the view's sample
//     merged view       position i has a line when it is the first of its run of equal T (the run has at most S entries,
//                       ascending in s) and some listed sample counts; the lane looks its columns up in the run
// and the line is
//     f_0,f_1,..,f_{G-1},c_0,c_1,..\n
// f_g: the ID of the set's entry, copied from the label pool (bc_line.h) when group g is a known set, else the
// capture's bases "ACTGN"[c_k], first base first;  c_k: the count of the column in decimal ("0" for a sample that does
// not count the tuple; a sample may be listed twice, the list may be in any order).
//
// A line is measured and written from its END backwards (bc_line.h); inside a raw field the bases come out in
// ascending k, which is the order the code gives them up.
#ifndef BC_RAW_RENDER_H
#define BC_RAW_RENDER_H

#include "bc_line.h"

namespace bc {

struct RawRenderView {
  const uint64_t* keys;        // the sorted keys T * S + s
  const uint32_t* cnts;        // their counts
  const uint32_t* cols;        // sample index of every column (the per-sample view has one)
  const uint32_t* label_off;   // the label pool, as RenderView's
  const uint8_t* label_bytes;
  uint64_t n;                  // entries of keys / cnts
  uint32_t S;                  // samples: the radix of s
  uint32_t n_cols;
  uint32_t merged;             // 0: the per-sample view of cols[0] = sample
  uint32_t sample;
  uint32_t G;                  // counted groups
  uint32_t raw_len[kRenderMaxG];    // bases of a raw group; 0: a known set
  uint32_t off_start[kRenderMaxG];  // known set: where its offsets start in label_off
  uint64_t radix[kRenderMaxG];      // the set's size, or 5^raw_len
};

// the count of sample `s` for the tuple whose run starts at position i (0: the sample does not count it).  The run is
// the at most S entries from i on with the same T, ascending in s: a binary search for T * S + s among them.
BC_HD uint32_t raw_run_count(const RawRenderView& v, uint64_t i, uint64_t T, uint32_t s) {
  const uint64_t want = T * v.S + s;
  const uint64_t lo = key_lower_bound(v.keys, i, i + v.S < v.n ? i + v.S : v.n, want);
  return lo < v.n && lo < i + v.S && v.keys[lo] == want ? v.cnts[lo] : 0u;
}

// Position i -> does it have a line at all, and its tuple number T.  (The count columns follow from raw_col_count.)
BC_HD bool raw_has_line(const RawRenderView& v, uint64_t i, uint64_t& T) {
  uint64_t r = v.keys[i];
  const uint32_t s = (uint32_t)take_digit(r, v.S);
  T = r;
  if (!v.merged) return s == v.sample;
  if (i == 0) return true;
  uint64_t p = v.keys[i - 1];
  (void)take_digit(p, v.S);
  return p != T;
}

// column c of the line at position i
BC_HD uint32_t raw_col_count(const RawRenderView& v, uint64_t i, uint64_t T, uint32_t c) {
  return v.merged ? raw_run_count(v, i, T, v.cols[c]) : v.cnts[i];
}

// bytes of position i's line, '\n' included; 0: no line
BC_HD uint32_t raw_row_len(const RawRenderView& v, uint64_t i) {
  uint64_t T;
  if (!raw_has_line(v, i, T)) return 0;
  uint32_t any = 0, len = 1u + (v.G ? v.G - 1u : 0u);  // '\n' and the commas between the fields
  for (uint32_t c = 0; c < v.n_cols; ++c) {
    const uint32_t x = raw_col_count(v, i, T, c);
    any |= x;
    len += 1u + digits_u32(x);  // ",count"
  }
  if (v.merged && !any) return 0;
  uint64_t r = T;
  for (uint32_t g = v.G; g-- > 0;) {
    const uint64_t d = take_digit(r, v.radix[g]);
    len += v.raw_len[g] ? v.raw_len[g] : label_len(v.label_off, v.off_start[g], (uint32_t)d);
  }
  return len;
}

// Writes the part of position i's line (len = raw_row_len, not 0) that falls into the window dst[0 .. win); the line
// starts at window position `at` (bc_line.h).
template <typename Byte>
BC_HD void raw_row_write(const RawRenderView& v, uint64_t i, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  uint64_t T;
  (void)raw_has_line(v, i, T);
  LineCursor<Byte> c(dst, at, len, win);
  c.put('\n');
  for (uint32_t k = v.n_cols; k-- > 0;) {
    c.put_u32(raw_col_count(v, i, T, k));
    c.put(',');
  }
  uint64_t r = T;
  for (uint32_t g = v.G; g-- > 0;) {
    const uint64_t d = take_digit(r, v.radix[g]);
    if (v.raw_len[g]) {
      c.put_bases(d, v.raw_len[g]);
    } else {
      const uint32_t* o = v.label_off + v.off_start[g] + (uint32_t)d;
      c.put_label(v.label_bytes, o[0], o[1] - o[0]);
    }
    if (g) c.put(',');
  }
}

// the names bc_text_kernels.h reaches a view's lane code by
BC_HD uint64_t text_keys(const RawRenderView& v) { return v.n; }
BC_HD uint32_t text_line_len(const RawRenderView& v, uint64_t i) { return raw_row_len(v, i); }
template <typename Byte>
BC_HD void text_line_write(const RawRenderView& v, uint64_t i, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  raw_row_write(v, i, len, dst, at, win);
}

}  // namespace bc

#endif
