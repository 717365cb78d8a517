// bc_raw_enrich_render.h -- the text of a raw-key plan's Single and Double enrichment files
// (bc_engine_render_raw_enriched / bc_engine_render_raw_enriched_merged): the lane-level pieces, shared by the kernels of
// bc_text.hip (the projection kernel; the text kernels of bc_text_kernels.h) and the host harness
// tests/render/raw_enrich_render_host.cpp (which runs this SAME code under AddressSanitizer; never a product path on the
// host).
//
// A raw-key plan has no table to sum at (bc_enrich.hip's trick): what the device holds is the sorted array of
// (T * S + s, count) of the raw-key renderer (bc_raw_render.h; T: the tuple's mixed-radix number over the counted
// groups, first group most significant; s: the sample index of S).  The sums are made from it in three steps per
// projection:
//   project   every entry -> a key that keeps only the digits of the projection, its count as the value
//                 Single, group g        d_g * S + s
//                 Double, pair g < h     (d_g * R_h + d_h) * S + s         R_h: group h's radix
//             (raw_enrich_project below; both are sub-products of T * S + s, so they fit a word whenever the key does)
//   sort      bc_sort.h, over the bit length of the projection's bound only
//   reduce    bc_reduce.h: one (projected key, u64 sum) per run of equal keys
// A digit is the raw-key renderer's: the set index of a known group, the base-5 code  sum c_k 5^k  (A, C, T, G, N =
// 0 .. 4, first base least significant) of a raw one.  Entries of a known set whose IDs are byte-equal are ONE key of the
// reference's maps (add_single / add_double key them by text, info.rs:840-904): the digit of a known group is first
// replaced by the smallest index of the set with the same ID (canon, as the dense enrichment writers), so such entries
// project to the same key and are summed by the reduction.  Text that coincides ACROSS groups or pairs (possible only
// with an empty ID) is NOT merged.
//
// What the view reads: per kind the projections' results back to back -- G segments for Single, G (G - 1) / 2 for
// Double in add_double's order (0,1), (0,2), .., (1,2), .. -- each an array of (projected key, sum) ascending by key,
// and the table of segment starts (n_seg + 1 entries).  A "key index" of the text kernels is a position i in the
// concatenated arrays; the lane finds its segment by a search over the starts.  Inside a segment the structure is the
// raw-key renderer's own: entries with the same digits differ only in s and form a run of at most S entries,
// ascending in s.
//     per-sample view   position i has a line when its s is the view's sample
//     merged view       position i has a line when it is the first of its run and some listed sample has a sum that is
//                       not zero; the lane looks its columns up in the run (binary search)
// and the line is G comma-joined fields of which only field g (Single) or fields g and h (Double) hold text -- the ID
// from the label pool for a known group, the bases "ACTGN"[c_k], first base first, for a raw one -- then one decimal
// u64 sum per column ("0" for a sample that is absent; a sample may be listed twice, in any order) and '\n':
//     ,ACGTACGT,,7\n            Single of group 1 of three raw 8-base groups
//     ACGTACGT,,TTGCAAGC,3\n    Double of (0,2)
// Lines come in ascending position: Single by (g, digit), Double by (pair, d_g, d_h).
//
// A line is measured and written from its END backwards (bc_line.h).
#ifndef BC_RAW_ENRICH_RENDER_H
#define BC_RAW_ENRICH_RENDER_H

#include "bc_enrich_render.h"  // kEnrichSingle / kEnrichDouble

namespace bc {

// One projection of the sorted keys T * S + s.
struct RawEnrichProj {
  const uint32_t* canon;             // canon[canon_off[g] + i]: the smallest index of known set g with i's ID; NULL: no
                                     // set shares an ID
  uint32_t S;                        // samples: the radix of s
  uint32_t G;                        // counted groups
  uint32_t g, h;                     // the groups kept, g < h; h == g: a Single
  uint32_t known[kRenderMaxG];       // 1: a known set (its digit goes through canon)
  uint32_t canon_off[kRenderMaxG];   // where known set g starts in canon
  uint64_t radix[kRenderMaxG];       // the set's size, or 5^len
};

// key = T * S + s  ->  the projected key
BC_HD uint64_t raw_enrich_project(const RawEnrichProj& p, uint64_t key) {
  uint64_t r = key;
  const uint64_t s = take_digit(r, p.S);
  uint64_t dg = 0, dh = 0;
  for (uint32_t f = p.G; f-- > 0;) {  // (the digits come off innermost group first; only two of them are kept)
    uint64_t d = take_digit(r, p.radix[f]);
    if (f != p.g && f != p.h) continue;
    if (p.canon && p.known[f]) d = p.canon[p.canon_off[f] + (uint32_t)d];
    if (f == p.h) dh = d;
    if (f == p.g) dg = d;
  }
  return (p.h == p.g ? dg : dg * p.radix[p.h] + dh) * p.S + s;
}

// the largest projected key + 1 (what bounds the sort's passes); it divides the plan's key space, so it fits a word
BC_HD uint64_t raw_enrich_bound(const RawEnrichProj& p) {
  return (p.h == p.g ? p.radix[p.g] : p.radix[p.g] * p.radix[p.h]) * p.S;
}

struct RawEnrichView {
  const uint64_t* keys;        // the segments' projected keys, back to back
  const uint64_t* sums;        // their sums
  const uint64_t* seg_start;   // n_seg + 1 positions: segment q is [seg_start[q], seg_start[q + 1])
  const uint32_t* cols;        // sample index of every column (the per-sample view has one)
  const uint32_t* label_off;   // the label pool, as RenderView's
  const uint8_t* label_bytes;
  uint64_t n;                  // entries of keys / sums = seg_start[n_seg]
  uint32_t S;
  uint32_t n_cols;
  uint32_t merged;             // 0: the per-sample view of cols[0] = sample
  uint32_t sample;
  uint32_t G;
  uint32_t kind;               // kEnrichSingle | kEnrichDouble
  uint32_t n_seg;              // G, or G (G - 1) / 2
  uint32_t raw_len[kRenderMaxG];    // bases of a raw group; 0: a known set
  uint32_t off_start[kRenderMaxG];  // known set: where its offsets start in label_off
  uint64_t radix[kRenderMaxG];
};

// What a position stands for.
struct RawEnrichLine {
  uint64_t lo, hi;   // its segment [lo, hi)
  uint64_t D;        // the projected key without its sample digit
  uint32_t g, h;     // the fields that hold text (h == g: a Single)
  uint32_t s;        // its sample digit
};

// position i (< v.n) -> its segment: the last one that starts at or before i (empty segments share their start with
// the next one; the search steps over them)
BC_HD uint32_t raw_enrich_segment(const RawEnrichView& v, uint64_t i) {
  uint32_t lo = 0, hi = v.n_seg;  // the answer is in [lo, hi)
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (v.seg_start[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

BC_HD RawEnrichLine raw_enrich_line(const RawEnrichView& v, uint64_t i) {
  RawEnrichLine L;
  const uint32_t q = raw_enrich_segment(v, i);
  L.lo = v.seg_start[q];
  L.hi = v.seg_start[q + 1u];
  L.g = L.h = q;
  if (v.kind == kEnrichDouble) {  // q -> (g, h) in add_double's order
    uint32_t left = q, g = 0;
    while (g + 2u < v.G && left >= v.G - 1u - g) left -= v.G - 1u - g++;
    L.g = g;
    L.h = g + 1u + left;
  }
  uint64_t r = v.keys[i];
  L.s = (uint32_t)take_digit(r, v.S);
  L.D = r;
  return L;
}

// the sum of sample `s` for the run of L's digits that starts at position i (0: the sample is absent): a binary search
// for D * S + s among the at most S entries from i on, inside the segment
BC_HD uint64_t raw_enrich_run_sum(const RawEnrichView& v, const RawEnrichLine& L, uint64_t i, uint32_t s) {
  const uint64_t want = L.D * v.S + s;
  const uint64_t end = i + v.S < L.hi ? i + v.S : L.hi;
  const uint64_t lo = key_lower_bound(v.keys, i, end, want);
  return lo < end && v.keys[lo] == want ? v.sums[lo] : 0ull;
}

// does position i have a line at all
BC_HD bool raw_enrich_has_line(const RawEnrichView& v, const RawEnrichLine& L, uint64_t i) {
  if (!v.merged) return L.s == v.sample;
  if (i == L.lo) return true;
  uint64_t p = v.keys[i - 1];
  (void)take_digit(p, v.S);
  return p != L.D;
}

BC_HD uint64_t raw_enrich_col_sum(const RawEnrichView& v, const RawEnrichLine& L, uint64_t i, uint32_t c) {
  return v.merged ? raw_enrich_run_sum(v, L, i, v.cols[c]) : v.sums[i];
}

// bytes of the text of group f's digit d
BC_HD uint32_t raw_enrich_field_len(const RawEnrichView& v, uint32_t f, uint64_t d) {
  return v.raw_len[f] ? v.raw_len[f] : label_len(v.label_off, v.off_start[f], (uint32_t)d);
}

// bytes of position i's line, '\n' included; 0: no line
BC_HD uint32_t raw_enrich_row_len(const RawEnrichView& v, uint64_t i) {
  const RawEnrichLine L = raw_enrich_line(v, i);
  if (!raw_enrich_has_line(v, L, i)) return 0;
  uint64_t any = 0;
  uint32_t len = 1u + (v.G ? v.G - 1u : 0u);  // '\n' and the commas between the fields
  for (uint32_t c = 0; c < v.n_cols; ++c) {
    const uint64_t x = raw_enrich_col_sum(v, L, i, c);
    any |= x;
    len += 1u + digits_u64(x);  // ",count"
  }
  if (v.merged && !any) return 0;
  uint64_t r = L.D;
  if (L.h != L.g) len += raw_enrich_field_len(v, L.h, take_digit(r, v.radix[L.h]));
  return len + raw_enrich_field_len(v, L.g, r);
}

// Writes the part of position i's line (len = raw_enrich_row_len, not 0) that falls into the window dst[0 .. win); the
// line starts at window position `at` (bc_line.h).
template <typename Byte>
BC_HD void raw_enrich_row_write(const RawEnrichView& v, uint64_t i, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  const RawEnrichLine L = raw_enrich_line(v, i);
  LineCursor<Byte> c(dst, at, len, win);
  c.put('\n');
  for (uint32_t m = v.n_cols; m-- > 0;) {
    c.put_u64(raw_enrich_col_sum(v, L, i, m));
    c.put(',');
  }
  uint64_t r = L.D;
  for (uint32_t f = v.G; f-- > 0;) {
    if (f == L.h || f == L.g) {  // (h comes first, and takes its digit off: what is left is g's)
      const uint64_t d = f == L.g ? r : take_digit(r, v.radix[f]);
      if (v.raw_len[f]) {
        c.put_bases(d, v.raw_len[f]);
      } else {
        const uint32_t* o = v.label_off + v.off_start[f] + (uint32_t)d;
        c.put_label(v.label_bytes, o[0], o[1] - o[0]);
      }
    }
    if (f) c.put(',');
  }
}

// the names bc_text_kernels.h reaches a view's lane code by
BC_HD uint64_t text_keys(const RawEnrichView& v) { return v.n; }
BC_HD uint32_t text_line_len(const RawEnrichView& v, uint64_t i) { return raw_enrich_row_len(v, i); }
template <typename Byte>
BC_HD void text_line_write(const RawEnrichView& v, uint64_t i, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  raw_enrich_row_write(v, i, len, dst, at, win);
}

}  // namespace bc

#endif
