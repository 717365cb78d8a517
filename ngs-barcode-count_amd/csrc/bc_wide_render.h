// bc_wide_render.h -- the text of a wide-key plan's counts files (bc_engine_render_wide_counts /
// bc_engine_render_wide_merged): the lane-level pieces, shared by the kernels of bc_text.hip / bc_text_kernels.h and the
// host harness tests/render/wide_render_host.cpp (which runs this SAME code under AddressSanitizer; never a product path
// on the host).
//
// A wide-key plan (bc_long.h) counts under keys of W = 2 .. 8 u64: word 0 a fingerprint, words 1 .. W-1 the payload, in
// which a known set takes 32 bits of index at its key_bit and a raw capture of len bases three bit planes at key_bit,
// key_bit + len, key_bit + 2 len (ASCII bit 1, ASCII bit 2, 'N').  The sample group, when the scheme has one, is the
// first group: its index is payload bits 0 .. 31.
//
// The order of the lines is bc_raw_render.h's, unchanged past 27 bases: lines ascend by the tuple of the counted
// groups' digits, group by group in scheme order; a known group's digit is its set index, a raw capture's the number
// sum c_k 5^k  with A, C, T, G, N = 0 .. 4 and the FIRST base least significant.  That number no longer fits a word, so
// the order is made from an ORDER KEY of K u64 (wide_order_word), compared word by word as unsigned numbers with word
// K-1 the most significant.  From bit 0 of word 0 upwards it holds
//     the sample index                      bit length of S - 1 (nothing without a sample group, or with one sample)
//     the counted groups, the LAST first    a known set: bit length of n_refs - 1;  a raw capture: 3 bits per base, the
//                                           code 0 .. 4 of base k at bits 3k .. 3k+2 of the field
// so that the first counted group is the most significant field and, inside a capture, the last base the most
// significant digit: comparing two captures' fields as numbers compares their base-5 codes.  K never passes W - 1: every
// field is at most as wide as in the payload.
//
// The view reads the keys and counts gathered into that order.  A "key index" of the text kernels is a position i:
//     per-sample view   position i has a line when its sample field is the view's sample
//     merged view       position i has a line when it is the first of its run of equal tuples (the payload with the
//                       sample field masked; at most S entries, ascending in s) and some listed sample counts
// and the line is bc_raw_render.h's, byte for byte:  f_0,f_1,..,f_{G-1},c_0,c_1,..\n  -- measured and written from its
// END backwards (bc_line.h).
#ifndef BC_WIDE_RENDER_H
#define BC_WIDE_RENDER_H

#include "bc_line.h"

namespace bc {

// payload -> order key: where every field is read and where it goes
struct WideOrder {
  uint32_t W;             // words per key (fingerprint + payload)
  uint32_t K;             // words per order key
  uint32_t G;             // counted groups
  uint32_t sample_bits;   // 32: payload bits 0 .. 31 are the sample index; 0: no sample group
  uint32_t sample_obits;  // bits of the sample index in the order key, at order bit 0
  uint32_t raw_len[kRenderMaxG];  // bases of a raw group; 0: a known set
  uint32_t key_bit[kRenderMaxG];  // payload bit of the group's field
  uint32_t obits[kRenderMaxG];    // bits of the group's field in the order key
  uint32_t obit[kRenderMaxG];     // ... and its first bit there
};

struct WideRenderView {
  const uint64_t* keys;        // the keys in file order, W words each (word 0 is not looked at)
  const uint32_t* cnts;        // their counts
  const uint32_t* cols;        // sample index of every column (the per-sample view has one)
  const uint32_t* label_off;   // the label pool, as RenderView's
  const uint8_t* label_bytes;
  uint64_t n;                  // entries of keys / cnts
  uint32_t W;
  uint32_t S;                  // samples
  uint32_t sample_bits;        // as WideOrder's
  uint32_t n_cols;
  uint32_t merged;             // 0: the per-sample view of cols[0] = sample
  uint32_t sample;
  uint32_t G;
  uint32_t raw_len[kRenderMaxG];
  uint32_t key_bit[kRenderMaxG];
  uint32_t n_ids[kRenderMaxG];      // known set: its size (an index at or above it has an empty field)
  uint32_t off_start[kRenderMaxG];  // known set: where its offsets start in label_off
};

BC_HD uint32_t wide_bit_length(uint32_t x) {
  uint32_t b = 0;
  while (x) {
    ++b;
    x >>= 1;
  }
  return b;
}

// obits[] (known groups), raw_len[], sample_obits filled in -> obits[] of the raw groups, obit[] and K
BC_HD void wide_order_layout(WideOrder& o) {
  uint32_t bit = o.sample_obits;
  for (uint32_t g = o.G; g-- > 0;) {
    if (o.raw_len[g]) o.obits[g] = 3u * o.raw_len[g];
    o.obit[g] = bit;
    bit += o.obits[g];
  }
  o.K = bit ? (bit + 63u) / 64u : 1u;
}

// n (1 .. 32) payload bits from bit `at` on; a field may straddle two words (the second is only read when it does)
BC_HD uint64_t wide_bits(const uint64_t* pay, uint32_t at, uint32_t n) {
  const uint32_t w = at >> 6, sh = at & 63u;
  uint64_t x = pay[w] >> sh;
  if (sh + n > 64u) x |= pay[w + 1u] << (64u - sh);
  return x & ((1ull << n) - 1ull);
}

// bit j of the three plane pieces -> the base's code 0 .. 4 (A, C, T, G, N)
BC_HD uint32_t wide_base_code(uint64_t p1, uint64_t p2, uint64_t pn, uint32_t j) {
  return ((pn >> j) & 1ull) ? 4u : (uint32_t)(((p1 >> j) & 1ull) | (((p2 >> j) & 1ull) << 1));
}

// x, whose bit 0 is order bit `pos`, as it falls into the order word that starts at order bit `lo`
BC_HD uint64_t wide_place(uint64_t x, uint32_t pos, uint32_t lo) { return pos >= lo ? x << (pos - lo) : x >> (lo - pos); }

// word w (0: least significant) of the order key of the payload `pay`.  Nothing is kept in a local array: every field
// that reaches into the word is read from the payload for it.
BC_HD uint64_t wide_order_word(const WideOrder& o, const uint64_t* pay, uint32_t w) {
  const uint32_t lo = 64u * w, hi = lo + 64u;  // the word holds order bits [lo, hi)
  uint64_t out = 0;
  if (w == 0 && o.sample_obits) out = wide_bits(pay, 0, 32) & ((1ull << o.sample_obits) - 1ull);
  for (uint32_t g = 0; g < o.G; ++g) {
    const uint32_t b0 = o.obit[g], nb = o.obits[g];
    if (nb == 0 || b0 >= hi || b0 + nb <= lo) continue;
    if (!o.raw_len[g]) {
      out |= wide_place(wide_bits(pay, o.key_bit[g], 32) & ((1ull << nb) - 1ull), b0, lo);
      continue;
    }
    // the bases whose three bits touch [lo, hi): at most 23 of them
    const uint32_t len = o.raw_len[g];
    const uint32_t k0 = lo > b0 ? (lo - b0) / 3u : 0u;
    uint32_t k1 = (hi - b0 + 2u) / 3u;
    if (k1 > len) k1 = len;
    const uint32_t cnt = k1 - k0, at = o.key_bit[g] + k0;
    const uint64_t p1 = wide_bits(pay, at, cnt), p2 = wide_bits(pay, at + len, cnt), pn = wide_bits(pay, at + 2u * len, cnt);
    for (uint32_t j = 0; j < cnt; ++j) out |= wide_place(wide_base_code(p1, p2, pn, j), b0 + 3u * (k0 + j), lo);
  }
  return out;
}

BC_HD const uint64_t* wide_payload(const WideRenderView& v, uint64_t i) { return v.keys + i * v.W + 1u; }

BC_HD uint32_t wide_sample_of(const WideRenderView& v, uint64_t i) {
  return v.sample_bits ? (uint32_t)wide_bits(wide_payload(v, i), 0, 32) : 0u;
}

// do positions i and j hold the same tuple (the payload, the sample field aside)?
BC_HD bool wide_same_tuple(const WideRenderView& v, uint64_t i, uint64_t j) {
  const uint64_t *a = wide_payload(v, i), *b = wide_payload(v, j);
  uint64_t diff = (a[0] ^ b[0]) >> v.sample_bits;
  for (uint32_t w = 1; w + 1u < v.W; ++w) diff |= a[w] ^ b[w];
  return diff == 0;
}

// one past the run of position i's tuple: the run is at most S entries long and nothing equal follows it
BC_HD uint64_t wide_run_end(const WideRenderView& v, uint64_t i) {
  uint64_t lo = i + 1u, hi = i + v.S < v.n ? i + v.S : v.n;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (wide_same_tuple(v, i, mid))
      lo = mid + 1u;
    else
      hi = mid;
  }
  return lo;
}

// the count of sample `s` in the run [i, e) (ascending in s); 0: the sample does not count the tuple
BC_HD uint32_t wide_run_count(const WideRenderView& v, uint64_t i, uint64_t e, uint32_t s) {
  uint64_t lo = i, hi = e;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (wide_sample_of(v, mid) < s)
      lo = mid + 1u;
    else
      hi = mid;
  }
  return lo < e && wide_sample_of(v, lo) == s ? v.cnts[lo] : 0u;
}

// Position i -> does it have a line at all, and (merged view) where its run ends
BC_HD bool wide_has_line(const WideRenderView& v, uint64_t i, uint64_t& run_end) {
  run_end = i + 1u;
  if (!v.merged) return wide_sample_of(v, i) == v.sample;
  if (i != 0 && wide_same_tuple(v, i - 1u, i)) return false;
  run_end = wide_run_end(v, i);
  return true;
}

BC_HD uint32_t wide_col_count(const WideRenderView& v, uint64_t i, uint64_t run_end, uint32_t c) {
  return v.merged ? wide_run_count(v, i, run_end, v.cols[c]) : v.cnts[i];
}

// known group g of position i: where its ID starts in label_bytes, and its length
BC_HD uint32_t wide_label(const WideRenderView& v, uint64_t i, uint32_t g, uint32_t& n) {
  const uint32_t idx = (uint32_t)wide_bits(wide_payload(v, i), v.key_bit[g], 32);
  n = 0;
  if (idx >= v.n_ids[g]) return 0;
  const uint32_t* o = v.label_off + v.off_start[g] + idx;
  n = o[1] - o[0];
  return o[0];
}

// bytes of position i's line, '\n' included; 0: no line
BC_HD uint32_t wide_row_len(const WideRenderView& v, uint64_t i) {
  uint64_t e;
  if (!wide_has_line(v, i, e)) return 0;
  uint32_t any = 0, len = 1u + (v.G ? v.G - 1u : 0u);  // '\n' and the commas between the fields
  for (uint32_t c = 0; c < v.n_cols; ++c) {
    const uint32_t x = wide_col_count(v, i, e, c);
    any |= x;
    len += 1u + digits_u32(x);  // ",count"
  }
  if (v.merged && !any) return 0;
  for (uint32_t g = 0; g < v.G; ++g) {
    if (v.raw_len[g]) {
      len += v.raw_len[g];
    } else {
      uint32_t n;
      (void)wide_label(v, i, g, n);
      len += n;
    }
  }
  return len;
}

// Writes the part of position i's line (len = wide_row_len, not 0) that falls into the window dst[0 .. win); the line
// starts at window position `at` (bc_line.h).
template <typename Byte>
BC_HD void wide_row_write(const WideRenderView& v, uint64_t i, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  uint64_t e;
  (void)wide_has_line(v, i, e);
  const uint64_t* pay = wide_payload(v, i);
  LineCursor<Byte> c(dst, at, len, win);
  c.put('\n');
  for (uint32_t k = v.n_cols; k-- > 0;) {
    c.put_u32(wide_col_count(v, i, e, k));
    c.put(',');
  }
  for (uint32_t g = v.G; g-- > 0;) {
    if (v.raw_len[g]) {
      // the capture lies at [p, p + n) once reserved: base k at p + k, read from the planes 32 bases at a time
      const uint32_t n = v.raw_len[g];
      c.reserve(n);
      for (uint32_t k0 = 0; k0 < n; k0 += 32u) {
        const uint32_t cnt = n - k0 < 32u ? n - k0 : 32u;
        if (c.p + (int64_t)(k0 + cnt) <= 0 || c.p + (int64_t)k0 >= (int64_t)win) continue;  // (all of it outside the window)
        const uint32_t b = v.key_bit[g] + k0;
        const uint64_t p1 = wide_bits(pay, b, cnt), p2 = wide_bits(pay, b + n, cnt), pn = wide_bits(pay, b + 2u * n, cnt);
        for (uint32_t j = 0; j < cnt; ++j) c.store(c.p + (int64_t)(k0 + j), raw_base_char(wide_base_code(p1, p2, pn, j)));
      }
    } else {
      uint32_t n;
      const uint32_t a = wide_label(v, i, g, n);
      c.put_label(v.label_bytes, a, n);
    }
    if (g) c.put(',');
  }
}

// the names bc_text_kernels.h reaches a view's lane code by
BC_HD uint64_t text_keys(const WideRenderView& v) { return v.n; }
BC_HD uint32_t text_line_len(const WideRenderView& v, uint64_t i) { return wide_row_len(v, i); }
template <typename Byte>
BC_HD void text_line_write(const WideRenderView& v, uint64_t i, uint32_t len, Byte* dst, int64_t at, uint32_t win) {
  wide_row_write(v, i, len, dst, at, win);
}

}  // namespace bc

#endif
