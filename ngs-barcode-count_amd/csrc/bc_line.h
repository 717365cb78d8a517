// bc_line.h -- what the lane code of every text view (bc_render.h, bc_raw_render.h, bc_wide_render.h,
// bc_enrich_render.h, bc_raw_enrich_render.h) measures and writes a line with.  Shared by the kernels of
// bc_text_kernels.h and the host harnesses under tests/render/ (line_host.cpp drives this header alone, under
// AddressSanitizer; never a product path on the host).
//
// A line is measured and written from its END backwards, in the order a key gives up its digits (innermost first), so
// no digit is ever kept in a local array.  The writer is handed a window dst[0 .. win) and the position `at` where the
// line starts in it, which may be negative or beyond the window: a wavefront stages the text of its 64 keys window by
// window, and a long line crosses windows.  Only bytes inside the window are touched.
//
// IDs are copied verbatim from the label pool: group g's offsets are label_off[off_start[g] .. off_start[g] + N_g],
// byte positions in label_bytes.  A raw capture is a base-5 code  sum c_k 5^k  (A, C, T, G, N = 0 .. 4, the FIRST base
// least significant).
#ifndef BC_LINE_H
#define BC_LINE_H

#include "bc_intrin.h"

namespace bc {

constexpr int kRenderMaxG = 18;                  // counted barcodes: as many as a plan may have groups (kMaxGroups)
constexpr uint32_t kRenderMaxLine = 1u << 25;    // longest line taken: 64 of them stay below 2^31 bytes

// ---- the length side ----

// decimal digits of x: 1 .. 10
BC_HD uint32_t digits_u32(uint32_t x) {
  return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) +
         (x >= 100000000u) + (x >= 1000000000u);
}

// decimal digits of x: 1 .. 20
BC_HD uint32_t digits_u64(uint64_t x) {
  if ((x >> 32) == 0) return digits_u32((uint32_t)x);
  uint32_t d = 10;
  uint64_t p = 10000000000ull;  // 10^d
  while (d < 19 && x >= p) {
    p *= 10u;
    ++d;
  }
  return d + (x >= p);  // (at d = 19 p = 10^19 still fits; 10^20 does not)
}

// bytes of entry d of the set whose offsets start at off_start
BC_HD uint32_t label_len(const uint32_t* label_off, uint32_t off_start, uint32_t d) {
  const uint32_t* o = label_off + off_start + d;
  return o[1] - o[0];
}

// ---- digits of a key ----

// r -> its least significant digit of the given radix; r loses it.  (One 64-bit division at most matters: after the
// innermost groups r fits 32 bits for every table that fits a GPU.)
BC_HD uint64_t take_digit(uint64_t& r, uint64_t radix) {
  if (((r | radix) >> 32) == 0) {
    const uint32_t r32 = (uint32_t)r, n32 = (uint32_t)radix, q = r32 / n32;
    r = q;
    return r32 - q * n32;
  }
  const uint64_t q = r / radix;
  const uint64_t d = r - q * radix;
  r = q;
  return d;
}

// x / 10 by multiplication: the high half of x * ceil(2^67 / 10), shifted by 3 -- exact for every u64
BC_HD uint64_t div10_u64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(x, 0xCCCCCCCCCCCCCCCDull) >> 3;
#else
  return (uint64_t)(((unsigned __int128)x * 0xCCCCCCCCCCCCCCCDull) >> 64) >> 3;
#endif
}

// "ACTGN"[d] without a table in memory
BC_HD uint32_t raw_base_char(uint32_t d) { return (uint32_t)((0x4E47544341ull >> (8u * d)) & 0xFFu); }

// the first position of [lo, hi) whose key is not below `want`; hi: there is none.  keys ascend over the range.
BC_HD uint64_t key_lower_bound(const uint64_t* keys, uint64_t lo, uint64_t hi, uint64_t want) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < want)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ---- the backwards cursor ----

// Writes a line of `len` bytes that starts at window position `at`, last byte first.  A view's lane function makes one
// on its stack and calls its members; nothing takes its address, so it lives in registers.
template <typename Byte>
struct LineCursor {
  Byte* dst;
  int64_t p;  // one past the byte written next
  uint32_t win;

  BC_HD LineCursor(Byte* dst_, int64_t at, uint32_t len, uint32_t win_) : dst(dst_), p(at + (int64_t)len), win(win_) {}

  // window position w takes ch, when it is inside the window
  BC_HD void store(int64_t w, uint32_t ch) {
    if (w >= 0 && w < (int64_t)win) dst[w] = (Byte)ch;
  }
  // the next n bytes are the caller's to store(): they lie at [p, p + n) afterwards
  BC_HD void reserve(uint32_t n) { p -= (int64_t)n; }
  BC_HD void put(uint32_t ch) {
    --p;
    store(p, ch);
  }
  BC_HD void put_u32(uint32_t x) {
    do {
      const uint32_t q = x / 10u;  // (a multiplication: the divisor is a constant)
      put('0' + (x - q * 10u));
      x = q;
    } while (x);
  }
  BC_HD void put_u64(uint64_t x) {
    do {
      const uint64_t q = div10_u64(x);
      put('0' + (uint32_t)(x - q * 10u));
      x = q;
    } while (x);
  }
  // the label pool[a .. a + n): it lies at [p - n, p), and only its bytes inside the window are touched
  BC_HD void put_label(const uint8_t* pool, uint32_t a, uint32_t n) {
    int64_t lo = p - (int64_t)n, hi = p;
    p = lo;
    if (lo < 0) lo = 0;
    if (hi > (int64_t)win) hi = (int64_t)win;
    for (int64_t w = lo; w < hi; ++w) dst[w] = (Byte)pool[a + (uint32_t)(w - p)];
  }
  // the n bases of the capture with base-5 code d, first base first: base k at p + k, and the code gives up base 0 first
  BC_HD void put_bases(uint64_t d, uint32_t n) {
    reserve(n);
    for (uint32_t k = 0; k < n; ++k) {
      uint32_t c5;
      if ((d >> 32) == 0) {
        const uint32_t d32 = (uint32_t)d, q = d32 / 5u;
        c5 = d32 - q * 5u;
        d = q;
      } else {
        const uint64_t q = d / 5u;
        c5 = (uint32_t)(d - q * 5u);
        d = q;
      }
      store(p + (int64_t)k, raw_base_char(c5));
    }
  }
};

}  // namespace bc

#endif
