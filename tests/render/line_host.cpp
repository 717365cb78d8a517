// line_host -- csrc/bc_line.h on its own, on the host: every member of the backwards cursor, the length side, take_digit
// and the run search, against snprintf and plain loops.  TEST-ONLY; built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_line_writer.py, which runs it once.
//
// A piece (one byte, a decimal, a label, a capture) is written whole, into a heap block of exactly its length, and then
// into windows of 1, 3, 4, 5 and 64 bytes -- heap blocks of exactly that size, so a byte outside the window is seen --
// at every start offset from -len to win.  What is visible in the window must be that part of the whole, every other
// byte of the window untouched, and the cursor must have moved back by the piece's length.
// Exit status 0 and "ok" on stdout, or 1 and the failed checks on stderr.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_line.h"

typedef bc::LineCursor<uint8_t> Cursor;

static int failures = 0;
static long checks = 0;

static void expect(bool ok, const char* what, const std::string& detail) {
  ++checks;
  if (ok) return;
  ++failures;
  fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

static const uint32_t kWindows[] = {1, 3, 4, 5, 64};
static const uint8_t kUntouched = 0xEE;

// `put` writes a piece whose text must be `want`
static void check_piece(const char* what, const std::string& want, const std::function<void(Cursor&)>& put) {
  const uint32_t len = (uint32_t)want.size();
  {
    uint8_t* whole = (uint8_t*)malloc(len);
    Cursor c(whole, 0, len, len);
    put(c);
    expect(c.p == 0, what, "whole: the cursor ends at " + std::to_string(c.p));
    expect(len == 0 || memcmp(whole, want.data(), len) == 0, what,
           "whole: got '" + std::string((const char*)whole, len) + "', want '" + want + "'");
    free(whole);
  }
  for (uint32_t win : kWindows)
    for (int64_t at = -(int64_t)len; at <= (int64_t)win; ++at) {
      uint8_t* dst = (uint8_t*)malloc(win);
      memset(dst, kUntouched, win);
      Cursor c(dst, at, len, win);
      put(c);
      bool same = c.p == at;
      for (int64_t w = 0; w < (int64_t)win; ++w) {
        const bool inside = w >= at && w < at + (int64_t)len;
        same = same && dst[w] == (inside ? (uint8_t)want[(size_t)(w - at)] : kUntouched);
      }
      expect(same, what, "'" + want + "' in a window of " + std::to_string(win) + " at " + std::to_string(at));
      free(dst);
    }
}

static uint64_t pow5(uint32_t n) {
  uint64_t x = 1;
  while (n--) x *= 5;
  return x;
}

static void check_decimals() {
  const uint64_t p32 = 1ull << 32, p19 = 10000000000000000000ull;
  const uint64_t values[] = {0, 9, 10, 99, 100, p32 - 1, p32, p19 - 1, p19, ~0ull};
  for (uint64_t x : values) {
    char text[32];
    snprintf(text, sizeof text, "%llu", (unsigned long long)x);
    expect(bc::digits_u64(x) == strlen(text), "digits_u64", text);
    check_piece("put_u64", text, [x](Cursor& c) { c.put_u64(x); });
    expect(bc::div10_u64(x) == x / 10, "div10_u64", text);
    if (x >= p32) continue;
    expect(bc::digits_u32((uint32_t)x) == strlen(text), "digits_u32", text);
    check_piece("put_u32", text, [x](Cursor& c) { c.put_u32((uint32_t)x); });
  }
}

static void check_bytes_and_labels() {
  check_piece("put", "\n", [](Cursor& c) { c.put('\n'); });
  check_piece("put x 3", "a,b", [](Cursor& c) {
    c.put('b');
    c.put(',');
    c.put('a');
  });
  // a pool of three labels -- empty, one byte, longer than the widest window -- between bytes that belong to none
  const std::string longer(70, 'L');
  const std::string pool_text = "<" + std::string("x") + longer.substr(0, 35) + "0123456789" + longer.substr(45) + ">";
  const std::string long_label = pool_text.substr(2, 70);
  const uint32_t off[4] = {1, 1, 2, 72};  // label d is pool[off[d] .. off[d + 1])
  uint8_t* pool = (uint8_t*)malloc(pool_text.size());
  memcpy(pool, pool_text.data(), pool_text.size());
  const std::string want[3] = {"", "x", long_label};
  for (uint32_t d = 0; d < 3; ++d) {
    expect(bc::label_len(off, 0, d) == want[d].size(), "label_len", std::to_string(d));
    check_piece("put_label", want[d], [&, d](Cursor& c) { c.put_label(pool, off[d], off[d + 1] - off[d]); });
  }
  const uint32_t later[6] = {9, 9, 1, 1, 2, 72};  // the same set, its offsets starting at entry 2
  expect(bc::label_len(later, 2, 2) == 70, "label_len", "off_start is added to the digit");
  // what a view does with several: a label, a comma, a label
  check_piece("label,label", "x," + long_label, [&](Cursor& c) {
    c.put_label(pool, off[2], 70);
    c.put(',');
    c.put_label(pool, off[1], 1);
  });
  free(pool);
}

static void check_captures() {
  for (uint32_t n : {1u, 13u, 14u, 27u}) {
    uint64_t mixed = 0;  // bases 0, 1, 2, 3, 4, 0, .. from the LAST base down, so the first base is not 0 for n > 1
    for (uint32_t k = 0; k < n; ++k) mixed = mixed * 5 + (n - k) % 5;
    for (uint64_t code : {(uint64_t)0, pow5(n) - 1, mixed}) {
      std::string want;
      uint64_t d = code;
      for (uint32_t k = 0; k < n; ++k) {  // the first base is the least significant digit
        want += "ACTGN"[d % 5];
        d /= 5;
      }
      const std::string what = "put_bases " + std::to_string(n) + " bases, code " + std::to_string(code);
      check_piece(what.c_str(), want, [code, n](Cursor& c) { c.put_bases(code, n); });
      // the wide view's way: reserve, then store at absolute window positions
      check_piece("reserve + store", want, [&want, n](Cursor& c) {
        c.reserve(n);
        for (uint32_t k = n; k-- > 0;) c.store(c.p + (int64_t)k, (uint8_t)want[k]);
      });
    }
  }
  for (uint32_t d = 0; d < 5; ++d) expect(bc::raw_base_char(d) == (uint32_t)"ACTGN"[d], "raw_base_char", std::to_string(d));
}

static void check_take_digit() {
  const uint64_t p32 = 1ull << 32;
  const uint64_t rs[] = {0, 1, 1220703124, 1220703125, 1220703126, p32 - 1, p32, p32 + 1, 5 * p32 + 7, ~0ull};
  const uint64_t radices[] = {1, 4, 1220703125 /* 5^13 */, p32 - 1, p32, p32 + 3, 6103515625ull /* 5^14 */, 7450580596923828125ull /* 5^27 */};
  for (uint64_t r0 : rs)
    for (uint64_t radix : radices) {
      uint64_t r = r0;
      const uint64_t d = bc::take_digit(r, radix);
      expect(d == r0 % radix && r == r0 / radix, "take_digit", std::to_string(r0) + " by " + std::to_string(radix));
    }
}

static void check_run_search() {
  // the keys of a raw-key view, T * S + s with S = 4: runs of T = 2 (s = 0, 1, 3), T = 5 (s = 2), T = 9 (s = 0, 3)
  const std::vector<uint64_t> src = {8, 9, 11, 22, 36, 39};
  const uint64_t n = src.size(), S = 4;
  uint64_t* keys = (uint64_t*)malloc(n * 8);  // exactly n entries: a read past the end is seen
  memcpy(keys, src.data(), n * 8);
  auto run_end = [&](uint64_t i) { return i + S < n ? i + S : n; };  // a run's bounds, as the views clip them
  expect(bc::key_lower_bound(keys, 3, 3, 22) == 3, "key_lower_bound", "an empty range");
  expect(bc::key_lower_bound(keys + n, 0, 0, 1) == 0, "key_lower_bound", "an empty range at the end of the keys");
  expect(bc::key_lower_bound(keys, 0, run_end(0), 9) == 1, "key_lower_bound", "a present key");
  expect(bc::key_lower_bound(keys, 0, run_end(0), 11) == 2, "key_lower_bound", "the last key of a run");
  expect(bc::key_lower_bound(keys, 0, run_end(0), 10) == 2, "key_lower_bound", "an absent key inside a run");
  expect(bc::key_lower_bound(keys, 0, run_end(0), 3) == 0, "key_lower_bound", "an absent key below every entry");
  expect(bc::key_lower_bound(keys, 0, run_end(0), 100) == 4, "key_lower_bound", "an absent key above every entry of the range");
  expect(run_end(4) == n && bc::key_lower_bound(keys, 4, run_end(4), 39) == 5, "key_lower_bound", "a range clipped by n, present");
  expect(bc::key_lower_bound(keys, 4, run_end(4), 38) == 5, "key_lower_bound", "a range clipped by n, absent inside");
  expect(bc::key_lower_bound(keys, 4, run_end(4), ~0ull) == n, "key_lower_bound", "a range clipped by n, above every entry");
  expect(bc::key_lower_bound(keys, 0, n, 22) == 3 && bc::key_lower_bound(keys, 0, n, 0) == 0, "key_lower_bound", "the whole array");
  free(keys);
}

int main() {
  check_decimals();
  check_bytes_and_labels();
  check_captures();
  check_take_digit();
  check_run_search();
  if (failures) {
    fprintf(stderr, "%d of %ld checks failed\n", failures, checks);
    return 1;
  }
  printf("ok %ld checks\n", checks);
  return 0;
}
