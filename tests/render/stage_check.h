// stage_check -- what the five render harnesses (render_host, raw_render_host, wide_render_host, enrich_render_host,
// raw_enrich_render_host) do with a view once its input is parsed, through the names bc_text_kernels.h reaches a view's
// lane code by.  TEST-ONLY.
//
// Every line is written twice: whole, into a heap block of exactly text_line_len bytes (AddressSanitizer sees a byte
// outside it, a NUL left in it is a byte not written), and the way a wavefront stages it -- the lines of 64 keys laid
// end to end from position `pad`, cut into windows of `win` bytes that are heap blocks of their own.  Both texts must
// agree; then OUT is written: u64 lines, u64 bytes, the text.
// Returns the harness's exit status: 0: ran; 2: OUT cannot be written; 3: the length predicted and the bytes written
// differ; 4: the windowed text differs from the whole one.
#ifndef BC_TESTS_STAGE_CHECK_H
#define BC_TESTS_STAGE_CHECK_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

template <class View>
int stage_check(const View& v, uint32_t win, uint32_t pad, const char* out_path) {
  const uint64_t n = bc::text_keys(v);
  std::string whole;
  std::vector<uint32_t> lens(n);
  uint64_t lines = 0;
  for (uint64_t t = 0; t < n; ++t) {
    const uint32_t len = lens[t] = bc::text_line_len(v, t);
    if (!len) continue;
    ++lines;
    uint8_t* row = (uint8_t*)calloc(len, 1);
    bc::text_line_write(v, t, len, row, 0, len);
    if (memchr(row, 0, len) || row[len - 1] != '\n') return 3;
    whole.append((const char*)row, len);
    free(row);
  }
  // the way a wavefront stages 64 lines: window coordinates start at `pad`
  std::string staged;
  for (uint64_t c0 = 0; c0 < n; c0 += 64) {
    const uint64_t c1 = c0 + 64 < n ? c0 + 64 : n;
    uint64_t tot = 0;
    for (uint64_t t = c0; t < c1; ++t) tot += lens[t];
    for (uint64_t w0 = 0; w0 < pad + tot; w0 += win) {
      uint8_t* wb = (uint8_t*)calloc(win, 1);
      uint64_t start = pad;
      for (uint64_t t = c0; t < c1; ++t) {
        if (lens[t] && start < w0 + win && start + lens[t] > w0)
          bc::text_line_write(v, t, lens[t], wb, (int64_t)start - (int64_t)w0, win);
        start += lens[t];
      }
      const uint64_t a = w0 > pad ? w0 : pad, e = pad + tot < w0 + win ? pad + tot : w0 + win;
      if (a < e) {  // (a window smaller than the pad holds no text at all)
        if (memchr(wb + (a - w0), 0, e - a)) return 3;
        staged.append((const char*)wb + (a - w0), e - a);
      }
      free(wb);
    }
  }
  if (staged != whole) return 4;
  FILE* f = fopen(out_path, "wb");
  if (!f) return 2;
  const uint64_t out_head[2] = {lines, whole.size()};
  fwrite(out_head, 8, 2, f);
  fwrite(whole.data(), 1, whole.size(), f);
  fclose(f);
  return 0;
}

#endif
