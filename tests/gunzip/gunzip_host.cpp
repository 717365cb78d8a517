// gunzip_host -- the span inflater's lane code (csrc/bc_gunzip.h) compiled for the host, with sanitizers: all five
// stages, in the order and with the arguments bc_gunzip_span_device gives them.  TEST-ONLY.
//
//   gunzip_host IN OUT
//
// IN : u64 src_bytes, start_bit, hist_bytes (0 or 32768), text_capacity, part_bytes; then the history, then the
//      compressed bytes.
// OUT: the fields of bc_gunzip_result (u32 status, detail; u64 text_bytes, end_bit; u32 member_end, segments, rejected,
//      crc32), then text_capacity bytes of text (0xAA where nothing was written).
//
// Every buffer is a heap block of exactly its own size, so AddressSanitizer sees any access outside it.  Exit status 0:
// ran (whatever the span's status); 2: bad arguments; a sanitizer report ends the process with its own status.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_gunzip.h"

using namespace bc;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t head[5];
  if (fread(head, 8, 5, f) != 5) return 2;
  const uint64_t src_bytes = head[0], start_bit = head[1], hist_bytes = head[2], capacity = head[3], part_bytes = head[4];
  if ((hist_bytes != 0 && hist_bytes != kGzHistory) || src_bytes >= (1ull << 28) || start_bit > 8 * src_bytes || capacity > 0x7FFFFFFFull ||
      part_bytes < 64 || (part_bytes & 7))
    return 2;
  uint8_t* hist = hist_bytes ? (uint8_t*)malloc(hist_bytes) : nullptr;
  uint8_t* src = (uint8_t*)malloc(src_bytes ? src_bytes : 1);
  if (hist_bytes && fread(hist, 1, hist_bytes, f) != hist_bytes) return 2;
  if (src_bytes && fread(src, 1, src_bytes, f) != src_bytes) return 2;
  fclose(f);
  uint8_t* text = (uint8_t*)malloc(capacity ? capacity : 1);
  memset(text, 0xAA, capacity ? capacity : 1);

  uint32_t crc_tab[256];
  for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = crc32_table_entry(i);
  InflateTables* T = new InflateTables;
  const uint32_t src_len = (uint32_t)src_bytes, n_parts = (uint32_t)((src_bytes + part_bytes - 1) / part_bytes);
  std::vector<uint32_t> cand(n_parts ? n_parts : 1, kGzNone);
  for (uint32_t p = 0; p < n_parts; ++p) {
    memset(T, 0xEE, sizeof *T);  // (no stage may depend on what an earlier wave left in the tables)
    cand[p] = gunzip_find(src, src_len, (uint32_t)start_bit, p * (uint32_t)part_bytes, (p + 1) * (uint32_t)part_bytes, *T, 0);
  }
  std::vector<GzMeasure> meas(n_parts + 1);
  for (uint32_t w = 0; w <= n_parts; ++w) {
    const uint32_t from = w == 0 ? (uint32_t)start_bit : cand[w - 1];
    GzMeasure m = {from, 0, kGzEndError, kGzNone, kInfOk};
    memset(T, 0xEE, sizeof *T);
    if (from != kGzNone) m = gunzip_measure(src, src_len, from, cand.data(), n_parts, (uint32_t)part_bytes, (uint32_t)capacity, *T, 0);
    meas[w] = m;
  }
  GzChain c = gunzip_chain((uint32_t)start_bit, cand.data(), n_parts, meas.data(), (uint32_t)capacity);
  uint32_t status = c.status, detail = c.detail, member_end = c.member_end, segments = (uint32_t)c.segs.size(), crc = 0;
  uint64_t text_bytes = c.text_bytes, end_bit = c.end_bit;
  if (c.status == kGzOk && !c.segs.empty()) {
    uint16_t* sym = (uint16_t*)malloc(c.text_bytes ? 2 * (size_t)c.text_bytes : 2);
    memset(sym, 0xFF, c.text_bytes ? 2 * (size_t)c.text_bytes : 2);
    for (const GzSegment& seg : c.segs) {
      memset(T, 0xEE, sizeof *T);
      const uint32_t st = gunzip_decode(src, src_len, seg, sym + seg.out_off, hist, (uint32_t)hist_bytes, *T, 0);
      if (st != kInfOk && status == kGzOk) {
        status = kGzBadStream;
        detail = st;
      }
    }
    uint32_t bad = 0;
    for (const GzSegment& seg : c.segs) gunzip_resolve_tail(sym, text, hist, (uint32_t)hist_bytes, seg, 0, 1, &bad);
    std::vector<uint32_t> seg_crc(c.segs.size(), 0);
    for (const GzSlice& sl : c.slices) seg_crc[sl.seg] ^= gunzip_resolve_slice(sym, text, hist, (uint32_t)hist_bytes, c.segs[sl.seg], sl, T->red, crc_tab, 0, &bad);
    for (size_t s = 0; s < c.segs.size(); ++s) crc = gunzip_crc_combine(crc, seg_crc[s], c.segs[s].out_bytes);
    if (bad && status == kGzOk) {
      status = kGzBadStream;
      detail = kInfBadSymbol;
    }
    free(sym);
    if (status != kGzOk) {
      text_bytes = 0;
      end_bit = start_bit;
      member_end = segments = crc = 0;
    }
  }
  delete T;
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  const uint32_t a[2] = {status, detail}, b[4] = {member_end, segments, c.rejected, crc};
  const uint64_t q[2] = {text_bytes, end_bit};
  fwrite(a, 4, 2, f);
  fwrite(q, 8, 2, f);
  fwrite(b, 4, 4, f);
  if (capacity) fwrite(text, 1, capacity, f);
  fclose(f);
  free(text);
  free(src);
  free(hist);
  return 0;
}
