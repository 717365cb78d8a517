// render_host -- the text renderer's lane code (csrc/bc_render.h) compiled for the host, with sanitizers.  TEST-ONLY.
//
//   render_host IN OUT
//
// IN : u32 G, u32 n_cols, u32 S, u32 win, u32 pad, u32 has_bits, then G x u32 N_g, n_cols x u32 column, per group N_g x
//      {u32 len, bytes}, S * T x u32 table, and with has_bits (S * T + 31) / 32 x u32 bit map.
// OUT: u64 lines, u64 bytes, then the text of the tuples 0 .. T-1 for those columns.
//
// Every line is written twice, whole and staged through windows, and both texts must agree (stage_check.h).
// Exit status 0: ran; 2: bad arguments; 3: the length predicted and the bytes written differ; 4: the windowed text
// differs from the whole one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_render.h"
#include "stage_check.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[6];
  if (!rd(f, head, sizeof head)) return 2;
  const uint32_t G = head[0], n_cols = head[1], S = head[2], win = head[3], pad = head[4], has_bits = head[5];
  if (G > (uint32_t)bc::kRenderMaxG || win == 0 || pad > 3) return 2;
  bc::RenderView v;
  memset(&v, 0, sizeof v);
  v.G = G;
  v.n_cols = n_cols;
  v.T = 1;
  if (!rd(f, v.n, G * 4)) return 2;
  for (uint32_t g = 0; g < G; ++g) v.T *= v.n[g];
  std::vector<uint32_t> cols(n_cols ? n_cols : 1);
  if (!rd(f, cols.data(), n_cols * 4)) return 2;
  std::vector<uint32_t> off;
  std::string bytes;
  for (uint32_t g = 0; g < G; ++g) {
    v.off_start[g] = (uint32_t)off.size();
    for (uint32_t i = 0; i < v.n[g]; ++i) {
      uint32_t len;
      if (!rd(f, &len, 4)) return 2;
      std::string id(len, '\0');
      if (!rd(f, &id[0], len)) return 2;
      off.push_back((uint32_t)bytes.size());
      bytes += id;
    }
    off.push_back((uint32_t)bytes.size());
  }
  const uint64_t entries = (uint64_t)S * v.T;
  // (heap blocks of exactly their own size, so a read outside the table, the offsets or the IDs is seen)
  uint32_t* table = (uint32_t*)malloc(entries ? entries * 4 : 1);
  if (!rd(f, table, entries * 4)) return 2;
  uint32_t* bits = nullptr;
  if (has_bits) {
    bits = (uint32_t*)malloc(((entries + 31) / 32) * 4 + 1);
    if (!rd(f, bits, ((entries + 31) / 32) * 4)) return 2;
  }
  fclose(f);
  uint32_t* d_off = (uint32_t*)malloc(off.size() * 4 + 1);
  memcpy(d_off, off.data(), off.size() * 4);
  uint8_t* d_bytes = (uint8_t*)malloc(bytes.size() + 1);
  memcpy(d_bytes, bytes.data(), bytes.size());
  for (uint32_t c = 0; c < n_cols; ++c)
    if (cols[c] >= S) return 2;
  v.table = table;
  v.bits = bits;
  v.cols = cols.data();
  v.label_off = d_off;
  v.label_bytes = d_bytes;

  const int rc = stage_check(v, win, pad, argv[2]);
  free(table);
  free(bits);
  free(d_off);
  free(d_bytes);
  return rc;
}
