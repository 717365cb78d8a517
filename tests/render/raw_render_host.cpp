// raw_render_host -- the raw-key renderer's lane code (csrc/bc_raw_render.h) compiled for the host, with sanitizers.
// TEST-ONLY.
//
//   raw_render_host IN OUT
//
// IN : u32 G, u32 n_cols, u32 S, u32 merged, u32 win, u32 pad, u64 n, then per group {u32 raw_len, u32 n_ids} and, for a
//      known group (raw_len 0), n_ids x {u32 len, bytes}; n_cols x u32 column; n x u64 sorted keys T * S + s; n x u32 counts.
// OUT: u64 lines, u64 bytes, then the text of the positions 0 .. n-1 for that view.
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

#include "../../ngs-barcode-count_amd/csrc/bc_raw_render.h"
#include "stage_check.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[6];
  uint64_t n;
  if (!rd(f, head, sizeof head) || !rd(f, &n, 8)) return 2;
  const uint32_t G = head[0], n_cols = head[1], S = head[2], merged = head[3], win = head[4], pad = head[5];
  if (G > (uint32_t)bc::kRenderMaxG || win == 0 || pad > 3 || S == 0) return 2;
  bc::RawRenderView v;
  memset(&v, 0, sizeof v);
  v.G = G;
  v.n_cols = n_cols;
  v.S = S;
  v.merged = merged;
  v.n = n;
  std::vector<uint32_t> off;
  std::string bytes;
  for (uint32_t g = 0; g < G; ++g) {
    uint32_t gh[2];
    if (!rd(f, gh, sizeof gh)) return 2;
    v.raw_len[g] = gh[0];
    v.off_start[g] = (uint32_t)off.size();
    if (gh[0]) {
      if (gh[0] > 27) return 2;
      v.radix[g] = 1;
      for (uint32_t k = 0; k < gh[0]; ++k) v.radix[g] *= 5;
    } else {
      v.radix[g] = gh[1];
      for (uint32_t i = 0; i < gh[1]; ++i) {
        uint32_t len;
        if (!rd(f, &len, 4)) return 2;
        std::string id(len, '\0');
        if (!rd(f, &id[0], len)) return 2;
        off.push_back((uint32_t)bytes.size());
        bytes += id;
      }
    }
    off.push_back((uint32_t)bytes.size());
  }
  // (heap blocks of exactly their own size, so a read outside the keys, the counts, the offsets or the IDs is seen)
  uint32_t* cols = (uint32_t*)malloc(n_cols ? n_cols * 4 : 1);
  if (!rd(f, cols, n_cols * 4)) return 2;
  uint64_t* keys = (uint64_t*)malloc(n ? n * 8 : 1);
  uint32_t* cnts = (uint32_t*)malloc(n ? n * 4 : 1);
  if (!rd(f, keys, n * 8) || !rd(f, cnts, n * 4)) return 2;
  fclose(f);
  uint32_t* d_off = (uint32_t*)malloc(off.size() * 4);
  memcpy(d_off, off.data(), off.size() * 4);
  uint8_t* d_bytes = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
  memcpy(d_bytes, bytes.data(), bytes.size());
  for (uint32_t c = 0; c < n_cols; ++c)
    if (cols[c] >= S) return 2;
  v.keys = keys;
  v.cnts = cnts;
  v.cols = cols;
  v.sample = n_cols ? cols[0] : 0;
  v.label_off = d_off;
  v.label_bytes = d_bytes;

  const int rc = stage_check(v, win, pad, argv[2]);
  free(cols);
  free(keys);
  free(cnts);
  free(d_off);
  free(d_bytes);
  return rc;
}
