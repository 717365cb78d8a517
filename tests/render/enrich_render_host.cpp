// enrich_render_host -- the enrichment renderer's lane code (csrc/bc_enrich_render.h) compiled for the host, with
// sanitizers.  TEST-ONLY.
//
//   enrich_render_host IN OUT
//
// IN : u32 G, u32 kind, u32 n_cols, u32 S, u32 win, u32 pad, u32 has_canon, u32 0, then G x u32 N_g, n_cols x u32 column,
//      per group N_g x {u32 len, bytes}, with has_canon SUM x u32 canon, and S * K x u64 raw sums (K = SUM or P).
// OUT: u64 lines, u64 bytes, then the text of the keys 0 .. K-1 for those columns.
//
// With has_canon the sums are folded first, key by key, through enrich_fold_target.  Then every line is written twice,
// whole and staged through windows, and both texts must agree (stage_check.h).
// Exit status 0: ran; 2: bad arguments; 3: the length predicted and the bytes written differ; 4: the windowed text
// differs from the whole one; 5: a key does not decode to itself.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_enrich_render.h"
#include "stage_check.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[8];
  if (!rd(f, head, sizeof head)) return 2;
  const uint32_t G = head[0], kind = head[1], n_cols = head[2], S = head[3], win = head[4], pad = head[5], has_canon = head[6];
  if (G == 0 || G > (uint32_t)bc::kRenderMaxG || win == 0 || pad > 3) return 2;
  if (kind != bc::kEnrichSingle && kind != bc::kEnrichDouble) return 2;
  bc::EnrichRenderView v;
  memset(&v, 0, sizeof v);
  v.G = G;
  v.kind = kind;
  v.n_cols = n_cols;
  if (!rd(f, v.n, G * 4)) return 2;
  uint64_t sum_n = 0, pairs = 0;
  for (uint32_t g = 0; g < G; ++g) sum_n += v.n[g];
  if (G >= 3)
    for (uint32_t g = 0; g + 1 < G; ++g)
      for (uint32_t h = g + 1; h < G; ++h) pairs += (uint64_t)v.n[g] * v.n[h];
  v.K = kind == bc::kEnrichSingle ? sum_n : pairs;
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
  // (heap blocks of exactly their own size, so a read outside the sums, the map, the offsets or the IDs is seen)
  uint32_t* canon = nullptr;
  if (has_canon) {
    canon = (uint32_t*)malloc(sum_n ? sum_n * 4 : 1);
    if (!rd(f, canon, sum_n * 4)) return 2;
  }
  const uint64_t entries = (uint64_t)S * v.K;
  unsigned long long* sums = (unsigned long long*)malloc(entries ? entries * 8 : 1);
  if (!rd(f, sums, entries * 8)) return 2;
  fclose(f);
  uint32_t* d_off = (uint32_t*)malloc(off.size() * 4 + 1);
  memcpy(d_off, off.data(), off.size() * 4);
  uint8_t* d_bytes = (uint8_t*)malloc(bytes.size() + 1);
  memcpy(d_bytes, bytes.data(), bytes.size());
  for (uint32_t c = 0; c < n_cols; ++c)
    if (cols[c] >= S) return 2;
  v.sums = sums;
  v.canon = canon;
  v.cols = cols.data();
  v.label_off = d_off;
  v.label_bytes = d_bytes;

  // every key decodes to fields and indices that give the key back
  for (uint64_t k = 0; k < v.K; ++k) {
    const bc::EnrichKey key = bc::enrich_key(v, k);
    if (key.g >= G || key.h >= G || key.i >= v.n[key.g] || key.j >= v.n[key.h]) return 5;
    uint64_t back = 0;
    if (kind == bc::kEnrichSingle) {
      back = bc::enrich_set_off(v, key.g) + key.i;
    } else {
      if (key.g >= key.h) return 5;
      for (uint32_t g = 0; g + 1 < G; ++g)
        for (uint32_t h = g + 1; h < G; ++h)
          if (g < key.g || (g == key.g && h < key.h)) back += (uint64_t)v.n[g] * v.n[h];
      back += (uint64_t)key.i * v.n[key.h] + key.j;
    }
    if (back != k) return 5;
  }
  // the fold, as the device does it: a key that is not its own target hands its sum over and becomes zero
  if (canon)
    for (uint64_t s = 0; s < S; ++s)
      for (uint64_t k = 0; k < v.K; ++k) {
        const uint64_t t = bc::enrich_fold_target(v, k);
        if (t >= v.K || t > k) return 5;
        if (t == k) continue;
        sums[s * v.K + t] += sums[s * v.K + k];
        sums[s * v.K + k] = 0;
      }

  const int rc = stage_check(v, win, pad, argv[2]);
  free(sums);
  free(canon);
  free(d_off);
  free(d_bytes);
  return rc;
}
