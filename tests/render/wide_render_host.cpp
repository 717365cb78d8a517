// wide_render_host -- the wide-key renderer's lane code (csrc/bc_wide_render.h) compiled for the host, with sanitizers.
// TEST-ONLY.
//
//   wide_render_host IN OUT ORDER
//
// IN : u32 G, u32 n_cols, u32 S, u32 merged, u32 win, u32 pad, u32 W, u32 has_sample, u64 n, then per group
//      {u32 raw_len, u32 n_ids, u32 key_bit} and, for a known group (raw_len 0), n_ids x {u32 len, bytes}; n_cols x u32
//      column; n keys of W u64 (word 0: anything; words 1 .. W-1: the payload) in ANY order; n x u32 counts.
// Step 1: every key's order key, word by word (bc::wide_order_word), written to ORDER: u32 K, u32 0, n x K u64 (word 0,
//      the least significant, first), in the order of IN.
// Step 2: the keys sorted by their order keys and gathered, as the device does; the view over them through
//      stage_check.h: every line written twice, whole and staged through windows, and both texts must agree.
// OUT: u64 lines, u64 bytes, then the text of the positions 0 .. n-1 for that view.
// Exit status 0: ran; 2: bad arguments; 3: the length predicted and the bytes written differ; 4: the windowed text
// differs from the whole one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_wide_render.h"
#include "stage_check.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[8];
  uint64_t n;
  if (!rd(f, head, sizeof head) || !rd(f, &n, 8)) return 2;
  const uint32_t G = head[0], n_cols = head[1], S = head[2], merged = head[3], win = head[4], pad = head[5], W = head[6],
                 has_sample = head[7];
  if (G > (uint32_t)bc::kRenderMaxG || win == 0 || pad > 3 || S == 0 || W < 2 || W > 8 || (!has_sample && S != 1)) return 2;
  bc::WideRenderView v;
  bc::WideOrder o;
  memset(&v, 0, sizeof v);
  memset(&o, 0, sizeof o);
  v.G = o.G = G;
  v.W = o.W = W;
  v.n_cols = n_cols;
  v.S = S;
  v.merged = merged;
  v.n = n;
  v.sample_bits = o.sample_bits = has_sample ? 32u : 0u;
  o.sample_obits = has_sample ? bc::wide_bit_length(S - 1u) : 0u;
  std::vector<uint32_t> off;
  std::string bytes;
  for (uint32_t g = 0; g < G; ++g) {
    uint32_t gh[3];
    if (!rd(f, gh, sizeof gh)) return 2;
    v.raw_len[g] = o.raw_len[g] = gh[0];
    v.key_bit[g] = o.key_bit[g] = gh[2];
    v.off_start[g] = (uint32_t)off.size();
    if (gh[2] + (gh[0] ? 3u * gh[0] : 32u) > 64u * (W - 1u)) return 2;
    if (!gh[0]) {
      v.n_ids[g] = gh[1];
      o.obits[g] = gh[1] ? bc::wide_bit_length(gh[1] - 1u) : 0u;
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
  bc::wide_order_layout(o);
  // (heap blocks of exactly their own size, so a read outside the keys, the counts, the offsets or the IDs is seen)
  uint32_t* cols = (uint32_t*)malloc(n_cols ? n_cols * 4 : 1);
  if (!rd(f, cols, n_cols * 4)) return 2;
  uint64_t* keys_in = (uint64_t*)malloc(n ? n * W * 8 : 1);
  uint32_t* cnts_in = (uint32_t*)malloc(n ? n * 4 : 1);
  if (!rd(f, keys_in, n * W * 8) || !rd(f, cnts_in, n * 4)) return 2;
  fclose(f);
  for (uint32_t c = 0; c < n_cols; ++c)
    if (cols[c] >= S) return 2;

  // step 1: the order keys, column by column as the device lays them out
  uint64_t* okeys = (uint64_t*)malloc(n ? n * o.K * 8 : 1);
  for (uint32_t w = 0; w < o.K; ++w)
    for (uint64_t i = 0; i < n; ++i) okeys[(uint64_t)w * n + i] = bc::wide_order_word(o, keys_in + i * W + 1u, w);
  {
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) return 2;
    const uint32_t oh[2] = {o.K, 0};
    fwrite(oh, 4, 2, fo);
    for (uint64_t i = 0; i < n; ++i)
      for (uint32_t w = 0; w < o.K; ++w) fwrite(&okeys[(uint64_t)w * n + i], 8, 1, fo);
    fclose(fo);
  }
  // step 2: sorted by order key (word K-1 the most significant), gathered, rendered
  std::vector<uint64_t> perm(n);
  for (uint64_t i = 0; i < n; ++i) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) {
    for (uint32_t w = o.K; w-- > 0;)
      if (okeys[(uint64_t)w * n + a] != okeys[(uint64_t)w * n + b]) return okeys[(uint64_t)w * n + a] < okeys[(uint64_t)w * n + b];
    return false;
  });
  uint64_t* keys = (uint64_t*)malloc(n ? n * W * 8 : 1);
  uint32_t* cnts = (uint32_t*)malloc(n ? n * 4 : 1);
  for (uint64_t j = 0; j < n; ++j) {
    memcpy(keys + j * W, keys_in + perm[j] * W, W * 8);
    cnts[j] = cnts_in[perm[j]];
  }
  uint32_t* d_off = (uint32_t*)malloc(off.size() * 4);
  memcpy(d_off, off.data(), off.size() * 4);
  uint8_t* d_bytes = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
  memcpy(d_bytes, bytes.data(), bytes.size());
  v.keys = keys;
  v.cnts = cnts;
  v.cols = cols;
  v.sample = n_cols ? cols[0] : 0;
  v.label_off = d_off;
  v.label_bytes = d_bytes;

  const int rc = stage_check(v, win, pad, argv[2]);
  free(cols);
  free(keys_in);
  free(cnts_in);
  free(okeys);
  free(keys);
  free(cnts);
  free(d_off);
  free(d_bytes);
  return rc;
}
