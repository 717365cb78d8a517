// raw_enrich_render_host -- the raw-key enrichment renderer's lane code (csrc/bc_raw_enrich_render.h) compiled for the
// host, with sanitizers.  TEST-ONLY.
//
//   raw_enrich_render_host IN OUT
//
// IN : u32 G, u32 n_cols, u32 S, u32 merged, u32 win, u32 pad, u32 kind (1 Single, 2 Double), u32 0, u64 n, then per
//      group {u32 raw_len, u32 n_ids} and, for a known group (raw_len 0), n_ids x {u32 len, bytes}; n_cols x u32 column;
//      n x u64 sorted keys T * S + s; n x u32 counts.
// OUT: u64 lines, u64 bytes, then the text of every position for that view.
//
// What the engine does on the device is done here in the plainest way: every sorted pair goes through the header's
// projection (raw_enrich_project), a host sort and a run sum of the harness's own make the segments, and the view's
// text_line_len / text_line_write render them -- every line twice, whole and staged through windows, and both texts
// must agree (stage_check.h).
// Exit status 0: ran; 2: bad arguments; 3: the length predicted and the bytes written differ; 4: the windowed text
// differs from the whole one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_raw_enrich_render.h"
#include "stage_check.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <typename T>
static T* exact(const std::vector<T>& v) {  // a heap block of exactly the vector's size: a read outside it is seen
  T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[8];
  uint64_t n;
  if (!rd(f, head, sizeof head) || !rd(f, &n, 8)) return 2;
  const uint32_t G = head[0], n_cols = head[1], S = head[2], merged = head[3], win = head[4], pad = head[5], kind = head[6];
  if (G == 0 || G > (uint32_t)bc::kRenderMaxG || win == 0 || pad > 3 || S == 0) return 2;
  if (kind != bc::kEnrichSingle && kind != bc::kEnrichDouble) return 2;
  bc::RawEnrichProj proj;
  bc::RawEnrichView v;
  memset(&proj, 0, sizeof proj);
  memset(&v, 0, sizeof v);
  proj.G = v.G = G;
  proj.S = v.S = S;
  v.n_cols = n_cols;
  v.merged = merged;
  v.kind = kind;
  std::vector<uint32_t> off, canon;
  std::string bytes;
  bool shared = false;
  for (uint32_t g = 0; g < G; ++g) {
    uint32_t gh[2];
    if (!rd(f, gh, sizeof gh)) return 2;
    v.raw_len[g] = gh[0];
    v.off_start[g] = (uint32_t)off.size();
    proj.canon_off[g] = (uint32_t)canon.size();
    if (gh[0]) {
      if (gh[0] > 27) return 2;
      v.radix[g] = 1;
      for (uint32_t k = 0; k < gh[0]; ++k) v.radix[g] *= 5;
    } else {
      v.radix[g] = gh[1];
      proj.known[g] = 1;
      std::vector<std::string> ids;
      for (uint32_t i = 0; i < gh[1]; ++i) {
        uint32_t len;
        if (!rd(f, &len, 4)) return 2;
        std::string id(len, '\0');
        if (!rd(f, &id[0], len)) return 2;
        off.push_back((uint32_t)bytes.size());
        bytes += id;
        const uint32_t c = (uint32_t)(std::find(ids.begin(), ids.end(), id) - ids.begin());  // the first entry with this ID
        shared = shared || c != i;
        canon.push_back(c);
        ids.push_back(id);
      }
    }
    proj.radix[g] = v.radix[g];
    off.push_back((uint32_t)bytes.size());
  }
  std::vector<uint32_t> cols(n_cols), cnts(n);
  std::vector<uint64_t> keys(n);
  if (!rd(f, cols.data(), n_cols * 4) || !rd(f, keys.data(), n * 8) || !rd(f, cnts.data(), n * 4)) return 2;
  fclose(f);
  for (uint32_t c = 0; c < n_cols; ++c)
    if (cols[c] >= S) return 2;
  uint32_t* d_canon = exact(canon);
  proj.canon = shared ? d_canon : nullptr;  // (as the engine: no map when no set shares an ID)

  // the segments: per projection the header's key of every pair, a plain sort, a plain run sum
  std::vector<uint64_t> seg_keys, seg_sums, seg_start;
  const uint32_t G_seg = kind == bc::kEnrichDouble && G < 3 ? 0 : G;  // (no Double file below three counted barcodes)
  for (uint32_t g = 0; g < G_seg; ++g)
    for (uint32_t h = kind == bc::kEnrichSingle ? g : g + 1; h < (kind == bc::kEnrichSingle ? g + 1 : G); ++h) {
      proj.g = g;
      proj.h = h;
      const uint64_t bound = bc::raw_enrich_bound(proj);
      std::vector<std::pair<uint64_t, uint32_t>> pk(n);
      for (uint64_t i = 0; i < n; ++i) {
        pk[i] = {bc::raw_enrich_project(proj, keys[i]), cnts[i]};
        if (pk[i].first >= bound) return 3;
      }
      std::stable_sort(pk.begin(), pk.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
      seg_start.push_back(seg_keys.size());
      for (uint64_t i = 0; i < n; ++i) {
        if (i == 0 || pk[i].first != pk[i - 1].first) {
          seg_keys.push_back(pk[i].first);
          seg_sums.push_back(0);
        }
        seg_sums.back() += pk[i].second;
      }
    }
  seg_start.push_back(seg_keys.size());

  uint64_t *d_keys = exact(seg_keys), *d_sums = exact(seg_sums), *d_start = exact(seg_start);
  uint32_t *d_cols = exact(cols), *d_off = exact(off);
  std::vector<uint8_t> pool(bytes.begin(), bytes.end());
  uint8_t* d_bytes = exact(pool);
  v.keys = d_keys;
  v.sums = d_sums;
  v.seg_start = d_start;
  v.n = seg_keys.size();
  v.n_seg = (uint32_t)seg_start.size() - 1;
  v.cols = d_cols;
  v.sample = n_cols ? cols[0] : 0;
  v.label_off = d_off;
  v.label_bytes = d_bytes;

  const int rc = stage_check(v, win, pad, argv[2]);
  free(d_canon);
  free(d_keys);
  free(d_sums);
  free(d_start);
  free(d_cols);
  free(d_off);
  free(d_bytes);
  return rc;
}
