// tests/emu/wide_emu.cpp -- TEST-ONLY: the lane code's wide-key assembly (csrc/bc_lane.h process_read<.., kWide>) on the
// host, next to a plain restatement of the key the wave-per-read kernel builds (csrc/bc_long.h wide_put /
// wide_put_capture / wide_fingerprint) from the read's text.
//
// For every read of the input: the outcome and key of process_read for the plan lowered with allow_wide, and the
// outcome and key of the restatement below, which walks bytes -- the leftmost exact match of the format, else the one
// best window of a repair; every known-set group by exact string, else by the unique nearest reference; the captures
// kept raw and the random barcode byte by byte into the payload, one bit at a time; the fingerprint over the payload
// words.  It uses none of the plane code: no bit planes, no wide_or_bits, no wide_layout.
//
// A program of its own (tests/test_wide_lane_emulation.py builds it with -fsanitize=address,undefined and runs it once
// per scheme); nothing outside tests/ builds or loads this file.
//   wide_emu <in> <out>
//   in:  i32 max_sample, max_barcode, max_constant (-1: the default budget) | u32 scheme bytes, scheme
//        | u32 n_samples, {u32 len, bytes}* | u32 n_sets, {u32 n, {u32 len, bytes}*}* | u32 n_reads, u32 stride
//        | reads (n_reads * stride bytes) | u16 lens[n_reads]
//   out: u32 key_words | per read: u8 outcome, u8 ref outcome, u64 key[8], u64 ref key[8]
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/barcode_count_hip.h"
#include "../../ngs-barcode-count_amd/csrc/bc_lane.h"
#include "../../ngs-barcode-count_amd/csrc/bc_plan.hpp"

namespace {

// the wave-level steps of the lane code, one read at a time (as tests/emu/emu.cpp has them)
struct HostOps {
  const bc::Quad* area = nullptr;
  const bc::Quad* lhash() const { return area; }
  bool tables() const { return area != nullptr; }
  const uint32_t* stage_quality(uint32_t) const { return nullptr; }
  void sequence_consumed() const {}
  void mark(int) const {}
  void issued() const {}
  bool any(bool c) const { return c; }
  uint32_t tier_single_n(const bc::DevGroup& G, uint32_t q1, uint32_t q2, uint32_t qn, bool want, bool& settled) const {
    settled = false;
    return want ? bc::tier_lookup_single_n(G, q1, q2, qn, settled) : bc::kFail;
  }
  uint32_t nearest(const bc::DevGroup& G, uint32_t q1, uint32_t q2, uint32_t qn, uint32_t qx, bool need) const {
    if (!need) return bc::kFail;
    bc::Nearest s;
    bc::nearest_init(s);
    for (uint32_t j = 0; j < G.n_refs; ++j) {
      bool ex;
      const uint32_t d = bc::ref_distance(q1, q2, qn, qx, G.len, G.r1()[j], G.r2()[j], G.rn()[j], G.rlen()[j], ex);
      bc::nearest_add(s, d, j, ex);
    }
    return bc::nearest_result(s.key, s.idx, s.count, G.max_err);
  }
};

struct EmuPlan {
  bc::HostDevPlan h;
  std::vector<std::vector<uint32_t>> dtables;
  std::vector<bc::Quad> lhash;
};

bool emu_open(const bc_plan* p, EmuPlan& E) {
  if (!p->lower(E.h, true)) return false;
  E.dtables.resize(E.h.plan.n_groups);
  E.lhash.resize(E.h.plan.lhash_vec);
  if (!E.lhash.empty()) memcpy(E.lhash.data(), E.h.lhash.data(), E.h.lhash.size() * 4);
  for (uint32_t g = 0; g < E.h.plan.n_groups; ++g) {
    bc::DevGroup& G = E.h.plan.groups[g];
    bc::HostSet& H = E.h.sets[g];
    G.r1_a = (uint64_t)(uintptr_t)H.r1.data();
    G.r2_a = (uint64_t)(uintptr_t)H.r2.data();
    G.rn_a = (uint64_t)(uintptr_t)H.rn.data();
    G.rlen_a = (uint64_t)(uintptr_t)H.rlen.data();
    G.hkeys_a = (uint64_t)(uintptr_t)H.hkeys.data();
    G.hvals_a = (uint64_t)(uintptr_t)H.hvals.data();
    G.tier_off_a = (uint64_t)(uintptr_t)H.tier_off.data();
    G.tier_list_a = (uint64_t)(uintptr_t)H.tier_list.data();
    G.tier_bkt_a = (uint64_t)(uintptr_t)H.tier_bkt.data();
    if (G.mode == bc::kSetDirect) {
      const uint32_t nq = 1u << (2 * G.len);
      E.dtables[g].resize(nq);
      for (uint32_t q = 0; q < nq; ++q) E.dtables[g][q] = bc::dtable_entry(G, q);
      G.dtable_a = (uint64_t)(uintptr_t)E.dtables[g].data();
    }
  }
  return true;
}

template <int NWW>
void lane_read(const EmuPlan& E, const uint8_t* read, uint32_t stride, uint32_t len, uint64_t i, uint8_t& outcome, uint64_t* key) {
  HostOps ops;
  ops.area = E.lhash.empty() ? nullptr : E.lhash.data();
  std::vector<uint32_t> s32((stride + 512) / 4 + 4);
  const bool aligned = (i & 4) != 0;  // (every byte misalignment, and the instantiation that knows there is none)
  const uint32_t base = aligned ? 4u * (uint32_t)(i & 3) : (uint32_t)(i & 3);
  memset(s32.data(), 'A', s32.size() * 4);
  memcpy((uint8_t*)s32.data() + base, read, stride);
  const uint32_t nd = (stride + 3) / 4;
  const bc::ReadResultT<true> r = aligned ? bc::process_read<HostOps, 4, NWW, true, true>(E.h.plan, ops, s32.data(), base, len, len, nd, true)
                                          : bc::process_read<HostOps, 4, NWW, false, true>(E.h.plan, ops, s32.data(), base, len, len, nd, true);
  outcome = (uint8_t)r.outcome;
  for (int w = 0; w < bc::kMaxKeyWords; ++w) key[w] = r.wkey[w];
}

// ---- the restatement: bytes in, key out --------------------------------------------------------------------------
uint64_t ref_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
void ref_set_bit(uint64_t* key, uint32_t at) { key[1u + at / 64u] |= 1ull << (at % 64u); }
bool ref_put_capture(uint64_t* key, uint32_t at, const uint8_t* cap, uint32_t len) {
  bool ok = true;
  for (uint32_t i = 0; i < len; ++i) {
    const uint8_t c = cap[i];
    if (c == 'N') {
      ref_set_bit(key, at + 2u * len + i);
      continue;
    }
    if (c != 'A' && c != 'C' && c != 'G' && c != 'T') ok = false;
    if ((c >> 1) & 1u) ref_set_bit(key, at + i);
    if ((c >> 2) & 1u) ref_set_bit(key, at + len + i);
  }
  return ok;
}

struct RefGroup {
  uint32_t type, off, len, max_err, key_bit;
  const bc::KnownSet* set;
};

uint8_t ref_read(const bc_plan* p, const std::vector<RefGroup>& groups, uint32_t rnd_bit, uint32_t key_words, const uint8_t* seq,
                 uint32_t len, uint64_t* key) {
  for (int w = 0; w < bc::kMaxKeyWords; ++w) key[w] = 0;
  for (uint32_t i = 0; i < len; ++i)
    if (seq[i] >= 0x80u) return (uint8_t)bc::kUnsupported;
  const uint32_t L = p->regex_length;
  auto base_ok = [](uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; };
  auto fmtn_ok = [&](uint32_t o) {
    for (uint32_t q = 0; q < L; ++q)
      if (p->pos[q].kind == bc::kPosFmtN && !base_ok(seq[o + q])) return false;
    return true;
  };
  bool found = false;
  uint32_t start = 0;
  for (uint32_t o = 0; len >= L && o + L <= len && !found; ++o) {
    bool ok = fmtn_ok(o);
    for (uint32_t q = 0; q < L && ok; ++q)
      if (p->pos[q].kind == bc::kPosConst) ok = seq[o + q] == (uint8_t)p->pos[q].letter;
    if (ok) {
      found = true;
      start = o;
    }
  }
  if (!found && len > L && !p->lowercase_constants) {
    uint32_t best = 0xFFFFFFFFu, at = 0, n_best = 0;
    for (uint32_t o = 0; o + L < len; ++o) {  // (the last window is never tested)
      uint32_t mm = 0;
      for (uint32_t q = 0; q < L; ++q)
        if (p->pos[q].kind == bc::kPosConst && seq[o + q] != (uint8_t)p->pos[q].letter && seq[o + q] != 'N') ++mm;
      if (mm < best) {
        best = mm;
        at = o;
        n_best = 1;
      } else if (mm == best) {
        ++n_best;
      }
    }
    if (n_best == 1 && best <= p->max_constant && fmtn_ok(at)) {
      found = true;
      start = at;
    }
  }
  if (!found) return (uint8_t)bc::kConstantRegion;
  bool foreign = false;
  for (const RefGroup& G : groups) {
    const uint8_t* cap = seq + start + G.off;
    if (G.set->size() == 0) {
      if (!ref_put_capture(key, G.key_bit, cap, G.len)) foreign = true;
      continue;
    }
    const std::string text((const char*)cap, G.len);
    uint32_t idx = 0xFFFFFFFFu;
    auto it = G.set->index.find(text);
    if (it != G.set->index.end()) {
      idx = it->second;
    } else {
      uint32_t best = 0xFFFFFFFFu, n_best = 0;
      for (uint32_t j = 0; j < G.set->size(); ++j) {
        const std::string& r = G.set->seqs[j];
        uint32_t d = 0;
        for (size_t k = 0; k < r.size() && k < text.size(); ++k)
          if (r[k] != text[k] && r[k] != 'N' && text[k] != 'N') ++d;
        if (d < best) {
          best = d;
          idx = j;
          n_best = 1;
        } else if (d == best) {
          ++n_best;
        }
      }
      if (n_best != 1 || best > G.max_err) idx = 0xFFFFFFFFu;
    }
    if (idx == 0xFFFFFFFFu) return (uint8_t)(G.type == bc::kGroupSample ? bc::kSampleBarcode : bc::kBarcode);
    for (uint32_t b = 0; b < 32u; ++b)
      if ((idx >> b) & 1u) ref_set_bit(key, G.key_bit + b);
  }
  for (const auto& g : p->groups)
    if (g.type == bc::kGroupRandom && !ref_put_capture(key, rnd_bit, seq + start + g.off, g.len)) foreign = true;
  if (foreign) return (uint8_t)bc::kUnsupported;
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (uint32_t w = 1; w < key_words; ++w) h = ref_mix(h ^ key[w]) + w;
  key[0] = h >> 1;
  return (uint8_t)bc::kMatched;
}

struct Reader {
  FILE* f;
  bool ok = true;
  void raw(void* p, size_t n) { ok = ok && fread(p, 1, n, f) == n; }
  uint32_t u32() {
    uint32_t v = 0;
    raw(&v, 4);
    return v;
  }
  std::string str() {
    const uint32_t n = u32();
    std::string s(ok && n < (1u << 20) ? n : 0, '\0');
    if (!s.empty()) raw(&s[0], s.size());
    return s;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: wide_emu <in> <out>\n");
    return 2;
  }
  Reader in{fopen(argv[1], "rb")};
  if (!in.f) return 2;
  int32_t budgets[3];
  in.raw(budgets, sizeof budgets);
  const std::string scheme = in.str();
  bc_plan* p = bc_plan_create(scheme.data(), scheme.size());
  if (!p) {
    fprintf(stderr, "plan: %s\n", bc_last_error());
    return 1;
  }
  for (uint32_t n = in.u32(), i = 0; i < n && in.ok; ++i) {
    const std::string s = in.str();
    bc_plan_add_sample(p, s.c_str(), s.c_str());
  }
  for (uint32_t sets = in.u32(), b = 0; b < sets && in.ok; ++b)
    for (uint32_t n = in.u32(), i = 0; i < n && in.ok; ++i) {
      const std::string s = in.str();
      bc_plan_add_counted(p, b, s.c_str(), s.c_str());
    }
  bc_plan_set_max_errors(p, budgets[0], budgets[1], budgets[2]);
  const uint32_t n_reads = in.u32(), stride = in.u32();
  if (!in.ok || stride == 0 || stride > 128u || n_reads > (1u << 22)) {
    fprintf(stderr, "bad input (reads of at most 128 bytes)\n");
    return 2;
  }
  std::vector<uint8_t> reads((size_t)n_reads * stride);
  std::vector<uint16_t> lens(n_reads);
  in.raw(reads.data(), reads.size());
  in.raw(lens.data(), lens.size() * 2);
  fclose(in.f);
  if (!in.ok) return 2;

  // the plan without the opt-in must be refused as it always was, with it lowered to a wide lane plan
  {
    bc::HostDevPlan plain;
    if (p->lower(plain)) {
      fprintf(stderr, "the plan is not a wide-key plan\n");
      return 1;
    }
  }
  EmuPlan E;
  if (!emu_open(p, E)) {
    fprintf(stderr, "lower: %s\n", bc_last_error());
    return 1;
  }
  const bc::DevPlan& P = E.h.plan;
  if (!P.wide || !P.sparse || P.defer_search()) {
    fprintf(stderr, "not lowered as a wide plan\n");
    return 1;
  }
  // the layout, restated: the sample group first, then the counted barcodes in order -- 32 bits for a known set, three
  // planes for a capture kept raw -- and the random barcode's planes last
  std::vector<RefGroup> groups;
  uint32_t bits = 0;
  auto add = [&](const bc::FormatGroup& g, const bc::KnownSet* set, uint32_t max_err) {
    groups.push_back({g.type, g.off, g.len, max_err, bits, set});
    bits += set->size() ? 32u : 3u * g.len;
  };
  for (const auto& g : p->groups)
    if (g.type == bc::kGroupSample) add(g, &p->samples, p->max_sample);
  for (uint32_t b = 1; b <= p->barcode_num; ++b)
    for (const auto& g : p->groups)
      if (g.type == bc::kGroupBarcode && g.number == b) add(g, &p->counted[b - 1], p->max_barcode[b - 1]);
  const uint32_t rnd_bit = bits;
  for (const auto& g : p->groups)
    if (g.type == bc::kGroupRandom) bits += 3u * g.len;
  const uint32_t key_words = 1u + (bits + 63u) / 64u;
  if (key_words != P.key_words || key_words > (uint32_t)bc::kMaxKeyWords) {
    fprintf(stderr, "key words: plan %u, restated %u\n", P.key_words, key_words);
    return 1;
  }

  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  fwrite(&key_words, 4, 1, out);
  const uint32_t nww = stride >= P.L ? (stride - P.L + 1 + 31) / 32 : 1;
  for (uint32_t i = 0; i < n_reads; ++i) {
    const uint8_t* rd = &reads[(size_t)i * stride];
    uint8_t oc[2];
    uint64_t key[2][bc::kMaxKeyWords];
    if (nww <= 1)
      lane_read<1>(E, rd, stride, lens[i], i, oc[0], key[0]);
    else if (nww <= 2)
      lane_read<2>(E, rd, stride, lens[i], i, oc[0], key[0]);
    else
      lane_read<4>(E, rd, stride, lens[i], i, oc[0], key[0]);
    oc[1] = ref_read(p, groups, rnd_bit, key_words, rd, lens[i], key[1]);
    fwrite(oc, 1, 2, out);
    fwrite(key, 8, 2 * bc::kMaxKeyWords, out);
  }
  fclose(out);
  bc_plan_destroy(p);
  return 0;
}
