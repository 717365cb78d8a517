// bam_host -- the BAM record framing (csrc/bc_bam.h) on the host, in plain loops, compiled with sanitizers.  TEST-ONLY.
//
//   bam_host IN OUT
//
// IN holds cases one after the other: u64 len, u64 start, u32 n_ref, u32 capacity, then len bytes of text.  The text is
// handed to the code under test in a heap block of exactly its size, so AddressSanitizer sees any access outside it.
// OUT gets, per case, a line "status n_records n_candidates end_pos" and a line "at l_seq flag" per record: what
// bc_bam_frame_device reports for the same text.  When the case asks for it (capacity's top bit), every record's line is
// followed by a "sequence ..." and a "quality ..." line: the read as the gather kernel unpacks it.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_bam.h"

using namespace bc;

static void frame(const uint8_t* text, uint64_t len, uint64_t start, uint32_t n_ref, uint32_t capacity, bool unpack, FILE* out) {
  std::vector<uint32_t> cand;
  bool over = false;
  for (uint64_t p = start; len >= kBamFixed && p <= len - kBamFixed && !over; ++p)
    if (bam_candidate_at(text, len, p, n_ref) == 1u) {
      if (cand.size() == capacity) over = true;
      else cand.push_back((uint32_t)p);
    }
  if (over) {
    fprintf(out, "%u 0 0 %llu\n", kBamCapacity, (unsigned long long)start);
    return;
  }
  const uint32_t n = (uint32_t)cand.size();
  uint32_t levels = 1;
  while (bam_level_used(levels, n)) ++levels;
  std::vector<std::vector<uint32_t>> jump(levels, std::vector<uint32_t>(n));
  std::vector<uint32_t> link(n), mark(n, 0);
  for (uint32_t i = 0; i < n; ++i) jump[0][i] = bam_successor(text, len, cand.data(), n, i, n_ref, &link[i]);
  for (uint32_t k = 1; k < levels; ++k)
    for (uint32_t i = 0; i < n; ++i) jump[k][i] = bam_jump_step(jump[k - 1].data(), i);
  uint32_t status = kBamOk;
  uint64_t end_pos = start;
  if (bam_chain_start(text, len, start, cand.data(), n, n_ref, &status)) mark[0] = 1;
  for (uint32_t k = levels; k-- > 0;)
    for (uint32_t i = 0; i < n; ++i)
      if (mark[i]) mark[jump[k][i]] = 1;
  std::vector<uint32_t> recs;
  for (uint32_t i = 0; i < n; ++i) {
    if (!mark[i]) continue;
    if (link[i] != kLinkPartial) recs.push_back(cand[i]);
    if (link[i] != kLinkNext) {
      uint32_t how;
      end_pos = bam_chain_end(text, cand[i], link[i], &how);
      if (how != kBamOk) status = how;
    }
  }
  fprintf(out, "%u %zu %u %llu\n", status, recs.size(), n, (unsigned long long)end_pos);
  for (uint32_t p : recs) {
    const uint32_t l_name = text[p + 12], n_cigar = (uint32_t)text[p + 16] | ((uint32_t)text[p + 17] << 8);
    const uint32_t flag = (uint32_t)text[p + 18] | ((uint32_t)text[p + 19] << 8), l_seq = bam_u32(text + p + 20);
    fprintf(out, "%u %u %u\n", p, l_seq, flag);
    if (!unpack) continue;
    const uint8_t* seq = text + p + kBamFixed + l_name + 4u * n_cigar;
    const uint8_t* qual = seq + (l_seq + 1u) / 2u;
    const bool rev = (flag & 0x10u) != 0, none = l_seq && qual[0] == 0xFFu;
    std::string s, q;
    for (uint32_t i = 0; i < l_seq; ++i) {
      const uint32_t j = rev ? l_seq - 1u - i : i;
      s += (char)bam_base_ascii((j & 1u) ? (seq[j >> 1] & 15u) : (seq[j >> 1] >> 4), rev);
      q += (char)bam_qual_ascii(qual[j], none);
    }
    fprintf(out, "sequence %s\nquality %s\n", s.c_str(), q.c_str());
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 2;
  for (;;) {
    uint64_t head[2];
    uint32_t tail[2];
    if (!in.read((char*)head, sizeof head)) break;
    if (!in.read((char*)tail, sizeof tail)) return 2;
    uint8_t* text = new uint8_t[head[0]];
    if (head[0] && !in.read((char*)text, (std::streamsize)head[0])) return 2;
    frame(text, head[0], head[1], tail[0], tail[1] & 0x7FFFFFFFu, (tail[1] >> 31) != 0, out);
    delete[] text;
  }
  fclose(out);
  return 0;
}
