// bc_bam.h -- framing of BAM records, the per-element logic: one function per candidate, per jump pointer, per mark.
// The kernels of bc_bam_kernels.h call these with one thread per element; tests/bam/bam_host.cpp compiles the same
// functions with g++ (through bc_intrin.h) and calls them in plain loops, under sanitizers.
//
// A BAM record is `block_size` (4 bytes) and block_size bytes behind it; where a record starts is known only from the
// record before.  The framing of a text T[0, len) whose first record starts at `start`:
//
//   candidates   every offset p in [start, len - 36] whose fixed 36 bytes pass bam_header_check (necessary conditions
//                only: a filter that never rejects a real record), in order of p
//   successor    of candidate i: the candidate at p + 4 + block_size (binary search), or how the chain ends there
//                (BamLink); level 0 of the jump pointers, a chain end pointing at itself
//   jump         level k holds every candidate's 2^k-th successor: jump[k][i] = jump[k-1][jump[k-1][i]]
//   marks        the candidate at `start` is marked; from the highest level down every marked candidate marks its
//                2^k-th successor.  After level 0 exactly the chain from `start` is marked: a mark is only ever put on
//                a candidate reached from `start`, and a candidate d links down the chain is reached through the set
//                bits of d, highest first.  Decoys (headers that only look like one, inside names or aux data) are
//                candidates but stay unmarked, also where their own chain runs into the true one.
//
// Correctness comes from the chain alone.
#pragma once
#include "bc_intrin.h"

namespace bc {

constexpr uint32_t kBamFixed = 36;              // block_size and the 32 fixed bytes behind it
constexpr uint32_t kBamMaxRecord = 4u << 20;    // a record, its length prefix included, fits the ingest's overlap

// what bc_bam_frame_device reports (BC_BAM_* of the header)
constexpr uint32_t kBamOk = 0, kBamBroken = 1, kBamCapacity = 2, kBamTooLong = 3;

// how the chain goes on behind a candidate
enum BamLink : uint32_t {
  kLinkNext = 0,      // its successor is a candidate: jump[0] holds it
  kLinkEnd = 1,       // whole record; fewer than 36 bytes of text follow it
  kLinkBroken = 2,    // whole record; what follows is no record header
  kLinkTooLong = 3,   // whole record; what follows is a header but for its length above kBamMaxRecord
  kLinkPartial = 4,   // the record ends beyond the text: the next chunk frames it
};

// "=ACMGRSVTWYHKDBN" and the same string for the complement: in BAM's code (A=1, C=2, G=4, T=8 and their unions) the
// complement of a base is its four bits in reverse order
// (eight characters to a word, the first in the lowest byte: "=ACMGRSV" "TWYHKDBN" and "=TGKCYSB" "AWRDMHVN")
constexpr uint64_t kBamAsciiLo = 0x565352474D43413DULL, kBamAsciiHi = 0x4E42444B48595754ULL;
constexpr uint64_t kBamCompLo = 0x425359434B47543DULL, kBamCompHi = 0x4E56484D44525741ULL;

BC_HD uint32_t bam_base_ascii(uint32_t nibble, bool complement) {
  const uint64_t lo = complement ? kBamCompLo : kBamAsciiLo, hi = complement ? kBamCompHi : kBamAsciiHi;
  return (uint32_t)(((nibble & 8u) ? hi : lo) >> (8u * (nibble & 7u))) & 0xFFu;
}
// Phred byte -> FASTQ character; `none`: the record stores no qualities (its first quality byte is 0xFF)
BC_HD uint32_t bam_qual_ascii(uint32_t q, bool none) { return none ? (uint32_t)'"' : (q > 93u ? 93u : q) + 33u; }

BC_HD uint32_t bam_u32(const uint8_t* t) {
  return (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
}

// fields of the fixed part, from its nine little-endian words
BC_HD uint32_t bam_block_size(const uint32_t* w) { return w[0]; }
BC_HD uint32_t bam_l_read_name(const uint32_t* w) { return w[3] & 0xFFu; }
BC_HD uint32_t bam_n_cigar(const uint32_t* w) { return w[4] & 0xFFFFu; }
BC_HD uint32_t bam_flag(const uint32_t* w) { return w[4] >> 16; }
BC_HD uint32_t bam_l_seq(const uint32_t* w) { return w[5]; }

// The necessary conditions on a record's fixed 36 bytes: 0 no record starts like this, 1 one may, 2 one may but it is
// longer than kBamMaxRecord.  (The name's closing NUL is bam_name_ok's.)
BC_HD uint32_t bam_header_check(const uint32_t* w, uint32_t n_ref) {
  const uint32_t block_size = w[0], l_name = bam_l_read_name(w);
  const uint64_t l_seq = w[5];
  const int32_t ref_id = (int32_t)w[1], pos = (int32_t)w[2], next_ref = (int32_t)w[6], next_pos = (int32_t)w[7];
  if (l_name < 1u) return 0;
  if (ref_id < -1 || next_ref < -1 || pos < -1 || next_pos < -1) return 0;
  if (ref_id >= 0 && (uint32_t)ref_id >= n_ref) return 0;
  if (next_ref >= 0 && (uint32_t)next_ref >= n_ref) return 0;
  if ((block_size >> 31) != 0u) return 0;  // (block_size is an int32 in the format)
  const uint64_t least = 32ull + l_name + 4ull * bam_n_cigar(w) + (l_seq + 1ull) / 2ull + l_seq;
  if (least > block_size) return 0;
  return 4ull + block_size <= kBamMaxRecord ? 1u : 2u;
}
// the read name ends with a NUL, where the text still holds that byte
BC_HD bool bam_name_ok(const uint8_t* text, uint64_t len, uint64_t p, uint32_t l_name) {
  const uint64_t at = p + kBamFixed + l_name - 1u;
  return at >= len || text[at] == 0;
}

// bam_header_check + bam_name_ok at offset p of the text, for any p (0 where fewer than 36 bytes are left)
BC_HD uint32_t bam_candidate_at(const uint8_t* text, uint64_t len, uint64_t p, uint32_t n_ref) {
  if (p > len || len - p < kBamFixed) return 0;
  uint32_t w[9];
  for (uint32_t k = 0; k < 9; ++k) w[k] = bam_u32(text + p + 4u * k);
  const uint32_t c = bam_header_check(w, n_ref);
  return c && bam_name_ok(text, len, p, bam_l_read_name(w)) ? c : 0u;
}

// index of offset `at` among the sorted candidate offsets, or n when it is not one of them
BC_HD uint32_t bam_find(const uint32_t* cand, uint32_t n, uint64_t at) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (cand[mid] < at) lo = mid + 1u; else hi = mid;
  }
  return lo < n && cand[lo] == at ? lo : n;
}

// Candidate i: how the chain goes on behind it (*link) and level 0 of its jump pointers (the return value).
BC_HD uint32_t bam_successor(const uint8_t* text, uint64_t len, const uint32_t* cand, uint32_t n, uint32_t i, uint32_t n_ref,
                             uint32_t* link) {
  const uint64_t p = cand[i];
  const uint64_t next = p + 4ull + bam_u32(text + p);
  if (next > len) {
    *link = kLinkPartial;
    return i;
  }
  if (len - next < kBamFixed) {
    *link = kLinkEnd;
    return i;
  }
  const uint32_t j = bam_find(cand, n, next);
  if (j < n) {
    *link = kLinkNext;
    return j;
  }
  *link = bam_candidate_at(text, len, next, n_ref) == 2u ? kLinkTooLong : kLinkBroken;
  return i;
}

// The chain's first link.  True: candidate 0 is the record at `start` and gets the first mark; false: there is none,
// and *status says whether that is an error (a header's worth of text at `start` that is no record header) or just
// the end of the text.
BC_HD bool bam_chain_start(const uint8_t* text, uint64_t len, uint64_t start, const uint32_t* cand, uint32_t n, uint32_t n_ref,
                           uint32_t* status) {
  *status = kBamOk;
  if (start > len || len - start < kBamFixed) return false;
  if (n && cand[0] == start) return true;
  *status = bam_candidate_at(text, len, start, n_ref) == 2u ? kBamTooLong : kBamBroken;
  return false;
}
// The marked candidate at offset p whose link is not kLinkNext ends the chain: where (the return value: just past the
// last whole record) and with what status.
BC_HD uint64_t bam_chain_end(const uint8_t* text, uint64_t p, uint32_t link, uint32_t* status) {
  *status = link == kLinkBroken ? kBamBroken : link == kLinkTooLong ? kBamTooLong : kBamOk;
  return link == kLinkPartial ? p : p + 4ull + bam_u32(text + p);
}

// level k of the jump pointers is needed (and built) for n candidates: a chain has at most n - 1 links
BC_HD bool bam_level_used(uint32_t k, uint32_t n) { return k == 0u || (k < 32u && (1u << k) < n); }
// element i of a level from the level below
BC_HD uint32_t bam_jump_step(const uint32_t* below, uint32_t i) { return below[below[i]]; }

}  // namespace bc
