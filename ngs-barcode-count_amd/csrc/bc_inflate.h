// bc_inflate.h -- RFC 1951 inflate of ONE gzip member (a BGZF block) by ONE wavefront.
//
// Written like bc_lane.h: the same text compiles for the device (bc_inflate.hip: one wave per block) and for the host
// (tests/inflate/inflate_host.cpp, with sanitizers), so every input a GPU test uses has gone through this code on a CPU
// first.  The shape of the work:
//
//   * Symbol decoding is a serial chain, so it is done wave-UNIFORMLY: every lane holds the same bit buffer and walks
//     the same symbols (LDS reads at one address are a broadcast).  Nothing has to be handed from a "decoder lane" to
//     the others.
//   * Everything with width is spread over the 64 lanes: the refill window (256 payload bytes per load), the table
//     construction, the copy of a match or a stored block, and the CRC.
//   * The member's output lives in global memory only; a back-reference reads it from there (at most 64 KiB per member:
//     cache resident).  Memory operations of one wave reach the cache in program order, so a wave-scope fence (no
//     instruction, a compiler barrier) is all that stands between a store and the loads of a later copy.
//
// Bounds: every payload byte is read by the refill window or the stored copy, which check against src_len (bytes past
// the end read as zero and are caught by the consumed-bits check); every store and back-reference is checked against
// [0, isize).  A violation ends the member with a status.  Every loop is bounded by bits consumed or bytes produced.
#pragma once
#include "bc_intrin.h"

namespace bc {

// per-member result (bc_bgzf_inflate_device's status words)
enum : uint32_t {
  kInfOk = 0,
  kInfBadBlockType = 1,    // BTYPE 3, or a stored block whose LEN / NLEN disagree
  kInfBadCodeLengths = 2,  // over-subscribed or incomplete Huffman code, bad repeat, too many symbols, no end-of-block
  kInfBadSymbol = 3,       // a code that no symbol has, a reserved symbol, or a distance before the member's start
  kInfInputOverrun = 4,    // the deflate stream goes past the payload
  kInfOutputOverrun = 5,   // the deflate stream makes more than ISIZE bytes
  kInfIsizeMismatch = 6,   // the deflate stream ends before ISIZE bytes
  kInfCrcMismatch = 7,
};

constexpr uint32_t kInfLitBits = 10, kInfDistBits = 8, kInfClBits = 7;
constexpr uint32_t kInfWindow = 256;  // payload bytes per refill load (4 per lane)

// one wave's working set (LDS on the device): 4,416 bytes
struct InflateTables {
  uint16_t lit[1u << kInfLitBits];    // primary tables: (symbol << 4) | code length; 0 = a longer code (or none)
  uint16_t dist[1u << kInfDistBits];  // (doubles as the code-length code's table while a dynamic header is read)
  uint16_t lsym[288];                 // symbols sorted by code length (canonical order), for codes beyond the primary bits
  uint16_t dsym[32];
  uint16_t lcount[16], dcount[16];    // symbols per code length
  uint16_t offs[16];
  uint8_t lens[352];                  // [0, 320): literal/length then distance code lengths; [320, 339): code-length code
  uint32_t win[kInfWindow / 4];       // refill window
  uint32_t red[64];                   // CRC terms of the lanes
};

#if defined(__HIP_DEVICE_COMPILE__)
// the body runs once, on every lane at once
#define BC_INF_LANES(lane) for (uint32_t lane = self_lane, _once = 1; _once; _once = 0)
#define BC_INF_WAVE_SYNC() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront")
#else
// the host walks the lanes one after the other; bodies never read what another lane writes in the same body
#define BC_INF_LANES(lane) for (uint32_t lane = 0; lane < 64; ++lane)
#define BC_INF_WAVE_SYNC() (void)0
#endif

BC_HD uint32_t crc32_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  return c;
}

// a * b mod P over GF(2), reflected representation (bit 31 is x^0), as zlib's multmodp but with a fixed trip count
BC_HD uint32_t crc32_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
  }
  return p;
}
// x^(8 n) mod P
BC_HD uint32_t crc32_x8n(uint32_t n) {
  uint32_t r = 0x80000000u, b = 0x00800000u;
  for (int i = 0; i < 32 && n; ++i, n >>= 1) {
    if (n & 1u) r = crc32_mulmod(r, b);
    b = crc32_mulmod(b, b);
  }
  return r;
}

struct InflateBits {
  uint64_t buf = 0;
  uint32_t cnt = 0;       // valid bits in buf
  uint32_t in_pos = 0;    // payload bytes taken into buf so far
  uint32_t win_base = 0;  // payload offset of win[0]; in_pos - win_base >= kInfWindow: the window has to be loaded
};

// Builds the decoding tables of one canonical Huffman code.  Returns the code space left over (0: complete code,
// < 0: over-subscribed, > 0: incomplete), as puff.c's construct().
BC_HD int inflate_build(const uint8_t* lens, uint32_t n, uint16_t* tab, uint32_t tab_bits, uint16_t* count, uint16_t* symbol,
                        uint16_t* offs, uint32_t self_lane) {
  (void)self_lane;
  BC_INF_WAVE_SYNC();
  BC_INF_LANES(lane) {
    if (lane < 16u) {
      uint32_t c = 0;
      for (uint32_t s = 0; s < n; ++s) c += lens[s] == lane;
      count[lane] = (uint16_t)c;
    }
  }
  BC_INF_WAVE_SYNC();
  int left = 1;
  uint32_t off = 0;
  for (uint32_t l = 1; l <= 15; ++l) {
    left = (left << 1) - (int)count[l];
    if (left < 0) return left;
    offs[l] = (uint16_t)off;  // (every lane writes the same value)
    off += count[l];
  }
  BC_INF_WAVE_SYNC();
  BC_INF_LANES(lane) {
    if (lane >= 1u && lane < 16u) {
      uint32_t at = offs[lane];
      for (uint32_t s = 0; s < n; ++s)
        if (lens[s] == lane) symbol[at++] = (uint16_t)s;
    }
  }
  BC_INF_WAVE_SYNC();
  // every primary entry decodes its own index bit by bit (canonical decoding, first bit of the code in bit 0)
  for (uint32_t base = 0; base < (1u << tab_bits); base += 64u) {
    BC_INF_LANES(lane) {
      const uint32_t e = base + lane;
      int code = 0, first = 0, index = 0;
      uint32_t ent = 0;
      for (uint32_t l = 1; l <= tab_bits; ++l) {
        code |= (int)((e >> (l - 1)) & 1u);
        const int cnt = (int)count[l];
        if (code - cnt < first) {
          ent = ((uint32_t)symbol[index + (code - first)] << 4) | l;
          break;
        }
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
      }
      if (e < (1u << tab_bits)) tab[e] = (uint16_t)ent;
    }
  }
  BC_INF_WAVE_SYNC();
  return left;
}

// one symbol off the low bits of `buf` (at least 15 valid or zero-padded bits): the symbol, or -1 when no symbol has
// that code; *len = bits to drop
BC_HD int inflate_symbol(uint64_t buf, const uint16_t* tab, uint32_t tab_bits, const uint16_t* count, const uint16_t* symbol,
                         uint32_t* len) {
  const uint32_t ent = tab[(uint32_t)buf & ((1u << tab_bits) - 1u)];
  if (ent) {
    *len = ent & 15u;
    return (int)(ent >> 4);
  }
  int code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l <= 15; ++l) {
    code |= (int)((buf >> (l - 1)) & 1u);
    const int cnt = (int)count[l];
    if (code - cnt < first) {
      *len = l;
      return (int)symbol[index + (code - first)];
    }
    index += cnt;
    first += cnt;
    first <<= 1;
    code <<= 1;
  }
  *len = 15;
  return -1;
}

// ---- the pieces inflate_member and the span inflater (bc_gunzip.h) share: the bit reader and the block header ----

// at least 32 valid bits afterwards (zero bits past the payload's end): the most one step takes is a distance code with
// its extra bits, 28
BC_HD void inflate_refill(InflateBits& r, const BC_GLOBAL uint8_t* src, uint32_t src_len, InflateTables& T, uint32_t self_lane) {
  (void)self_lane;
  if (r.cnt <= 32u) {
    if (r.in_pos - r.win_base >= kInfWindow) {
      BC_INF_WAVE_SYNC();
      BC_INF_LANES(lane) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4u; ++k) {
          const uint32_t at = r.in_pos + 4u * lane + k;
          if (at < src_len) w |= (uint32_t)src[at] << (8u * k);
        }
        T.win[lane] = w;
      }
      BC_INF_WAVE_SYNC();
      r.win_base = r.in_pos;
    }
    r.buf |= (uint64_t)T.win[(r.in_pos - r.win_base) >> 2] << r.cnt;
    r.cnt += 32u;
    r.in_pos += 4u;
  }
}
BC_HD void inflate_drop(InflateBits& r, uint32_t n) {
  r.buf >>= n;
  r.cnt -= n;
}
// payload bytes of which at least one bit has been consumed > src_len
BC_HD bool inflate_overrun(const InflateBits& r, uint32_t src_len) { return r.in_pos - (r.cnt >> 3) > src_len; }

// The code of a block of type 1 (fixed) or 2 (dynamic: its header is read off `r`): the code lengths, both decoding
// tables and the checks zlib applies to them.  kInfOk, or the status the block ends the stream with.
BC_HD uint32_t inflate_block_tables(InflateBits& r, const BC_GLOBAL uint8_t* src, uint32_t src_len, uint32_t type, InflateTables& T,
                                    uint32_t self_lane) {
#define BC_INF_REFILL() inflate_refill(r, src, src_len, T, self_lane)
#define BC_INF_DROP(n) inflate_drop(r, (n))
#define BC_INF_OVERRUN() inflate_overrun(r, src_len)
  uint32_t n_lit = 288, n_dist = 32;
  if (type == 1u) {
    for (uint32_t base = 0; base < 320u; base += 64u) {
      BC_INF_LANES(lane) {
        const uint32_t s = base + lane;
        T.lens[s] = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : s < 288u ? 8u : 5u);
      }
    }
  } else {
    BC_INF_REFILL();
    n_lit = ((uint32_t)r.buf & 31u) + 257u;
    n_dist = (((uint32_t)r.buf >> 5) & 31u) + 1u;
    const uint32_t n_cl = (((uint32_t)r.buf >> 10) & 15u) + 4u;
    BC_INF_DROP(14u);
    if (n_lit > 286u || n_dist > 30u) return kInfBadCodeLengths;
    BC_INF_WAVE_SYNC();
    BC_INF_LANES(lane) {
      if (lane < 19u) T.lens[320u + lane] = 0;
    }
    BC_INF_WAVE_SYNC();
    constexpr uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
#pragma unroll
    for (uint32_t i = 0; i < 19u; ++i) {
      if (i < n_cl) {
        BC_INF_REFILL();
        T.lens[320u + kOrder[i]] = (uint8_t)((uint32_t)r.buf & 7u);
        BC_INF_DROP(3u);
      }
    }
    if (BC_INF_OVERRUN()) return kInfInputOverrun;
    if (inflate_build(T.lens + 320, 19u, T.dist, kInfClBits, T.dcount, T.dsym, T.offs, self_lane) != 0) return kInfBadCodeLengths;
    const uint32_t n_all = n_lit + n_dist;
    uint32_t idx = 0;
    while (idx < n_all) {  // (every turn adds at least one length)
      BC_INF_REFILL();
      uint32_t cl = 0;
      const int sym = inflate_symbol(r.buf, T.dist, kInfClBits, T.dcount, T.dsym, &cl);
      if (sym < 0) return kInfBadSymbol;
      BC_INF_DROP(cl);
      uint32_t value = (uint32_t)sym, rep = 1;
      if (sym == 16) {
        if (idx == 0) return kInfBadCodeLengths;
        value = T.lens[idx - 1];
        rep = 3u + ((uint32_t)r.buf & 3u);
        BC_INF_DROP(2u);
      } else if (sym == 17) {
        value = 0;
        rep = 3u + ((uint32_t)r.buf & 7u);
        BC_INF_DROP(3u);
      } else if (sym == 18) {
        value = 0;
        rep = 11u + ((uint32_t)r.buf & 127u);
        BC_INF_DROP(7u);
      }
      if (BC_INF_OVERRUN()) return kInfInputOverrun;
      if (rep > n_all - idx) return kInfBadCodeLengths;
      for (uint32_t k = 0; k < rep; ++k) T.lens[idx + k] = (uint8_t)value;  // (the same store on every lane)
      idx += rep;
    }
    BC_INF_WAVE_SYNC();
    if (T.lens[256] == 0) return kInfBadCodeLengths;
  }
  const int left_lit = inflate_build(T.lens, n_lit, T.lit, kInfLitBits, T.lcount, T.lsym, T.offs, self_lane);
  const int left_dist = inflate_build(T.lens + n_lit, n_dist, T.dist, kInfDistBits, T.dcount, T.dsym, T.offs, self_lane);
  if (left_lit < 0 || left_dist < 0) return kInfBadCodeLengths;
  if (type == 2u) {
    // as zlib: an incomplete literal/length code is refused; an incomplete distance code only passes when it has no
    // code at all (a block of literals) or a single code of one bit
    if (left_lit > 0) return kInfBadCodeLengths;
    uint32_t n_codes = 0;
    for (uint32_t l = 1; l <= 15u; ++l) n_codes += T.dcount[l];
    if (left_dist > 0 && !(n_codes == 0u || (n_codes == 1u && T.dcount[1] == 1u))) return kInfBadCodeLengths;
  }
  return kInfOk;
#undef BC_INF_REFILL
#undef BC_INF_DROP
#undef BC_INF_OVERRUN
}

// the length of a match from its symbol (257 .. 285) and the extra bits on `r`
BC_HD uint32_t inflate_match_length(InflateBits& r, uint32_t sym) {
  if (sym < 265u) return sym - 254u;
  if (sym == 285u) return 258u;
  const uint32_t eb = (sym - 261u) >> 2;
  const uint32_t len = 3u + ((4u + ((sym - 265u) & 3u)) << eb) + ((uint32_t)r.buf & ((1u << eb) - 1u));
  inflate_drop(r, eb);
  return len;
}
// the distance of a match from its symbol (0 .. 29) and the extra bits on `r`
BC_HD uint32_t inflate_match_distance(InflateBits& r, uint32_t ds) {
  if (ds < 4u) return ds + 1u;
  const uint32_t eb = (ds >> 1) - 1u;
  const uint32_t dist = 1u + ((2u + (ds & 1u)) << eb) + ((uint32_t)r.buf & ((1u << eb) - 1u));
  inflate_drop(r, eb);
  return dist;
}

// Inflates the deflate stream src[0, src_len) into out[0, isize) and checks ISIZE and CRC32.  Called by all 64 lanes of
// a wave with the same arguments (self_lane = the lane's number; the host passes 0 and plays every lane in turn).
BC_HD uint32_t inflate_member(const BC_GLOBAL uint8_t* src, uint32_t src_len, BC_GLOBAL uint8_t* out, uint32_t isize,
                              uint32_t want_crc, InflateTables& T, const uint32_t* crc_tab, uint32_t self_lane) {
  (void)self_lane;
  InflateBits r;
  r.win_base = 0u - kInfWindow;
  uint32_t pos = 0;  // bytes of output made

#define BC_INF_REFILL() inflate_refill(r, src, src_len, T, self_lane)
#define BC_INF_DROP(n) inflate_drop(r, (n))
#define BC_INF_OVERRUN() inflate_overrun(r, src_len)

  uint32_t last = 0;
  do {
    BC_INF_REFILL();
    last = (uint32_t)r.buf & 1u;
    const uint32_t type = ((uint32_t)r.buf >> 1) & 3u;
    BC_INF_DROP(3u);
    if (BC_INF_OVERRUN()) return kInfInputOverrun;
    if (type == 3u) return kInfBadBlockType;
    if (type == 0u) {
      BC_INF_DROP(r.cnt & 7u);
      BC_INF_REFILL();
      const uint32_t len = (uint32_t)r.buf & 0xFFFFu, nlen = ((uint32_t)r.buf >> 16) & 0xFFFFu;
      BC_INF_DROP(32u);
      if (BC_INF_OVERRUN()) return kInfInputOverrun;
      if ((len ^ 0xFFFFu) != nlen) return kInfBadBlockType;
      const uint32_t from = r.in_pos - (r.cnt >> 3);  // (cnt is a multiple of 8 here)
      if (len > src_len - from) return kInfInputOverrun;
      if (len > isize - pos) return kInfOutputOverrun;
      for (uint32_t base = 0; base < len; base += 64u) {
        BC_INF_LANES(lane) {
          const uint32_t i = base + lane;
          if (i < len) out[pos + i] = src[from + i];
        }
      }
      pos += len;
      r.buf = 0;
      r.cnt = 0;
      r.in_pos = from + len;
      r.win_base = r.in_pos - kInfWindow;
      continue;
    }
    {
      const uint32_t st = inflate_block_tables(r, src, src_len, type, T, self_lane);
      if (st != kInfOk) return st;
    }
    for (;;) {  // (every turn consumes at least one bit: bounded by the overrun check)
      BC_INF_REFILL();
      uint32_t cl = 0;
      const int sym = inflate_symbol(r.buf, T.lit, kInfLitBits, T.lcount, T.lsym, &cl);
      if (sym < 0) return kInfBadSymbol;
      BC_INF_DROP(cl);
      if (BC_INF_OVERRUN()) return kInfInputOverrun;
      if (sym < 256) {
        if (pos >= isize) return kInfOutputOverrun;
        BC_INF_LANES(lane) {
          if (lane == (pos & 63u)) out[pos] = (uint8_t)sym;
        }
        ++pos;
        continue;
      }
      if (sym == 256) break;
      if (sym > 285) return kInfBadSymbol;
      const uint32_t len = inflate_match_length(r, (uint32_t)sym);
      BC_INF_REFILL();
      const int ds = inflate_symbol(r.buf, T.dist, kInfDistBits, T.dcount, T.dsym, &cl);
      if (ds < 0 || ds > 29) return kInfBadSymbol;
      BC_INF_DROP(cl);
      const uint32_t dist = inflate_match_distance(r, (uint32_t)ds);
      if (BC_INF_OVERRUN()) return kInfInputOverrun;
      if (dist > pos) return kInfBadSymbol;
      if (len > isize - pos) return kInfOutputOverrun;
      // 64 bytes per step.  dist >= 64: a step's sources were all written before the step.  dist < 64: the match is
      // the dist bytes before `pos` over and over, which were all written before the match.
      for (uint32_t base = 0; base < len; base += 64u) {
        BC_INF_WAVE_SYNC();
        BC_INF_LANES(lane) {
          const uint32_t i = base + lane;
          if (i < len) {
            const uint32_t from = dist >= 64u ? pos + i - dist : pos - dist + i % dist;
            out[pos + i] = out[from];
          }
        }
      }
      pos += len;
    }
  } while (!last);
#undef BC_INF_REFILL
#undef BC_INF_DROP
#undef BC_INF_OVERRUN
  if (pos != isize) return kInfIsizeMismatch;

  // CRC-32: a contiguous slice per lane, each slice's value moved to its place by x^(8 * bytes behind it), all XORed
  BC_INF_WAVE_SYNC();
  const uint32_t slice = (isize + 63u) / 64u;
  BC_INF_LANES(lane) {
    const uint32_t a = lane * slice < isize ? lane * slice : isize;
    const uint32_t b = a + slice < isize ? a + slice : isize;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = a; i < b; ++i) c = crc_tab[(c ^ out[i]) & 0xFFu] ^ (c >> 8);
    c ^= 0xFFFFFFFFu;
    T.red[lane] = b > a ? crc32_mulmod(crc32_x8n(isize - b), c) : 0u;
  }
  BC_INF_WAVE_SYNC();
  uint32_t crc = 0;
  for (uint32_t l = 0; l < 64u; ++l) crc ^= T.red[l];
  return crc == want_crc ? (uint32_t)kInfOk : (uint32_t)kInfCrcMismatch;
}

BC_HD const char* inflate_status_name(uint32_t s) {
  switch (s) {
    case kInfOk: return "ok";
    case kInfBadBlockType: return "bad block type";
    case kInfBadCodeLengths: return "bad code lengths";
    case kInfBadSymbol: return "invalid symbol or distance";
    case kInfInputOverrun: return "input overrun";
    case kInfOutputOverrun: return "output overrun";
    case kInfIsizeMismatch: return "ISIZE mismatch";
    case kInfCrcMismatch: return "CRC32 mismatch";
  }
  return "unknown status";
}

}  // namespace bc
