// bc_gunzip.h -- a SPAN of an ordinary gzip member (one long deflate stream, not BGZF), inflated by many wavefronts.
//
// Lane code in the style of bc_inflate.h, whose bit reader, table builder and block-header reader it calls: the same
// text compiles for the device (bc_gunzip.hip) and for the host (tests/gunzip/gunzip_host.cpp, with sanitizers).
//
// A span is the compressed bytes src[0, src_len), a start bit that is a known block boundary (the anchor) and the
// 32 KiB of text before it.  Nothing else about the stream is known, so (as pugz and rapidgzip do):
//
//   find     a wavefront per partition of `part_bytes` compressed bytes looks for the first bit offset at which a
//            dynamic block header passes every check the decoder applies: the partition's candidate;
//   measure  a wavefront per candidate (and one for the anchor) decodes without storing, counting bytes, until a block
//            ends exactly on a later candidate (a link), the final block ends, or the bytes run out;
//   chain    the host follows the links from the anchor: the segments on that path are real, every other candidate is
//            false; a prefix sum of their sizes gives every segment its place in the text;
//   decode   a wavefront per segment decodes again, into 16-bit symbols: a byte, or 256 + k for "byte k of the 32 KiB
//            before this segment", which the segment does not know;
//   resolve  segment after segment, the last 32 KiB of each become bytes (one workgroup); then every symbol becomes a
//            byte through the 32 KiB before its segment, all at once, and a CRC-32 per segment is taken.
//
// No stage waits for another wavefront: every stage is a kernel that ends on its own.  Every loop is bounded by bits
// consumed or bytes produced; every load and store is checked against its buffer.
#pragma once
#include "bc_inflate.h"

#include <vector>

namespace bc {

constexpr uint32_t kGzHistory = 32768;
constexpr uint32_t kGzNone = 0xFFFFFFFFu;
constexpr uint32_t kGzSliceBytes = 32768;  // text bytes per wavefront of the parallel resolve

// why a measure stopped
enum : uint32_t {
  kGzEndLink = 0,   // a block ended on candidate `link`
  kGzEndFinal = 1,  // the member's last block ended
  kGzEndInput = 2,  // the bytes ran out: end_bit is the last block end before that
  kGzEndFull = 3,   // more text than the budget: end_bit is the last block end within it
  kGzEndError = 4,  // not a deflate stream from here (`status` says why)
};

struct GzMeasure {
  uint32_t end_bit, out_bytes, reason, link, status;
};

struct GzSegment {
  uint32_t start_bit, end_bit;
  uint32_t out_off, out_bytes;
  uint32_t anchor, pad;
};

struct GzSlice {
  uint32_t seg, from, upto, pad;  // text bytes [from, upto) of segment `seg`
};

#if defined(__HIP_DEVICE_COMPILE__)
#define BC_GZ_VOTE(mask, lane, pred) mask = __builtin_amdgcn_ballot_w64(pred)
#else
#define BC_GZ_VOTE(mask, lane, pred) mask |= (uint64_t)((pred) ? 1u : 0u) << (lane)
#endif

// the bit reader at bit `bit` of the span
BC_HD void gunzip_seek(InflateBits& r, uint32_t bit, const BC_GLOBAL uint8_t* src, uint32_t src_len, InflateTables& T, uint32_t self_lane) {
  r.buf = 0;
  r.cnt = 0;
  r.in_pos = bit >> 3;
  r.win_base = r.in_pos - kInfWindow;
  inflate_refill(r, src, src_len, T, self_lane);
  inflate_drop(r, bit & 7u);
}
BC_HD uint32_t gunzip_bit(const InflateBits& r) { return 8u * r.in_pos - r.cnt; }

// n <= 25 bits at bit `at` of the six words of the find window
BC_HD uint32_t gunzip_window_bits(const uint32_t* win, uint32_t at, uint32_t n) {
  const uint32_t w = at >> 5, sh = at & 31u;
  uint32_t v = win[w] >> sh;
  if (sh) v |= win[w + 1] << (32u - sh);
  return v & ((1u << n) - 1u);
}

// FIND: the first bit offset in (after_bit, ...) and [8 * part_from, 8 * part_upto) at which a dynamic block header
// passes the decoder's own checks; kGzNone when there is none.
BC_HD uint32_t gunzip_find(const BC_GLOBAL uint8_t* src, uint32_t src_len, uint32_t after_bit, uint32_t part_from, uint32_t part_upto,
                           InflateTables& T, uint32_t self_lane) {
  (void)self_lane;
  if (part_upto > src_len) part_upto = src_len;
  // (no offset up to after_bit can pass: the walk begins at its byte, on the partition's 8-byte grid; a partition that
  // lies wholly before it is not walked at all)
  if ((after_bit >> 3) > part_from) part_from += ((after_bit >> 3) - part_from) & ~7u;
  for (uint32_t byte0 = part_from; byte0 < part_upto; byte0 += 8u) {  // 64 bit offsets per turn
    BC_INF_WAVE_SYNC();
    BC_INF_LANES(lane) {
      if (lane < 6u) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4u; ++k) {
          const uint32_t at = byte0 + 4u * lane + k;
          if (at < src_len) w |= (uint32_t)src[at] << (8u * k);
        }
        T.win[lane] = w;
      }
    }
    BC_INF_WAVE_SYNC();
    uint64_t surv = 0;
    BC_INF_LANES(lane) {
      // the cheap tests: BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, a complete code-length code
      const uint32_t o = 8u * byte0 + lane;
      bool ok = o > after_bit && o < 8u * part_upto;
      const uint32_t head = gunzip_window_bits(T.win, lane, 17u);
      ok = ok && (head & 7u) == 4u && ((head >> 3) & 31u) <= 29u && ((head >> 8) & 31u) <= 29u;
      const uint32_t n_cl = ((head >> 13) & 15u) + 4u;
      uint32_t kraft = 0;
      for (uint32_t i = 0; i < 19u; ++i) {
        const uint32_t l = gunzip_window_bits(T.win, lane + 17u + 3u * i, 3u);
        if (i < n_cl && l) kraft += 128u >> l;
      }
      ok = ok && kraft == 128u;
      BC_GZ_VOTE(surv, lane, ok);
    }
    // the survivors, one at a time, through the full header check (it reuses the window: the votes are in already)
    while (surv) {
      const uint32_t lane_of = (uint32_t)__builtin_ctzll(surv);
      surv &= surv - 1u;
      const uint32_t o = 8u * byte0 + lane_of;
      InflateBits r;
      gunzip_seek(r, o, src, src_len, T, self_lane);
      inflate_drop(r, 3u);
      if (inflate_block_tables(r, src, src_len, 2u, T, self_lane) == kInfOk) return o;
    }
  }
  return kGzNone;
}

// the candidate a block end at `bit` lands on (its partition's number), or kGzNone
BC_HD uint32_t gunzip_candidate_at(const uint32_t* cand, uint32_t n_parts, uint32_t part_bytes, uint32_t bit) {
  const uint32_t p = (bit >> 3) / part_bytes;
  return p < n_parts && cand[p] == bit ? p : kGzNone;
}

// MEASURE: decodes from start_bit without storing.  `budget`: the most text the caller can take.
BC_HD GzMeasure gunzip_measure(const BC_GLOBAL uint8_t* src, uint32_t src_len, uint32_t start_bit, const uint32_t* cand, uint32_t n_parts,
                               uint32_t part_bytes, uint32_t budget, InflateTables& T, uint32_t self_lane) {
  GzMeasure m;
  m.end_bit = start_bit;
  m.out_bytes = 0;
  m.reason = kGzEndInput;
  m.link = kGzNone;
  m.status = kInfOk;
  InflateBits r;
  gunzip_seek(r, start_bit, src, src_len, T, self_lane);
  uint32_t pos = 0;
  // (bits past the span's end read as zero: what looks like an error within a step's reach of the end, 28 bits, is the
  // bytes running out; a stream that is damaged there shows when the caller comes back with more bytes, or with none)
#define BC_GZ_ERROR(st)                                          \
  do {                                                           \
    if (r.in_pos - (r.cnt >> 3) + 4u > src_len) return m;        \
    m.reason = kGzEndError;                                      \
    m.status = (st);                                             \
    return m;                                                    \
  } while (0)
  for (;;) {  // (a block consumes at least three bits: bounded by the overrun check)
    inflate_refill(r, src, src_len, T, self_lane);
    const uint32_t last = (uint32_t)r.buf & 1u, type = ((uint32_t)r.buf >> 1) & 3u;
    inflate_drop(r, 3u);
    if (inflate_overrun(r, src_len)) return m;
    if (type == 3u) BC_GZ_ERROR(kInfBadBlockType);
    if (type == 0u) {
      inflate_drop(r, r.cnt & 7u);
      inflate_refill(r, src, src_len, T, self_lane);
      const uint32_t len = (uint32_t)r.buf & 0xFFFFu, nlen = ((uint32_t)r.buf >> 16) & 0xFFFFu;
      inflate_drop(r, 32u);
      if (inflate_overrun(r, src_len)) return m;
      if ((len ^ 0xFFFFu) != nlen) BC_GZ_ERROR(kInfBadBlockType);
      const uint32_t from = r.in_pos - (r.cnt >> 3);
      if (len > src_len - from) return m;
      pos += len;
      r.buf = 0;
      r.cnt = 0;
      r.in_pos = from + len;
      r.win_base = r.in_pos - kInfWindow;
    } else {
      const uint32_t st = inflate_block_tables(r, src, src_len, type, T, self_lane);
      if (st == kInfInputOverrun) return m;
      if (st != kInfOk) BC_GZ_ERROR(st);
      for (;;) {  // (every turn consumes at least one bit)
        inflate_refill(r, src, src_len, T, self_lane);
        uint32_t cl = 0;
        const int sym = inflate_symbol(r.buf, T.lit, kInfLitBits, T.lcount, T.lsym, &cl);
        if (sym < 0) BC_GZ_ERROR(kInfBadSymbol);
        inflate_drop(r, cl);
        if (inflate_overrun(r, src_len)) return m;
        if (sym < 256) {
          ++pos;
        } else if (sym == 256) {
          break;
        } else {
          if (sym > 285) BC_GZ_ERROR(kInfBadSymbol);
          pos += inflate_match_length(r, (uint32_t)sym);
          inflate_refill(r, src, src_len, T, self_lane);
          const int ds = inflate_symbol(r.buf, T.dist, kInfDistBits, T.dcount, T.dsym, &cl);
          if (ds < 0 || ds > 29) BC_GZ_ERROR(kInfBadSymbol);
          inflate_drop(r, cl);
          (void)inflate_match_distance(r, (uint32_t)ds);  // (where it points is the decode stage's to check)
          if (inflate_overrun(r, src_len)) return m;
        }
        if (pos > budget) break;
      }
    }
    if (pos > budget) {
      m.reason = kGzEndFull;
      return m;
    }
    m.end_bit = gunzip_bit(r);
    m.out_bytes = pos;
    if (last) {
      m.reason = kGzEndFinal;
      return m;
    }
    m.link = gunzip_candidate_at(cand, n_parts, part_bytes, m.end_bit);
    if (m.link != kGzNone) {
      m.reason = kGzEndLink;
      return m;
    }
  }
#undef BC_GZ_ERROR
}

// DECODE: the blocks from seg.start_bit to seg.end_bit into out[0, seg.out_bytes) (the segment's own part of the
// symbol buffer).  The anchor reads what lies before it from `hist` (the 32 KiB before the span, of which the last
// hist_len bytes are the member's own text: a distance may not reach before those; 0 at a member's
// start); every other segment writes a marker instead.
BC_HD uint32_t gunzip_decode(const BC_GLOBAL uint8_t* src, uint32_t src_len, const GzSegment& seg, BC_GLOBAL uint16_t* out,
                             const BC_GLOBAL uint8_t* hist, uint32_t hist_len, InflateTables& T, uint32_t self_lane) {
  (void)self_lane;
  const uint32_t cap = seg.out_bytes;
  InflateBits r;
  gunzip_seek(r, seg.start_bit, src, src_len, T, self_lane);
  uint32_t pos = 0;
  while (gunzip_bit(r) < seg.end_bit) {  // (a block consumes at least three bits)
    inflate_refill(r, src, src_len, T, self_lane);
    const uint32_t type = ((uint32_t)r.buf >> 1) & 3u;
    inflate_drop(r, 3u);
    if (inflate_overrun(r, src_len)) return kInfInputOverrun;
    if (type == 3u) return kInfBadBlockType;
    if (type == 0u) {
      inflate_drop(r, r.cnt & 7u);
      inflate_refill(r, src, src_len, T, self_lane);
      const uint32_t len = (uint32_t)r.buf & 0xFFFFu, nlen = ((uint32_t)r.buf >> 16) & 0xFFFFu;
      inflate_drop(r, 32u);
      if (inflate_overrun(r, src_len)) return kInfInputOverrun;
      if ((len ^ 0xFFFFu) != nlen) return kInfBadBlockType;
      const uint32_t from = r.in_pos - (r.cnt >> 3);
      if (len > src_len - from) return kInfInputOverrun;
      if (len > cap - pos) return kInfOutputOverrun;
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
      inflate_refill(r, src, src_len, T, self_lane);
      uint32_t cl = 0;
      const int sym = inflate_symbol(r.buf, T.lit, kInfLitBits, T.lcount, T.lsym, &cl);
      if (sym < 0) return kInfBadSymbol;
      inflate_drop(r, cl);
      if (inflate_overrun(r, src_len)) return kInfInputOverrun;
      if (sym < 256) {
        if (pos >= cap) return kInfOutputOverrun;
        BC_INF_LANES(lane) {
          if (lane == (pos & 63u)) out[pos] = (uint16_t)sym;
        }
        ++pos;
        continue;
      }
      if (sym == 256) break;
      if (sym > 285) return kInfBadSymbol;
      const uint32_t len = inflate_match_length(r, (uint32_t)sym);
      inflate_refill(r, src, src_len, T, self_lane);
      const int ds = inflate_symbol(r.buf, T.dist, kInfDistBits, T.dcount, T.dsym, &cl);
      if (ds < 0 || ds > 29) return kInfBadSymbol;
      inflate_drop(r, cl);
      const uint32_t dist = inflate_match_distance(r, (uint32_t)ds);
      if (inflate_overrun(r, src_len)) return kInfInputOverrun;
      // a distance that reaches more than 32 KiB before the segment, or before the member's start on the anchor
      if (dist > pos && (dist - pos > kGzHistory || (seg.anchor && dist - pos > hist_len))) return kInfBadSymbol;
      if (len > cap - pos) return kInfOutputOverrun;
      // 64 symbols per step, as inflate_member: dist >= 64: a step's sources were all written before the step;
      // dist < 64: the match is the dist symbols before `pos` over and over
      for (uint32_t base = 0; base < len; base += 64u) {
        BC_INF_WAVE_SYNC();
        BC_INF_LANES(lane) {
          const uint32_t i = base + lane;
          if (i < len) {
            const uint32_t fwd = dist >= 64u ? i : i % dist;  // source = pos - dist + fwd
            uint16_t v;
            if (pos + fwd >= dist) {
              v = out[pos + fwd - dist];
            } else {
              const uint32_t d = dist - pos - fwd;  // bytes before the segment's start, 1 .. 32768
              v = seg.anchor ? (uint16_t)hist[kGzHistory - d] : (uint16_t)(256u + (kGzHistory - d));
            }
            out[pos + i] = v;
          }
        }
      }
      pos += len;
    }
  }
  BC_INF_WAVE_SYNC();
  if (gunzip_bit(r) != seg.end_bit) return kInfBadSymbol;
  return pos == cap ? (uint32_t)kInfOk : (uint32_t)kInfIsizeMismatch;
}

// one symbol of a segment that starts at text offset seg_off -> its byte; *bad: it points before the member's start
BC_HD uint8_t gunzip_resolve_one(uint16_t v, uint32_t seg_off, const BC_GLOBAL uint8_t* text, const BC_GLOBAL uint8_t* hist, uint32_t hist_len,
                                 uint32_t* bad) {
  if (v < 256u) return (uint8_t)v;
  const uint32_t k = (uint32_t)v - 256u;
  if (k >= kGzHistory) {
    *bad = 1;
    return 0;
  }
  if (seg_off + k >= kGzHistory) return text[seg_off + k - kGzHistory];
  if (seg_off + k < kGzHistory - hist_len) {  // before the member's first byte
    *bad = 1;
    return 0;
  }
  return hist[seg_off + k];  // (kGzHistory - (kGzHistory - seg_off - k) bytes into the history)
}

// RESOLVE, sequential step: the last 32 KiB of one segment, by thread `tid` of `n_threads`.  The 32 KiB before the
// segment are resolved already (they are the last 32 KiB of the segments before it).
BC_HD void gunzip_resolve_tail(const BC_GLOBAL uint16_t* sym, BC_GLOBAL uint8_t* text, const BC_GLOBAL uint8_t* hist, uint32_t hist_len,
                               const GzSegment& seg, uint32_t tid, uint32_t n_threads, uint32_t* bad) {
  const uint32_t from = seg.out_bytes > kGzHistory ? seg.out_bytes - kGzHistory : 0u;
  for (uint32_t i = from + tid; i < seg.out_bytes; i += n_threads)
    text[seg.out_off + i] = gunzip_resolve_one(sym[seg.out_off + i], seg.out_off, text, hist, hist_len, bad);
}

// RESOLVE, parallel step: bytes [sl.from, sl.upto) of a segment (those the sequential step has not made), then the
// slice's CRC-32 term of the segment's CRC (the slice's own CRC moved by the bytes behind it in the segment)
BC_HD uint32_t gunzip_resolve_slice(const BC_GLOBAL uint16_t* sym, BC_GLOBAL uint8_t* text, const BC_GLOBAL uint8_t* hist, uint32_t hist_len,
                                    const GzSegment& seg, const GzSlice& sl, uint32_t* red, const uint32_t* crc_tab, uint32_t self_lane, uint32_t* bad) {
  (void)self_lane;
  const uint32_t tail = seg.out_bytes > kGzHistory ? seg.out_bytes - kGzHistory : 0u;
  const uint32_t upto = sl.upto < seg.out_bytes ? sl.upto : seg.out_bytes;
  for (uint32_t base = sl.from; base < upto && base < tail; base += 64u) {
    BC_INF_LANES(lane) {
      const uint32_t i = base + lane;
      if (i < upto && i < tail) text[seg.out_off + i] = gunzip_resolve_one(sym[seg.out_off + i], seg.out_off, text, hist, hist_len, bad);
    }
  }
  BC_INF_WAVE_SYNC();
  const uint32_t n = upto > sl.from ? upto - sl.from : 0u, per = (n + 63u) / 64u;
  BC_INF_LANES(lane) {
    const uint32_t a = sl.from + (lane * per < n ? lane * per : n);
    const uint32_t b = a + per < upto ? a + per : upto;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = a; i < b; ++i) c = crc_tab[(c ^ text[seg.out_off + i]) & 0xFFu] ^ (c >> 8);
    c ^= 0xFFFFFFFFu;
    red[lane] = b > a ? crc32_mulmod(crc32_x8n(seg.out_bytes - b), c) : 0u;
  }
  BC_INF_WAVE_SYNC();
  uint32_t crc = 0;
  for (uint32_t l = 0; l < 64u; ++l) crc ^= red[l];
  return crc;
}

// ---- host only: the chain walk and what the launcher derives from it ----

// statuses of a span (BC_GUNZIP_* of the C ABI)
enum : uint32_t { kGzOk = 0, kGzOutputFull = 1, kGzBadStream = 2 };

struct GzChain {
  uint32_t status = kGzOk, detail = kInfOk;
  uint32_t text_bytes = 0, end_bit = 0, member_end = 0, rejected = 0;
  std::vector<GzSegment> segs;
  std::vector<GzSlice> slices;
};

// CHAIN: meas[0] is the anchor's measure, meas[1 + p] that of partition p's candidate.  The segments that fit
// `capacity`; when one does not, the status is kGzOutputFull and end_bit the last boundary that does fit.
inline GzChain gunzip_chain(uint32_t start_bit, const uint32_t* cand, uint32_t n_parts, const GzMeasure* meas, uint32_t capacity) {
  GzChain c;
  c.end_bit = start_bit;
  uint32_t verified = 0;
  uint32_t cur = 0, at = start_bit;
  for (uint32_t turn = 0; turn <= n_parts; ++turn) {  // (a link goes to a later partition: at most n_parts + 1 segments)
    const GzMeasure& m = meas[cur];
    if (m.reason == kGzEndError) {
      c.status = kGzBadStream;
      c.detail = m.status;
      break;
    }
    if (m.end_bit != at) {  // at least one whole block
      if (m.out_bytes > capacity - c.text_bytes) {
        c.status = kGzOutputFull;
        break;
      }
      GzSegment s;
      s.start_bit = at;
      s.end_bit = m.end_bit;
      s.out_off = c.text_bytes;
      s.out_bytes = m.out_bytes;
      s.anchor = cur == 0;
      s.pad = 0;
      c.segs.push_back(s);
      c.text_bytes += m.out_bytes;
      c.end_bit = m.end_bit;
    }
    if (m.reason == kGzEndFull) {
      c.status = kGzOutputFull;
      break;
    }
    if (m.reason == kGzEndFinal) {
      c.member_end = 1;
      break;
    }
    if (m.reason != kGzEndLink || m.link >= n_parts || cand[m.link] != m.end_bit) break;  // the bytes ran out
    ++verified;
    cur = 1u + m.link;
    at = m.end_bit;
  }
  // rejected: the candidates the chain walked past without landing on them (those beyond its end were never reached:
  // most of them are real block headers of text that did not fit, or of blocks the span does not hold whole)
  uint32_t passed = 0;
  for (uint32_t p = 0; p < n_parts; ++p) passed += cand[p] != kGzNone && cand[p] <= c.end_bit;
  c.rejected = passed - verified;
  if (c.status == kGzBadStream) {
    c.segs.clear();
    c.text_bytes = 0;
    c.end_bit = start_bit;
    c.member_end = 0;
  }
  if (c.status == kGzOutputFull) c.member_end = 0;
  for (uint32_t s = 0; s < c.segs.size(); ++s)
    for (uint32_t from = 0; from < c.segs[s].out_bytes; from += kGzSliceBytes) {
      GzSlice sl;
      sl.seg = s;
      sl.from = from;
      sl.upto = from + kGzSliceBytes < c.segs[s].out_bytes ? from + kGzSliceBytes : c.segs[s].out_bytes;
      sl.pad = 0;
      c.slices.push_back(sl);
    }
  return c;
}

// crc(A ++ B) from crc(A), crc(B) and B's length (zlib's crc32_combine, with this header's arithmetic)
inline uint32_t gunzip_crc_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) {
  return crc32_mulmod(crc32_x8n(len_b), crc_a) ^ crc_b;
}

}  // namespace bc
