// bc_fastq_host.hpp -- the parts of the FASTQ ingest (bc_ingest.hip) that decide counts and need no GPU: which input
// path a file takes, the first-record check, the end-of-stream rules, the gzip member header, how a BGZF index is cut
// into chunks and shards, where a shard's first record starts, and the header of a BAM file.  Plain C++17: every function returns a code or a small
// struct, the caller words the error.  Tested on the host with sanitizers (tests/ingest/ingest_host.cpp).
#pragma once
#include <stdint.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <functional>
#include <string>
#include <vector>

#include "bc_bgzf.hpp"

namespace bc {

// How a file's text reaches the device; decided once per call from the file name, BC_GZ_DEVICE and the BGZF index.
enum class InputPath {
  Plain,       // *.fastq: pread into pinned memory
  Zlib,        // *.fastq.gz through gzread on the host
  BgzfDevice,  // *.fastq.gz that is BGZF through and through: the compressed blocks travel, bc_inflate.hip inflates them
  GzipDevice,  // *.fastq.gz, any gzip stream, BC_GZ_DEVICE=all: span by span through bc_gunzip.hip
  BamDevice,   // *.bam (unaligned BAM): BGZF blocks as above, then the record framing of bc_bam.hip instead of newlines
};
// The reference reads a .gz file with read_line, a plain one with BufReader::lines(): a '\r' before the newline stays
// (input.rs:66-68 against input.rs:44), and the reader is handed one more, empty line at the end of the stream
// (input.rs:69-73).
// (Neither applies to BAM: its records are binary, and every whole one is one read.)
inline bool gz_line_rules(InputPath p) { return p != InputPath::Plain && p != InputPath::BamDevice; }
// the file is read by its BGZF index, block by block, and inflated by bc_inflate.hip
inline bool bgzf_blocks(InputPath p) { return p == InputPath::BgzfDevice || p == InputPath::BamDevice; }
// the text arrives on the device without a host copy: the host sees compressed bytes only
inline bool text_on_device(InputPath p) { return bgzf_blocks(p) || p == InputPath::GzipDevice; }
inline const char* input_path_name(InputPath p) {
  switch (p) {
    case InputPath::Plain: return "plain";
    case InputPath::Zlib: return "gzread";
    case InputPath::BgzfDevice: return "bgzf-device";
    case InputPath::BamDevice: return "bam-device";
    default: return "gzip-device";
  }
}

inline bool ends_with(const std::string& s, const char* suf) {
  const size_t n = strlen(suf);
  return s.size() >= n && memcmp(s.data() + s.size() - n, suf, n) == 0;
}

// test_sequence (parse.rs:414-427): a line is "Sequence" unless fewer than half of its bytes are A,G,C,T,N
inline bool looks_like_sequence(const char* s, size_t n) {
  size_t dna = 0;
  for (size_t i = 0; i < n; ++i) dna += s[i] == 'A' || s[i] == 'G' || s[i] == 'C' || s[i] == 'T' || s[i] == 'N';
  return !(dna < n / 2);
}

// First record only (input.rs:139-142, parse.rs:377-394): lines 1 and 2 of the file, in the stream's first `len` bytes of
// text.  `eof`: the stream ends with them.
enum class FirstRecord { Ok, FirstLineIsSequence, SecondLineNotSequence };
inline FirstRecord first_record_check(const char* t, size_t len, bool eof, bool gz_rules) {
  const char* e1 = len ? (const char*)memchr(t, '\n', len) : nullptr;
  const char* e2 = e1 ? (const char*)memchr(e1 + 1, '\n', len - (size_t)(e1 + 1 - t)) : nullptr;
  // (a file of fewer than four whole lines never posts a record, so the reference never looks at it)
  const char* e3 = e2 ? (const char*)memchr(e2 + 1, '\n', len - (size_t)(e2 + 1 - t)) : nullptr;
  const bool whole = e3 && (memchr(e3 + 1, '\n', len - (size_t)(e3 + 1 - t)) || (eof && !gz_rules && (size_t)(e3 + 1 - t) < len));
  if (!whole) return FirstRecord::Ok;
  size_t n1 = (size_t)(e1 - t), n2 = (size_t)(e2 - (e1 + 1));
  if (!gz_rules && n1 && t[n1 - 1] == '\r') --n1;
  if (!gz_rules && n2 && e2[-1] == '\r') --n2;
  if (looks_like_sequence(t, n1)) return FirstRecord::FirstLineIsSequence;
  if (!looks_like_sequence(e1 + 1, n2)) return FirstRecord::SecondLineNotSequence;
  return FirstRecord::Ok;
}

// What the end of the stream adds to "Total sequences", given the whole lines `seen` (0..3) after the last whole record.
// `gz_end`: the gz line rules apply and this call reads the stream's end.
struct StreamTail {
  unsigned extra_total;
  bool post_partial_record;
};
inline StreamTail stream_tail(size_t seen, bool gz_end) {
  StreamTail t = {0, false};
  if (seen > 0 && seen < 4) t.extra_total += 1;  // a trailing partial record is counted when its first line is seen (input.rs:128-130)
  // the gz loop calls read("") once more at EOF (input.rs:69-73): when that lands on "line 1" the total grows
  // by one (README.md:159 vs 176)
  if (gz_end && seen % 4 == 0) t.extra_total += 1;
  // After three lines of a record that empty line makes "line 4": the reference posts the partial record -- header,
  // sequence, '+' line and an EMPTY quality line (post() pops the last character, unpack() fills what lines there are:
  // parse.rs:236-267) -- and its workers score it like any other read (an empty quality line passes the quality filter:
  // nothing is zipped, parse.rs:340-345).
  t.post_partial_record = gz_end && seen == 3;
  return t;
}

// The gzip member header at bytes[0, have): > 0 its length, 0: more bytes are needed, -1: no gzip member here,
// -2: refused.  `file_end`: the file holds nothing after these bytes.
inline long gzip_member_header(const uint8_t* b, size_t have, bool file_end) {
  if (have < 10) return file_end ? -1 : 0;
  if (b[0] != 0x1F || b[1] != 0x8B) return -1;
  if (b[2] != 8 || (b[3] & 0xE0)) return -2;  // (not deflate, or reserved flags: a preset dictionary among them)
  const uint32_t flg = b[3];
  size_t p = 10;
  if (flg & 4) {  // FEXTRA
    if (have < p + 2) return file_end ? -1 : 0;
    p += 2 + ((size_t)b[p] | ((size_t)b[p + 1] << 8));
  }
  for (uint32_t f : {8u, 16u})  // FNAME, FCOMMENT
    if (flg & f) {
      const void* z = p < have ? memchr(b + p, 0, have - p) : nullptr;
      if (!z) return file_end ? -1 : 0;
      p = (size_t)((const uint8_t*)z - b) + 1;
    }
  if (flg & 2) p += 2;  // FHCRC
  if (p > have) return file_end ? -1 : 0;
  return (long)p;
}

// BGZF chunks are cut at block boundaries.  The run of blocks [from, upto) that makes the next chunk: text of at most
// `fill_cap` bytes, compressed bytes of at most `chunk`, at most `blk_cap` blocks -- but always a whole block, whatever
// its size.  upto == from only when from == end_member.
struct BgzfRun {
  size_t upto;
  unsigned long long text_bytes, comp_bytes;
};
inline BgzfRun bgzf_next_run(const std::vector<BgzfMember>& members, size_t from, size_t end_member, size_t fill_cap, size_t chunk,
                             size_t blk_cap) {
  BgzfRun r = {from, 0, 0};
  while (r.upto < end_member) {
    const BgzfMember& m = members[r.upto];
    if (r.upto > from && (r.text_bytes + m.isize > fill_cap || r.comp_bytes + m.total > chunk || r.upto - from >= blk_cap)) break;
    r.text_bytes += m.isize;
    r.comp_bytes += m.total;
    ++r.upto;
  }
  return r;
}

// The blocks that cover a shard's share [text_a, text_b) of the inflated bytes.  The text of a shared first block before
// text_a is skipped by the framing; first_member == end_member: no record starts in this shard.
struct BgzfShard {
  size_t first_member, end_member;
};
inline BgzfShard bgzf_shard_members(const std::vector<BgzfMember>& members, unsigned long long text_a, unsigned long long text_b,
                                    uint32_t shard, uint32_t n_shards) {
  BgzfShard s = {0, members.size()};
  auto starts_after = [](unsigned long long v, const BgzfMember& m) { return v < m.out_off; };
  if (shard != 0) s.first_member = (size_t)(std::upper_bound(members.begin(), members.end(), text_a, starts_after) - members.begin()) - 1;
  if (shard + 1 != n_shards) {
    s.end_member = (size_t)(std::lower_bound(members.begin(), members.end(), text_b,
                                             [](const BgzfMember& m, unsigned long long v) { return m.out_off < v; }) -
                            members.begin());
    if (text_b == text_a || s.end_member < s.first_member) s.end_member = s.first_member;
  }
  return s;
}

// First record of a plain FASTQ file that starts at or after byte `off`: the first line start p >= off whose line
// begins with '@' while the line two further down begins with '+' (a quality line may begin with '@', but then the line
// two further down is a sequence line, which never begins with '+').  `size` when there is none; -1 on a read error or
// when no record boundary is found within 16 MiB (no FASTQ record is that long: the framing kernels allow 4 MiB).
// `read_at(dst, n, at)` delivers bytes [at, at + n) of the text (fewer at its end; < 0: error): a plain file's bytes, or a
// BGZF file's inflated ones, fetched `step` bytes at a time.
using ReadAt = std::function<long(char* dst, size_t n, unsigned long long at)>;
inline long long record_start_at_or_after(const ReadAt& read_at, unsigned long long off, unsigned long long size, size_t step = 1u << 20) {
  if (off == 0) return 0;
  if (off >= size) return (long long)size;
  const unsigned long long from = off - 1;  // (the byte before tells whether `off` itself starts a line)
  std::vector<char> buf;
  const size_t limit = 16u << 20;
  for (;;) {
    const size_t have = buf.size();
    if (from + have >= size || have >= limit) break;
    const size_t want = (size_t)std::min<unsigned long long>(step, size - (from + have));
    buf.resize(have + want);
    const long got = read_at(buf.data() + have, want, from + have);
    // (want > 0 here, so nothing delivered means the text is shorter than `size`: truncated since it was measured)
    if (got <= 0) return -1;
    buf.resize(have + (size_t)got);
    const bool at_end = from + buf.size() >= size;
    // line starts inside the window (buffer offsets), from the first one at or after `off`
    size_t p = 0;
    if (buf[0] != '\n') {
      const char* nl = (const char*)memchr(buf.data(), '\n', buf.size());
      if (!nl) {
        if (at_end) return (long long)size;
        continue;  // one long line so far
      }
      p = (size_t)(nl - buf.data());
    }
    p += 1;  // first byte after a newline that sits at or after off - 1
    bool need_more = false;
    while (p < buf.size()) {
      const char* e1 = (const char*)memchr(buf.data() + p, '\n', buf.size() - p);
      const char* e2 = e1 ? (const char*)memchr(e1 + 1, '\n', buf.size() - (size_t)(e1 + 1 - buf.data())) : nullptr;
      if (!e1 || !e2 || (size_t)(e2 + 1 - buf.data()) >= buf.size()) {
        need_more = true;  // the line two further down is not in the window yet
        break;
      }
      if (buf[p] == '@' && e2[1] == '+') return (long long)(from + p);
      p = (size_t)(e1 + 1 - buf.data());
    }
    if (at_end) return (long long)size;  // fewer than three lines left: no whole record starts here
    if (!need_more && p >= buf.size()) continue;
    if (buf.size() >= limit) return -1;
  }
  return from + buf.size() >= size ? (long long)size : -1;
}

// The header of a BAM file, read from its inflated bytes: magic, l_text, the text, n_ref and the reference entries
// (l_name, name, l_ref each).  error: what is wrong with it (a literal), or null.
struct BamHeader {
  uint32_t n_ref;
  uint64_t first_record;  // inflated offset just past the dictionary
  const char* error;
};
inline BamHeader bam_parse_header(const ReadAt& read_at, uint64_t inflated) {
  BamHeader h = {0, 0, nullptr};
  auto fail = [&h](const char* what) {
    h.error = what;
    return h;
  };
  // four bytes at `at` as a little-endian word; false: the stream ends before them (or cannot be read)
  auto word = [&](uint64_t at, uint32_t* v) {
    unsigned char b[4];
    if (at > inflated || inflated - at < 4 || read_at((char*)b, 4, at) != 4) return false;
    *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    return true;
  };
  const char* cut = "the header runs past the end of the file (or a block of it is damaged)";
  uint32_t magic = 0, l_text = 0, l_name = 0;
  if (!word(0, &magic)) return fail("no room for the magic");
  if (magic != 0x014D4142u) return fail("bad magic (not \"BAM\\1\")");
  if (!word(4, &l_text)) return fail(cut);
  uint64_t at = 8ull + l_text;
  if (!word(at, &h.n_ref)) return fail(cut);
  at += 4;
  if (h.n_ref > 0x7FFFFFFFu) return fail("a negative number of references");
  for (uint32_t r = 0; r < h.n_ref; ++r) {
    if (!word(at, &l_name)) return fail(cut);
    at += 4ull + l_name;
    if (at > inflated || inflated - at < 4) return fail(cut);
    at += 4;  // l_ref
  }
  h.first_record = at;
  return h;
}

inline ReadAt plain_reader(int fd) {
  return [fd](char* dst, size_t want, unsigned long long at) -> long {
    size_t got = 0;
    while (got < want) {
      const ssize_t n = pread(fd, dst + got, want - got, (off_t)(at + got));
      if (n < 0) return -1;
      if (n == 0) break;
      got += (size_t)n;
    }
    return (long)got;
  };
}

}  // namespace bc
