// ingest_host -- the FASTQ ingest's host-only logic (csrc/bc_fastq_host.hpp) behind a query file, compiled with
// sanitizers.  TEST-ONLY.
//
//   ingest_host IN OUT
//
// IN holds one query per line, OUT gets one answer line per query.  Bytes travel as hex ("-": none) and are handed to the
// code under test in a heap block of exactly their size, so AddressSanitizer sees any access outside them.
//
//   header FILE_END HEX               -> gzip_member_header
//   first EOF GZ_RULES HEX            -> first_record_check: 0 ok, 1 first line is a sequence, 2 second line is not
//   tail SEEN GZ_END                  -> stream_tail: EXTRA_TOTAL POST_PARTIAL_RECORD
//   members N ISIZE TOTAL ...         -> (sets the BGZF index of the queries below: N blocks, laid end to end)  "ok"
//   runs FROM END FILL_CAP CHUNK BLK_CAP -> bgzf_next_run from FROM on, each run starting where the last one ended, until END or
//                                        an empty run: UPTO TEXT COMP ... (three numbers per run)
//   shard TEXT_A TEXT_B SHARD N_SHARDS -> bgzf_shard_members: FIRST END
//   start_empty OFF SIZE DRY          -> record_start_at_or_after with a reader whose call number DRY (from 0) delivers
//                                        nothing; every other call delivers a stretch of one long line: ANSWER CALLS
//
// Exit status 0: every query answered; 2: bad arguments or a query it does not know; a sanitizer report ends the process
// with its own status.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_fastq_host.hpp"

using namespace bc;

// the bytes of a hex word in a heap block of their own size (nullptr for none)
struct Bytes {
  uint8_t* p = nullptr;
  size_t n = 0;
  explicit Bytes(const std::string& hex) {
    if (hex == "-") return;
    n = hex.size() / 2;
    p = (uint8_t*)malloc(n);
    for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
  }
  ~Bytes() { free(p); }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1]);
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 2;
  std::vector<BgzfMember> members;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream q(line);
    std::string what;
    q >> what;
    if (what == "header") {
      int file_end;
      std::string hex;
      q >> file_end >> hex;
      const Bytes b(hex);
      fprintf(out, "%ld\n", gzip_member_header(b.p, b.n, file_end != 0));
    } else if (what == "first") {
      int eof, gz_rules;
      std::string hex;
      q >> eof >> gz_rules >> hex;
      const Bytes b(hex);
      fprintf(out, "%d\n", (int)first_record_check((const char*)b.p, b.n, eof != 0, gz_rules != 0));
    } else if (what == "tail") {
      size_t seen;
      int gz_end;
      q >> seen >> gz_end;
      const StreamTail t = stream_tail(seen, gz_end != 0);
      fprintf(out, "%u %d\n", t.extra_total, t.post_partial_record ? 1 : 0);
    } else if (what == "members") {
      size_t n;
      q >> n;
      members.assign(n, BgzfMember{});
      uint64_t file_off = 0, out_off = 0;
      for (BgzfMember& m : members) {
        q >> m.isize >> m.total;
        m.file_off = file_off;
        m.out_off = out_off;
        file_off += m.total;
        out_off += m.isize;
      }
      fprintf(out, "ok\n");
    } else if (what == "runs") {
      size_t from, end, fill_cap, chunk, blk_cap;
      q >> from >> end >> fill_cap >> chunk >> blk_cap;
      while (from < end) {
        const BgzfRun r = bgzf_next_run(members, from, end, fill_cap, chunk, blk_cap);
        fprintf(out, "%zu %llu %llu ", r.upto, r.text_bytes, r.comp_bytes);
        if (r.upto <= from) break;
        from = r.upto;
      }
      fprintf(out, "\n");
    } else if (what == "shard") {
      unsigned long long text_a, text_b;
      uint32_t shard, n_shards;
      q >> text_a >> text_b >> shard >> n_shards;
      const BgzfShard s = bgzf_shard_members(members, text_a, text_b, shard, n_shards);
      fprintf(out, "%zu %zu\n", s.first_member, s.end_member);
    } else if (what == "start_empty") {
      unsigned long long off, size;
      int dry;
      q >> off >> size >> dry;
      int calls = 0;
      const ReadAt runs_dry = [&calls, dry](char* dst, size_t n, unsigned long long) -> long {
        if (calls++ == dry) return 0;
        memset(dst, 'A', n);
        return (long)n;
      };
      const long long at = record_start_at_or_after(runs_dry, off, size);
      fprintf(out, "%lld %d\n", at, calls);  // (the answer, and how often the reader was asked)
    } else {
      return 2;
    }
    if (q.fail()) return 2;
  }
  fclose(out);
  return 0;
}
