// inflate_host -- the device inflater's decoder (csrc/bc_inflate.h) compiled for the host, with sanitizers.  TEST-ONLY.
//
//   inflate_host IN OUT
//
// IN : u64 n_blocks, u64 src_bytes, u64 dst_bytes, then n_blocks x {u64 src_off, u64 dst_off, u32 src_len, u32 isize,
//      u32 crc32, u32 pad}, then src_bytes of compressed data (the arguments of bc_bgzf_inflate_device).
// OUT: n_blocks x u32 status, then dst_bytes of output (0xAA where nothing was written).
//
// Every block's deflate stream and output live in heap blocks of exactly their own size, so AddressSanitizer sees any
// access outside [0, src_len) or [0, isize).  Exit status 0: ran (whatever the blocks' statuses); 2: bad arguments or
// a table that contradicts the sizes; a sanitizer report ends the process with its own status.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../ngs-barcode-count_amd/csrc/bc_inflate.h"

struct Block {
  uint64_t src_off, dst_off;
  uint32_t src_len, isize, crc32, pad;
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t head[3];
  if (fread(head, 8, 3, f) != 3) return 2;
  const uint64_t n = head[0], src_bytes = head[1], dst_bytes = head[2];
  std::vector<Block> blocks(n);
  if (n && fread(blocks.data(), sizeof(Block), n, f) != n) return 2;
  std::vector<uint8_t> src(src_bytes);
  if (src_bytes && fread(src.data(), 1, src_bytes, f) != src_bytes) return 2;
  fclose(f);

  uint32_t crc_tab[256];
  for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = bc::crc32_table_entry(i);
  std::vector<uint8_t> dst(dst_bytes, 0xAA);
  std::vector<uint32_t> status(n, 0);
  bc::InflateTables* T = new bc::InflateTables;
  for (uint64_t i = 0; i < n; ++i) {
    const Block& b = blocks[i];
    if (b.src_off > src_bytes || b.src_len > src_bytes - b.src_off || b.dst_off > dst_bytes || b.isize > dst_bytes - b.dst_off) return 2;
    uint8_t* in = (uint8_t*)malloc(b.src_len ? b.src_len : 1);
    uint8_t* out = (uint8_t*)malloc(b.isize ? b.isize : 1);
    memcpy(in, src.data() + b.src_off, b.src_len);
    memset(out, 0xAA, b.isize ? b.isize : 1);
    memset(T, 0xEE, sizeof *T);  // (the decoder may not depend on what an earlier block left in the tables)
    status[i] = bc::inflate_member(in, b.src_len, out, b.isize, b.crc32, *T, crc_tab, 0);
    memcpy(dst.data() + b.dst_off, out, b.isize);
    free(in);
    free(out);
  }
  delete T;
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  if (n) fwrite(status.data(), 4, n, f);
  if (dst_bytes) fwrite(dst.data(), 1, dst_bytes, f);
  fclose(f);
  return 0;
}
