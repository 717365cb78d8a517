// bc_bgzf.hpp -- BGZF block index and the launch of the device inflater, shared by bc_inflate.hip and bc_ingest.hip.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/barcode_count_hip.h"

namespace bc {

struct BgzfMember {
  uint64_t file_off;     // where the member starts in the file
  uint64_t out_off;      // where its text starts in the inflated stream
  uint32_t total;        // BSIZE + 1: bytes of the member
  uint32_t payload_off;  // from file_off to the deflate stream
  uint32_t payload_len;
  uint32_t isize, crc32;
};

// Walks the member headers.  0: BGZF through and through; 1: not BGZF (*why says where the chain broke);
// -1: the file cannot be read.
int bgzf_index(const std::string& path, std::vector<BgzfMember>* members, uint64_t* inflated_bytes, std::string* why);

// One member's text through zlib on the host (ISIZE and CRC32 checked); false when the member is damaged.
bool bgzf_inflate_host(int fd, const BgzfMember& m, std::vector<uint8_t>* text);

// Bytes [off, off + n) of the inflated stream through zlib on the host, the members around them only.  Returns the
// bytes delivered (fewer than n at the stream's end), -1 on a read error or a damaged member.
struct BgzfHostReader {
  int fd = -1;
  const std::vector<BgzfMember>* members = nullptr;
  uint64_t inflated = 0;
  size_t cached = (size_t)-1;  // the member whose text is in `text`
  std::vector<uint8_t> text;
  long read_at(char* dst, size_t n, unsigned long long off);
};

// Enqueues the inflate kernel on `stream`: d_blocks[0, n_blocks) is the table on the device (ranges already checked
// by the caller), d_status gets one word per block.  Returns a hipError_t as int.
int bgzf_inflate_launch(void* stream, const void* d_src, const bc_bgzf_block* d_blocks, uint64_t n_blocks, void* d_dst,
                        uint32_t* d_status);
// d_text[at] = '\n' on `stream` (the gz rule for an unterminated last character)
int bgzf_patch_newline_launch(void* stream, void* d_text, uint64_t at);

const char* bgzf_status_name(uint32_t status);

// BGZF blocks inflated on the device for this engine (bc_engine.hip)
void engine_add_gz_blocks(bc_engine* e, uint64_t n);

// bc_gunzip_span_device (bc_gunzip.hip), for the ingest.  history_bytes: how many of the 32 KiB at d_history are the
// member's own text (the last ones): a distance that reaches before them is kInfBadSymbol.
int gunzip_span(int device_id, void* hip_stream, const void* d_src, uint64_t src_bytes, uint64_t start_bit, const void* d_history,
                uint32_t history_bytes, void* d_text, uint64_t text_capacity, uint32_t part_bytes, bc_gunzip_result* res);
// segments of ordinary gzip streams inflated on the device for this engine (bc_engine.hip)
void engine_add_gz_segments(bc_engine* e, uint64_t n);

}  // namespace bc
