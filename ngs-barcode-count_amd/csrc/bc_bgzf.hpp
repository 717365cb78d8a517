// bc_bgzf.hpp -- BGZF block index and the launch of the device inflater, shared by bc_inflate.hip and bc_ingest.hip;
// and what bc_bam.hip offers the ingest: the BAM header on the host, the record framing and the gather on the device.
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

// ---- BAM: the framing kernels of bc_bam.hip, for the ingest ----

// what the device reports per framed text
struct BamStats {
  unsigned long long n_cand;   // offsets that pass the header filter
  unsigned long long n_rec;    // records handed on
  unsigned long long end_pos;  // just past the chain's last whole record (= start when there is none)
  long long start;             // offset of the chain's first record; < 0: the overlap was too short
  unsigned int min_len, max_len;  // l_seq over the records handed on
  unsigned int status;         // kBam* of bc_bam.h
  unsigned int pad;
};
// where the record table goes: the three arrays of bc_bam_frame_device, or the ingest's four (each set may be null)
struct BamTables {
  uint32_t *rec_at, *rec_len, *rec_flag;
  uint32_t *seq_at, *qual_at;  // seq_at: bit 31 is the record's reverse-strand flag
  uint16_t *lens, *qlens;
};
// the device buffers a framing works in
struct BamWork {
  uint32_t* cand;      // cap words: candidate offsets
  uint32_t* link;      // cap words
  uint32_t* mark;      // cap words
  uint32_t* jump;      // levels * cap words
  uint32_t* blk_cnt;   // bam_count_blocks(len, cap) words each
  uint32_t* blk_off;
  uint32_t cap, levels;
};
uint32_t bam_levels(uint32_t cap);  // jump-pointer levels that any chain among `cap` candidates needs
size_t bam_count_blocks(uint64_t len_max, uint32_t cap);
// Enqueues the framing of text[0, len) (16-byte aligned) on `stream`.  The chain starts at *d_next_off - buf_file_off,
// or at `start` when d_next_off is null.  Records with one of the `skip_flags` set are left out.  Returns a hipError_t
// as int.
int bam_frame_launch(void* stream, const uint8_t* d_text, uint64_t len, uint32_t n_ref, const unsigned long long* d_next_off,
                     unsigned long long buf_file_off, long long start, uint32_t skip_flags, const BamWork& work, const BamTables& out,
                     BamStats* d_stats);
// records [first, first + n) of the ingest's table -> the fixed-stride batch
int bam_gather_launch(void* stream, const uint8_t* d_text, const uint32_t* d_seq_at, const uint32_t* d_qual_at, const uint16_t* d_lens,
                      uint64_t first, uint64_t n, uint32_t stride, uint8_t* d_out_seq, uint8_t* d_out_qual);
// The header of a BAM file through zlib on the host: how many references its dictionary has and where, in the
// inflated stream, the first record starts.  false: *why says what is wrong with it.
bool bam_header(int fd, const std::vector<BgzfMember>& members, uint64_t inflated, uint32_t* n_ref, uint64_t* first_record,
                std::string* why);

}  // namespace bc
