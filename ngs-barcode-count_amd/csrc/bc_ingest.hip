// bc_ingest.hip -- FASTQ ingest for the engine.
//
// Replaces the reference's reader thread (input::read_fastq + FastqLineReader, input.rs:24-149): same 4-line
// framing, same "Total sequences" accounting (with its quirks), same first-record sanity check
// (RawSequenceRead::check_fastq_format, parse.rs:377-427).  The reference pushes one packed String per read onto a
// mutex-guarded VecDeque; here the host only MOVES bytes and the device does the framing:
//
//   host     a reader team pread()s the file (page cache -> pinned chunk buffers, several threads; zlib for .gz,
//            unless the file is BGZF: then the compressed bytes travel and the device inflates them, bc_inflate.hip;
//            with BC_GZ_DEVICE=all the same holds for an ordinary gzip stream, span by span, bc_gunzip.hip),
//   PCIe     the raw text goes to the device as it is (hipMemcpyAsync on the ingest stream),
//   device   newline scan (count, prefix sum, positions), record table (where each record's sequence and quality
//            line start, how long they are), then a gather into the fixed-stride sequence / quality batch the match
//            kernel reads -- bc_engine_submit_device[_q] on the engine's stream.
//
// Chunks are arbitrary byte ranges of the file.  A record that straddles two chunks is finished in the second: the
// device keeps the file offset of the first unframed byte, and every device text buffer starts with a copy of the
// previous chunk's last kOverlap bytes (device to device), so the second chunk sees the whole record.
// Three slots rotate: while the device frames and counts chunk i, the team reads chunk i+1 and chunk i-1's batch may
// still be in the match kernel.
//
// A *.bam file (unaligned BAM) is a BGZF container of binary, length-prefixed records: it takes the BGZF way to the
// device, and there the framing kernels of bc_bam.hip stand in for the newline scan and the gather (they find the chain
// of records from the first unframed byte on, skip secondary and supplementary records, and unpack nibbles and Phred
// bytes into the same batch).  Every whole record is one read; none of the .gz quirks apply.  With several shards a BAM
// file goes to shard 0 whole and the others get nothing: record-aligned BAM shards are not built.
//
// Which of five input paths a file takes (InputPath) is decided once per call.  A producer thread fills the slots through
// one of three Producers (plain / zlib reader, BGZF blocks, gzip spans on the device); the calling thread frames each
// chunk, counts the one before it, and applies the end-of-stream rules.  What decides counts without a GPU -- the
// first-record check, those rules, the gzip member header, the cut of a BGZF index into chunks and shards -- lives in
// bc_fastq_host.hpp; the kernels in bc_ingest_kernels.h.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/barcode_count_hip.h"
#include "bc_bam.h"
#include "bc_bgzf.hpp"
#include "bc_fastq_host.hpp"
#include "bc_ingest_kernels.h"
#include "bc_plan.hpp"

using namespace bc;

namespace {

constexpr size_t kOverlap = 4u << 20;  // longest record tail that may be carried into the next chunk
constexpr int kSlots = 3;

#define HIP_TRY(expr)                                                     \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) {                                               \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));       \
      return BC_ERR_HIP;                                                  \
    }                                                                     \
  } while (0)

struct Slot {
  uint8_t* pin = nullptr;       // [kOverlap headroom unused on the host | chunk bytes]
  uint8_t* d_text = nullptr;    // [kOverlap | chunk bytes]
  uint32_t* d_blk_cnt = nullptr;
  uint32_t* d_blk_off = nullptr;
  uint32_t* d_nl_pos = nullptr;
  uint32_t* d_seq_at = nullptr;
  uint32_t* d_qual_at = nullptr;
  uint16_t* d_lens = nullptr;
  uint16_t* d_qlens = nullptr;
  uint8_t* d_out_seq = nullptr;
  uint8_t* d_out_qual = nullptr;
  ChunkStats* stats = nullptr;  // pinned host
  ChunkStats* d_stats = nullptr;
  hipEvent_t uploaded = nullptr;   // the pinned text may be overwritten
  hipEvent_t framed = nullptr;     // the stats have arrived on the host
  hipEvent_t gathered = nullptr;   // the batch arrays are complete (ingest stream)
  hipEvent_t consumed = nullptr;   // the match kernel has read the batch arrays (engine stream)
  // BGZF chunks: `pin` holds the compressed bytes of blocks [first_blk, first_blk + nblk) of the file's index, the
  // inflate kernel writes their text behind the overlap of d_text
  uint8_t* d_comp = nullptr;
  BamStats* d_bam_stats = nullptr;     // BAM: what the framing of bc_bam.hip reports (ingest_from_bam_kernel hands it on)
  bc_bgzf_block* blk_tab = nullptr;    // pinned host
  bc_bgzf_block* d_blk_tab = nullptr;
  uint32_t* blk_status = nullptr;      // pinned host
  uint32_t* d_blk_status = nullptr;
  size_t clen = 0, nblk = 0, first_blk = 0;
  long long patch_at = -1;         // text offset of the stream's unterminated last character (it becomes '\n'), or -1
  size_t len = 0;                  // text bytes of the chunk held now
  size_t ov = 0;                   // bytes of overlap in front of them on the device
  unsigned long long file_off = 0; // file offset of the chunk's first byte
  bool eof = false;
};

struct Ingest {
  bc_engine* engine = nullptr;
  hipStream_t st = nullptr, engine_stream = nullptr;
  size_t chunk = 0, out_cap = 0;
  uint64_t line_cap = 0, rec_cap = 0;
  uint32_t n_blk_cap = 0;
  Slot slot[kSlots];
  DevState* d_state = nullptr;
  InputPath kind = InputPath::Plain;  // this call's
  // GzipDevice: the producer thread inflates span after span into the slot's text buffer on a stream of its own, and
  // copies the overlap itself (a span's history is the 32 KiB in front of its text)
  hipStream_t st_gz = nullptr;
  uint8_t* gz_pin = nullptr;       // pinned: the compressed bytes not yet inflated, from the current block boundary on
  uint8_t* d_gz_comp = nullptr;
  size_t comp_cap = 0;
  std::vector<uint8_t> gz_head;    // the stream's first text, for the first-record check
  size_t blk_cap = 0;              // blocks per chunk the BGZF buffers hold (0: not allocated yet)
  const std::vector<BgzfMember>* members = nullptr;
  std::string path;
  uint64_t blocks_inflated = 0;    // this call
  uint32_t stride = 0, ragged_stride = 0;
  // BAM: the dictionary's size (a record's refID lies below it), the candidates one text may hold (a record has at least
  // 37 bytes: an eighth more than the text can hold real ones), and the jump pointers, one set for all slots (a chunk's
  // framing is over before the next one's begins: both are on `st`); some twenty levels of one word per candidate, 0.4 GB
  // for chunks of 128 MiB
  uint32_t n_ref = 0, bam_cap = 0, bam_levels_n = 0;
  uint32_t* d_bam_jump = nullptr;

  int alloc_bam() {
    if (d_bam_jump) return BC_OK;
    bam_cap = (uint32_t)((kOverlap + chunk) / 32);
    bam_levels_n = bam_levels(bam_cap);
    for (Slot& s : slot) HIP_TRY(hipMalloc((void**)&s.d_bam_stats, sizeof(BamStats)));
    HIP_TRY(hipMalloc((void**)&d_bam_jump, (size_t)bam_cap * bam_levels_n * sizeof(uint32_t)));
    return BC_OK;
  }

  // the buffers only BGZF input needs, made at the first such call
  int alloc_bgzf() {
    if (blk_cap) return BC_OK;
    const size_t cap = chunk / 256 + 64;
    for (Slot& s : slot) {
      HIP_TRY(hipMalloc((void**)&s.d_comp, chunk + 16));
      HIP_TRY(hipHostMalloc((void**)&s.blk_tab, cap * sizeof(bc_bgzf_block), hipHostMallocDefault));
      HIP_TRY(hipMalloc((void**)&s.d_blk_tab, cap * sizeof(bc_bgzf_block)));
      HIP_TRY(hipHostMalloc((void**)&s.blk_status, cap * sizeof(uint32_t), hipHostMallocDefault));
      HIP_TRY(hipMalloc((void**)&s.d_blk_status, cap * sizeof(uint32_t)));
    }
    blk_cap = cap;
    return BC_OK;
  }

  int alloc_gzdev(size_t cap) {
    if (comp_cap >= cap) return BC_OK;
    if (gz_pin) (void)hipHostFree(gz_pin);
    if (d_gz_comp) (void)hipFree(d_gz_comp);
    gz_pin = d_gz_comp = nullptr;
    comp_cap = 0;
    if (!st_gz) HIP_TRY(hipStreamCreateWithFlags(&st_gz, hipStreamNonBlocking));
    HIP_TRY(hipHostMalloc((void**)&gz_pin, cap, hipHostMallocDefault));
    HIP_TRY(hipMalloc((void**)&d_gz_comp, cap + 64));
    comp_cap = cap;
    return BC_OK;
  }

  // a new call on these buffers
  void begin_call(bc_engine* e, InputPath k, const std::vector<BgzfMember>* index, const std::string& file) {
    engine = e;
    engine_stream = (hipStream_t)bc_engine_hip_stream(e);
    kind = k;
    members = index;
    path = file;
    gz_head.clear();
    blocks_inflated = 0;
    stride = ragged_stride = 0;
    for (Slot& sl : slot) {
      sl.len = sl.ov = 0;
      sl.file_off = 0;
      sl.eof = false;
      sl.clen = sl.nblk = sl.first_blk = 0;
      sl.patch_at = -1;
    }
  }

  // the device state of a new call: nothing framed yet, or (a BGZF shard) the framing starts at the shard's first record
  int set_start(unsigned long long text_a) {
    if (hipMemsetAsync(d_state, 0, sizeof(DevState), st) != hipSuccess) {
      set_error("bc_fastq_count: hipMemsetAsync failed");
      return BC_ERR_HIP;
    }
    const DevState first{text_a};
    if (text_a && (hipMemcpyAsync(d_state, &first, sizeof first, hipMemcpyHostToDevice, st) != hipSuccess ||
                   hipStreamSynchronize(st) != hipSuccess)) {
      set_error("bc_fastq_count: setting the shard's start failed");
      return BC_ERR_HIP;
    }
    return BC_OK;
  }

  int alloc() {
    n_blk_cap = (uint32_t)((kOverlap + chunk + kScanBlock - 1) / kScanBlock);
    line_cap = (kOverlap + chunk) / 2;
    rec_cap = line_cap / 4;
    out_cap = 2 * (kOverlap + chunk);
    HIP_TRY(hipMalloc((void**)&d_state, sizeof(DevState)));
    HIP_TRY(hipMemset(d_state, 0, sizeof(DevState)));
    for (Slot& s : slot) {
      HIP_TRY(hipHostMalloc((void**)&s.pin, chunk + 16, hipHostMallocDefault));
      HIP_TRY(hipHostMalloc((void**)&s.stats, sizeof(ChunkStats), hipHostMallocDefault));
      HIP_TRY(hipMalloc((void**)&s.d_stats, sizeof(ChunkStats)));
      HIP_TRY(hipMalloc((void**)&s.d_text, kOverlap + chunk + 64));
      HIP_TRY(hipMalloc((void**)&s.d_blk_cnt, (size_t)n_blk_cap * 4));
      HIP_TRY(hipMalloc((void**)&s.d_blk_off, (size_t)n_blk_cap * 4));
      HIP_TRY(hipMalloc((void**)&s.d_nl_pos, line_cap * 4));
      HIP_TRY(hipMalloc((void**)&s.d_seq_at, rec_cap * 4));
      HIP_TRY(hipMalloc((void**)&s.d_qual_at, rec_cap * 4));
      HIP_TRY(hipMalloc((void**)&s.d_lens, rec_cap * 2));
      HIP_TRY(hipMalloc((void**)&s.d_qlens, rec_cap * 2));
      HIP_TRY(hipMalloc((void**)&s.d_out_seq, out_cap));
      HIP_TRY(hipMalloc((void**)&s.d_out_qual, out_cap));
      HIP_TRY(hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&s.framed, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&s.gathered, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming));
    }
    return BC_OK;
  }

  void release() {
    for (Slot& s : slot) {
      if (s.pin) (void)hipHostFree(s.pin);
      if (s.stats) (void)hipHostFree(s.stats);
      if (s.blk_tab) (void)hipHostFree(s.blk_tab);
      if (s.blk_status) (void)hipHostFree(s.blk_status);
      void* dev[] = {s.d_stats, s.d_text, s.d_blk_cnt, s.d_blk_off, s.d_nl_pos, s.d_seq_at, s.d_qual_at, s.d_lens, s.d_qlens,
                     s.d_out_seq, s.d_out_qual, s.d_comp, s.d_blk_tab, s.d_blk_status, s.d_bam_stats};
      for (void* p : dev)
        if (p) (void)hipFree(p);
      for (hipEvent_t ev : {s.uploaded, s.framed, s.gathered, s.consumed})
        if (ev) (void)hipEventDestroy(ev);
    }
    if (d_state) (void)hipFree(d_state);
    if (d_bam_jump) (void)hipFree(d_bam_jump);
    if (gz_pin) (void)hipHostFree(gz_pin);
    if (d_gz_comp) (void)hipFree(d_gz_comp);
    if (st_gz) (void)hipStreamDestroy(st_gz);
    if (st) (void)hipStreamDestroy(st);
  }

  // chunk in slot b (host side filled) -> device, framed; the stats travel back asynchronously
  int frame(int b, const Slot* prev) {
    Slot& s = slot[b];
    HIP_TRY(hipStreamWaitEvent(st, s.consumed, 0));  // the batch arrays of this slot may still be read by a match kernel
    if (kind == InputPath::GzipDevice) {
      // (the text and the overlap in front of it are in place: the producer put them there and waited for them)
    } else if (!bgzf_blocks(kind)) {
      HIP_TRY(hipMemcpyAsync(s.d_text + kOverlap, s.pin, s.len, hipMemcpyHostToDevice, st));
      HIP_TRY(hipEventRecord(s.uploaded, st));
    } else {
      const int rc = inflate(s);
      if (rc != BC_OK) return rc;
    }
    s.ov = 0;
    if (prev) {
      s.ov = std::min(kOverlap, prev->ov + prev->len);
      if (kind != InputPath::GzipDevice)
        hipLaunchKernelGGL(ingest_overlap_kernel, dim3((uint32_t)((s.ov + 255) / 256)), dim3(256), 0, st,
                           prev->d_text + kOverlap + prev->len, s.d_text + kOverlap, (uint32_t)s.ov);
    }
    const uint8_t* text = s.d_text + kOverlap - s.ov;  // 16-byte aligned: kOverlap and ov are multiples of 16 ...
    // ... unless the previous chunk was shorter than the overlap (only the file's first chunks can be): align down
    const size_t mis = (size_t)((uintptr_t)text & 15u);
    text -= mis;
    const unsigned long long buf_off = s.file_off - s.ov - mis;  // may wrap below zero only together with start >= mis
    const unsigned long long len = s.ov + mis + s.len;
    const uint32_t n_blk = (uint32_t)((len + kScanBlock - 1) / kScanBlock);
    if (kind == InputPath::BamDevice) {
      // the line-position array holds sixteen words per candidate: offsets, links and marks take three
      const BamWork work = {s.d_nl_pos, s.d_nl_pos + bam_cap, s.d_nl_pos + 2 * (size_t)bam_cap, d_bam_jump, s.d_blk_cnt, s.d_blk_off,
                            bam_cap, bam_levels_n};
      const BamTables out = {nullptr, nullptr, nullptr, s.d_seq_at, s.d_qual_at, s.d_lens, s.d_qlens};
      HIP_TRY((hipError_t)bam_frame_launch(st, text, len, n_ref, &d_state->next_off, buf_off, 0, 0x900u, work, out, s.d_bam_stats));
      hipLaunchKernelGGL(ingest_from_bam_kernel, dim3(1), dim3(1), 0, st, s.d_bam_stats, s.d_stats);
      return frame_end(b, text, len, buf_off);
    }
    hipLaunchKernelGGL(ingest_begin_kernel, dim3(1), dim3(1), 0, st, d_state, buf_off, len, s.d_stats, text);
    hipLaunchKernelGGL(ingest_count_kernel, dim3(n_blk), dim3(256), 0, st, text, len, s.d_stats, s.d_blk_cnt);
    hipLaunchKernelGGL(ingest_scan_kernel, dim3(1), dim3(1024), 0, st, s.d_blk_cnt, n_blk, s.d_blk_off, s.d_stats, line_cap);
    hipLaunchKernelGGL(ingest_positions_kernel, dim3(n_blk), dim3(256), 0, st, text, len, s.d_stats, s.d_blk_off, s.d_nl_pos,
                       line_cap);
    // the record kernel is sized for the most records the text can hold (a record has at least four bytes)
    const unsigned long long rec_max = std::min<unsigned long long>(rec_cap, len / 4 + 1);
    hipLaunchKernelGGL(ingest_records_kernel, dim3((uint32_t)((rec_max + 255) / 256)), dim3(256), 0, st, text, s.d_nl_pos,
                       s.d_stats, gz_line_rules(kind) ? 0 : 1, s.d_seq_at, s.d_qual_at, s.d_lens, s.d_qlens);
    return frame_end(b, text, len, buf_off);
  }
  // the framing's last steps: the device state moves on, the stats travel back
  int frame_end(int b, const uint8_t* text, unsigned long long len, unsigned long long buf_off) {
    Slot& s = slot[b];
    hipLaunchKernelGGL(ingest_advance_kernel, dim3(1), dim3(1), 0, st, d_state, s.d_stats, buf_off);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s.stats, s.d_stats, sizeof(ChunkStats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(s.framed, st));
    s_text[b] = text;
    s_text_len[b] = len;
    return BC_OK;
  }
  // BGZF: compressed bytes and block table -> device, one wavefront inflates one block into the slot's text buffer, the
  // statuses travel back with the chunk's stats
  int inflate(Slot& s) {
    HIP_TRY(hipMemcpyAsync(s.d_comp, s.pin, s.clen, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s.d_blk_tab, s.blk_tab, s.nblk * sizeof(bc_bgzf_block), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(s.uploaded, st));
    HIP_TRY((hipError_t)bgzf_inflate_launch(st, s.d_comp, s.d_blk_tab, s.nblk, s.d_text + kOverlap, s.d_blk_status));
    if (s.patch_at >= 0) HIP_TRY((hipError_t)bgzf_patch_newline_launch(st, s.d_text + kOverlap, (uint64_t)s.patch_at));
    HIP_TRY(hipMemcpyAsync(s.blk_status, s.d_blk_status, s.nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return BC_OK;
  }
  // blocks that hold no text (EOF markers) in a chunk of their own: inflated and checked, nothing to frame
  int inflate_only(int b) {
    Slot& s = slot[b];
    const int rc = inflate(s);
    if (rc != BC_OK) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return check_blocks(s);
  }
  // the statuses of a chunk's blocks (they have arrived): a damaged block ends the call
  int check_blocks(const Slot& s) {
    for (size_t k = 0; k < s.nblk; ++k) {
      if (s.blk_status[k] == 0) continue;
      set_error("read error in " + path + ": BGZF block at file offset " +
                std::to_string((unsigned long long)(*members)[s.first_blk + k].file_off) + ": " + bgzf_status_name(s.blk_status[k]));
      return BC_ERR_INVALID;
    }
    blocks_inflated += s.nblk;
    engine_add_gz_blocks(engine, s.nblk);
    return BC_OK;
  }
  const uint8_t* s_text[kSlots] = {nullptr, nullptr, nullptr};
  unsigned long long s_text_len[kSlots] = {0, 0, 0};  // bytes of the framed text behind s_text

  // the framed chunk of slot b -> batches for the engine
  int submit(int b, uint64_t* n_rec_out) {
    Slot& s = slot[b];
    HIP_TRY(hipEventSynchronize(s.framed));
    const ChunkStats cs = *s.stats;
    *n_rec_out = 0;
    if (bgzf_blocks(kind)) {
      const int rc = check_blocks(s);
      if (rc != BC_OK) return rc;
    }
    if (cs.start < 0) {
      set_error("a FASTQ record is longer than 4 MiB");
      return BC_ERR_INVALID;
    }
    if (kind == InputPath::BamDevice && cs.pad != kBamOk) {  // (the framing's status)
      const std::string at = " (inflated offset " + std::to_string(s.file_off - s.ov + cs.end_pos - (s_text_len[b] - s.ov - s.len)) + ")";
      if (cs.pad == kBamBroken) {
        set_error("read error in " + path + ": the chain of BAM records breaks" + at + ": what follows a record is no record header");
        return BC_ERR_INVALID;
      }
      set_error(cs.pad == kBamTooLong ? "a BAM record of " + path + " is longer than 4 MiB" + at + " (not supported by the engine)"
                                      : "a chunk of " + path + " holds more BAM record headers, real or apparent, than the engine frames");
      return BC_ERR_UNSUPPORTED;
    }
    if (cs.n_rec == 0) return BC_OK;
    if (cs.n_lines >= line_cap) {
      set_error("FASTQ text with lines of under two bytes on average: not supported by the engine");
      return BC_ERR_UNSUPPORTED;
    }
    if (cs.max_len > 65535u || cs.max_qlen > 65535u) {
      set_error("a FASTQ line is longer than 65535 bytes (not supported by the engine)");
      return BC_ERR_UNSUPPORTED;
    }
    const uint32_t want = std::max<uint32_t>(4u, (cs.max_len + 3u) & ~3u);
    const bool uniform = cs.min_len == cs.max_len && !cs.qual_differs;
    // fixed-length chunks get exactly their stride (the kernel is specialised for the shape); ragged ones keep the
    // widest stride seen so far, so that a file of varying lengths settles on one kernel shape
    if (!uniform) ragged_stride = std::max(ragged_stride, want);
    stride = uniform ? want : ragged_stride;
    // the batch arrays hold out_cap bytes: a chunk whose stride is far above its average line goes in several parts
    const uint64_t per = std::max<uint64_t>(256, (out_cap / stride) & ~255ull);
    for (uint64_t first = 0; first < cs.n_rec; first += per) {
      const uint64_t n = std::min<uint64_t>(per, cs.n_rec - first);
      if (first) HIP_TRY(hipStreamWaitEvent(st, s.consumed, 0));  // the previous part's kernel still reads the arrays
      if (kind == InputPath::BamDevice)
        HIP_TRY((hipError_t)bam_gather_launch(st, s_text[b], s.d_seq_at, s.d_qual_at, s.d_lens, first, n, stride, s.d_out_seq, s.d_out_qual));
      else
        hipLaunchKernelGGL(ingest_gather_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, st, s_text[b], s.d_seq_at, s.d_qual_at,
                           s.d_lens, s.d_qlens, first, n, stride, s.d_out_seq, s.d_out_qual);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(s.gathered, st));
      HIP_TRY(hipStreamWaitEvent(engine_stream, s.gathered, 0));
      int rc;
      if (uniform)
        rc = bc_engine_submit_device(engine, s.d_out_seq, s.d_out_qual, nullptr, stride, cs.max_len, n);
      else if (!cs.qual_differs)
        rc = bc_engine_submit_device(engine, s.d_out_seq, s.d_out_qual, s.d_lens + first, stride, stride, n);
      else
        rc = bc_engine_submit_device_q(engine, s.d_out_seq, s.d_out_qual, s.d_lens + first, s.d_qlens + first, stride, n);
      if (rc != BC_OK) return rc;
      HIP_TRY(hipEventRecord(s.consumed, engine_stream));
    }
    *n_rec_out = cs.n_rec;
    return BC_OK;
  }
};

// what a plain or zlib reader needs (the device paths use `fd` and read_span only)
struct Source {
  gzFile zf = nullptr;  // InputPath::Zlib: the stream; every other path reads `fd`
  int fd = -1;
  bool zlib() const { return zf != nullptr; }  // this source reads through gzread (set by open(), from the InputPath)
  unsigned long long pos = 0;  // next byte to read (plain files)
  unsigned long long size = 0; // plain files
  unsigned threads = 4;
  bool open(const std::string& path, InputPath kind) {
    if (kind != InputPath::Zlib) return (fd = ::open(path.c_str(), O_RDONLY)) >= 0;
    zf = gzopen(path.c_str(), "rb");  // multi-member aware (flate2 MultiGzDecoder, input.rs:63)
    if (zf) gzbuffer(zf, 4 << 20);
    return zf != nullptr;
  }
  void close() {
    if (zlib()) gzclose(zf);
    if (fd >= 0) ::close(fd);
    zf = nullptr;
    fd = -1;
  }
  // nothing left after what fill() has returned so far
  bool at_end() {
    if (!zlib()) return pos >= size;
    const int c = gzgetc(zf);
    if (c < 0) return true;
    gzungetc(c, zf);
    return false;
  }
  // fills dst with up to cap bytes; returns the count (0 at end of file), -1 on error
  long fill(uint8_t* dst, size_t cap) {
    if (zlib()) {
      size_t got = 0;
      while (got < cap) {
        const int n = gzread(zf, dst + got, (unsigned)std::min<size_t>(cap - got, 1u << 30));
        if (n < 0) return -1;
        if (n == 0) break;
        got += (size_t)n;
      }
      return (long)got;
    }
    // (size = where this reader's share of the file ends: the file's end, or the shard's)
    if (pos >= size) return 0;
    cap = (size_t)std::min<unsigned long long>(cap, size - pos);
    const long total = read_span(dst, pos, cap);
    if (total > 0) pos += (unsigned long long)total;
    return total;
  }
  // bytes [pos, pos + cap) of the file, as many as there are; -1 on error
  long read_span(uint8_t* dst, unsigned long long pos, size_t cap) {
    if (cap == 0) return 0;
    // page cache -> pinned memory, one slice per thread
    const size_t slice = (((cap + threads - 1) / threads) + 4095) & ~(size_t)4095;  // (never 0: cap may be a few bytes)
    std::vector<long> got(threads, 0);
    std::vector<std::thread> team;
    auto work = [&](unsigned t) {
      const size_t a = std::min(cap, (size_t)t * slice), b = std::min(cap, a + slice);
      size_t done = 0;
      while (a + done < b) {
        const ssize_t n = pread(fd, dst + a + done, b - a - done, (off_t)(pos + a + done));
        if (n < 0) {
          got[t] = -1;
          return;
        }
        if (n == 0) break;
        done += (size_t)n;
      }
      got[t] = (long)done;
    };
    for (unsigned t = 1; t < threads; ++t) team.emplace_back(work, t);
    work(0);
    for (auto& th : team) th.join();
    size_t total = 0;
    for (unsigned t = 0; t < threads; ++t) {
      if (got[t] < 0) return -1;
      total += (size_t)got[t];
      if ((size_t)got[t] < std::min(cap, (size_t)(t + 1) * slice) - std::min(cap, (size_t)t * slice)) break;  // end of file inside this slice
    }
    return (long)total;
  }
};

// (a BGZF block holds at most 64 KiB of text: fetching by the block keeps the host inflate to the blocks around `off`)
long long gz_record_start_at_or_after(BgzfHostReader& hr, unsigned long long off) {
  return record_start_at_or_after([&hr](char* dst, size_t n, unsigned long long at) { return hr.read_at(dst, n, at); }, off,
                                  hr.inflated, 64u << 10);
}

// What a producer put into a slot: the chunk's text (or, for BGZF, the compressed blocks that hold it), where it sits
// in the file, whether the stream ends with it -- or why there is no chunk.
struct Filled {
  size_t len = 0, clen = 0, nblk = 0, first_blk = 0;
  long long patch_at = -1;
  unsigned long long file_off = 0;
  bool eof = false;
  int error_code = BC_OK;
  std::string error;
  int fail(int code, const std::string& what) {
    len = nblk = 0;
    eof = true;
    error = what;
    return error_code = code;
  }
};

// Fills slot s with chunk i of the stream, once the consumer has released the slot; returns out->error_code.
struct Producer {
  virtual ~Producer() = default;
  virtual int next(int i, Slot& s, Filled* out) = 0;
};

// What the producer thread and the consumer share.  The producer fills chunk i into slot i % kSlots once i < released_upto
// and says so by filled_upto; the consumer frames it and, once the chunk before it is counted, releases that one's slot.
struct Handoff {
  std::mutex mu;
  std::condition_variable cv;
  int filled_upto = 0;         // chunks [0, filled_upto) are in their slots
  int released_upto = kSlots;  // the producer may fill chunks [.., released_upto)
  bool stop = false;
  int rc = BC_OK;              // what the producer found wrong (it becomes the call's error)
  std::string error;
};

// The producer thread: wait for the slot's release, fill it, publish the chunk (or the error) under the mutex, notify; ends
// with the stream, on an error, or when told to stop.
void produce(Producer& producer, Slot* slots, Handoff& h) {
  for (int i = 0;; ++i) {
    {
      std::unique_lock<std::mutex> lk(h.mu);
      h.cv.wait(lk, [&] { return h.stop || i < h.released_upto; });
      if (h.stop) return;
    }
    Slot& s = slots[i % kSlots];
    Filled f;
    producer.next(i, s, &f);
    {
      std::lock_guard<std::mutex> lk(h.mu);
      if (f.error_code != BC_OK) {
        h.rc = f.error_code;
        h.error = f.error;
      }
      s.len = f.len;
      s.clen = f.clen;
      s.nblk = f.nblk;
      s.first_blk = f.first_blk;
      s.patch_at = f.patch_at;
      s.file_off = f.file_off;
      s.eof = f.eof;
      h.filled_upto = i + 1;
    }
    h.cv.notify_all();
    if (f.eof) return;  // end of the stream (or error)
  }
}

// plain files (a reader team) and zlib streams: text into the pinned buffer
struct ReaderProducer : Producer {
  Source& src;
  const size_t chunk;
  const std::string& path;
  unsigned long long off = 0;
  ReaderProducer(Source& source, size_t chunk_bytes, const std::string& file) : src(source), chunk(chunk_bytes), path(file) {}
  int next(int, Slot& s, Filled* f) override {
    (void)hipEventSynchronize(s.uploaded);  // the slot's previous text has left for the device
    const long n = src.fill(s.pin, chunk);
    if (n < 0) return f->fail(BC_ERR_INVALID, "read error in " + path);
    f->len = (size_t)n;
    f->file_off = off;
    f->eof = n == 0 || (size_t)n < chunk || src.at_end();
    off += (unsigned long long)n;
    return BC_OK;
  }
};

// Blocks [first_member, end_member) of a BGZF file's index, the shard's share: run after run of whole blocks, their
// compressed bytes into the pinned buffer and their table beside it (Ingest::inflate takes it from there).
struct BgzfProducer : Producer {
  Source& src;
  const std::vector<BgzfMember>& members;
  const std::string& path;
  size_t fill_cap = 0, chunk = 0, blk_cap = 0;
  size_t first_member = 0, end_member = 0;
  unsigned long long text_b = 0;          // where the shard's text ends in the inflated stream
  bool patch_last = false;                // the stream's unterminated last character becomes '\n' ...
  size_t last_text_member = (size_t)-1;   // ... in this block, the file's last that holds text
  BgzfProducer(Source& source, const std::vector<BgzfMember>& index, const std::string& file) : src(source), members(index), path(file) {}
  int next(int, Slot& s, Filled* f) override {
    (void)hipEventSynchronize(s.uploaded);  // the slot's previous bytes have left for the device
    // the next run of blocks whose text fits the chunk (at least one block), their bytes read as one span
    const size_t from = first_member;
    const BgzfRun run = bgzf_next_run(members, from, end_member, fill_cap, chunk, blk_cap);
    const size_t upto = run.upto;
    const long n = upto > from ? src.read_span(s.pin, members[from].file_off, (size_t)run.comp_bytes) : 0;
    f->clen = (size_t)run.comp_bytes;
    f->first_blk = from;
    if (n < 0 || (unsigned long long)n != run.comp_bytes) return f->fail(BC_ERR_INVALID, "read error in " + path);
    const unsigned long long text_off = upto > from ? members[from].out_off : text_b;
    for (size_t k = from; k < upto; ++k) {
      const BgzfMember& m = members[k];
      bc_bgzf_block& t = s.blk_tab[k - from];
      t.src_off = m.file_off - members[from].file_off + m.payload_off;
      t.dst_off = m.out_off - text_off;
      t.src_len = m.payload_len;
      t.isize = m.isize;
      t.crc32 = m.crc32;
      if (patch_last && k == last_text_member) f->patch_at = (long long)(t.dst_off + m.isize - 1);
    }
    // (a shard that does not end the file stops at its last record's end, inside its last block)
    unsigned long long text = run.text_bytes;
    if (text_off + text > text_b) text = text_b > text_off ? text_b - text_off : 0;
    f->len = (size_t)text;
    f->nblk = upto - from;
    f->file_off = text_off;
    f->eof = upto >= end_member;
    first_member = upto;
    return BC_OK;
  }
};

struct GzDevStats {
  uint64_t spans = 0, segments = 0, rejected = 0, retries = 0;
};

// The gzip-device producer: compressed bytes from the file, member headers and trailers on the host, the deflate
// stream between them span by span through the device (bc_gunzip.hip).  What it keeps between chunks: the compressed
// bytes from the current block boundary on (pin[0, have), the boundary at bit `bit` of pin[0]) and the member's running
// CRC and length; and the overlap of the chunk before, which it copies in front of the slot's text itself.
struct GzDevProducer : Producer {
  Ingest* in = nullptr;
  unsigned long long off = 0;        // text bytes handed over so far
  size_t prev_ov = 0, prev_len = 0;  // the overlap of the chunk before, as Ingest::frame will work it out
  int fd = -1, device = 0;
  hipStream_t st = nullptr;
  uint8_t* pin = nullptr;
  uint8_t* d_comp = nullptr;
  size_t comp_cap = 0, span_bytes = 0;
  uint32_t part_bytes = 32768;
  std::string path, error;
  GzDevStats* stats = nullptr;
  unsigned long long fpos = 0;      // next file byte to read
  size_t have = 0;
  uint32_t bit = 0;
  bool file_end = false, in_member = false, any_member = false, stream_end = false;
  unsigned long long member_off = 0, member_len = 0;
  uint32_t member_crc = 0;

  unsigned long long pin_off() const { return fpos - have; }  // file offset of pin[0]
  int fail(const std::string& what, int code = BC_ERR_INVALID) {
    error = "read error in " + path + ": gzip member at file offset " + std::to_string(member_off) + ": " + what;
    return code;
  }
  // pin[0, want) from the file, as far as it goes
  int top_up(size_t want) {
    want = std::min(want, comp_cap);
    while (have < want && !file_end) {
      const ssize_t n = pread(fd, pin + have, want - have, (off_t)fpos);
      if (n < 0) return fail("pread failed");
      if (n == 0) file_end = true;
      have += (size_t)n;
      fpos += (unsigned long long)n;
    }
    return BC_OK;
  }
  void consume(size_t n) {
    memmove(pin, pin + n, have - n);
    have -= n;
  }
  long header() const { return gzip_member_header(pin, have, file_end); }

  int next(int i, Slot& s, Filled* f) override {
    // everything that reads this slot's text (its last chunk's framing and gather, the next chunk's overlap copy)
    // was enqueued before the slot was released
    bool ok = hipSetDevice(device) == hipSuccess && hipStreamSynchronize(in->st) == hipSuccess;
    const size_t ov = i > 0 ? std::min(kOverlap, prev_ov + prev_len) : 0;
    if (ok && ov) {
      const Slot& prev = in->slot[(i - 1) % kSlots];
      hipLaunchKernelGGL(ingest_overlap_kernel, dim3((uint32_t)((ov + 255) / 256)), dim3(256), 0, st, prev.d_text + kOverlap + prev_len,
                         s.d_text + kOverlap, (uint32_t)ov);
      ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) return f->fail(BC_ERR_HIP, "read error in " + path + ": the device refused the gzip stage");
    size_t text = 0;
    bool last = true, patched = false;
    const int rc = fill(s.d_text + kOverlap, in->chunk, &text, &last, &patched, i == 0 ? &in->gz_head : nullptr);
    if (rc != BC_OK) return f->fail(rc, error);
    f->len = text;
    f->patch_at = patched ? (long long)text - 1 : -1;
    f->file_off = off;
    f->eof = last;
    off += text;
    prev_ov = ov;
    prev_len = text;
    return BC_OK;
  }

  // Fills d_text[0, cap) with the stream's next text (behind it: the text before, at least 32 KiB of it unless the
  // stream is younger).  *last: the stream ends with this text; *patched: its unterminated last character became '\n'.
  int fill(uint8_t* d_text, size_t cap, size_t* text, bool* last, bool* patched, std::vector<uint8_t>* head) {
    size_t cur = 0, target = span_bytes;
    *last = *patched = false;
    while (!stream_end) {
      if (!in_member) {
        int rc = top_up(std::max<size_t>(target, 4096));
        if (rc != BC_OK) return rc;
        if (have == 0) {
          stream_end = true;
          break;
        }
        member_off = pin_off();
        long hb = header();
        if (hb == 0) {
          if ((rc = top_up(comp_cap)) != BC_OK) return rc;
          hb = header();
        }
        if (hb == -2) return fail("not deflate, or a header flag this program refuses", BC_ERR_UNSUPPORTED);
        if (hb <= 0) {
          if (!any_member) return fail("no gzip header");
          stream_end = true;  // (what follows the last member is ignored, as zlib's gzread does)
          break;
        }
        consume((size_t)hb);
        in_member = any_member = true;
        bit = 0;
        member_len = 0;
        member_crc = 0;
      }
      int rc = top_up(target);
      if (rc != BC_OK) return rc;
      size_t n = std::min(have, target);
      bc_gunzip_result res;
      for (int attempt = 0;; ++attempt) {
        if (hipMemcpyAsync(d_comp, pin, n, hipMemcpyHostToDevice, st) != hipSuccess) return fail("upload failed", BC_ERR_HIP);
        const void* hist = member_len ? d_text + cur - 32768 : nullptr;  // (in front of d_text lies the overlap: 4 MiB)
        const uint32_t hist_len = (uint32_t)std::min<unsigned long long>(member_len, 32768);  // the member's own text among them
        if (gunzip_span(device, st, d_comp, n, bit, hist, hist_len, d_text + cur, cap - cur, part_bytes, &res) != BC_OK)
          return fail("the device inflater failed", BC_ERR_HIP);
        ++stats->spans;
        stats->rejected += res.rejected;
        if (res.status != BC_GUNZIP_OUTPUT_FULL || res.text_bytes == 0 || attempt) break;
        n = (size_t)((res.end_bit + 7) / 8);  // the text does not fit: the span again, cut at the last boundary that does
        ++stats->retries;
      }
      if (res.status == BC_GUNZIP_BAD_STREAM) return fail(bgzf_status_name(res.detail));
      if (res.status == BC_GUNZIP_OUTPUT_FULL) {
        if (cur > 0 && res.text_bytes == 0) break;  // the chunk is full: the next one starts with this block
        // (a span cut at the boundary that fits measures as it did before the cut: it cannot be full again)
        if (res.text_bytes) return fail("internal error: a span cut at the boundary that fits is reported full again", BC_ERR_STATE);
        return fail("a single deflate block holds more text than the ingest's text buffer of " + std::to_string(cap) +
                        " bytes: raise BC_INGEST_CHUNK, or read this file through zlib with BC_GZ_DEVICE=1",
                    BC_ERR_UNSUPPORTED);
      }
      if (res.end_bit == bit && !res.member_end) {  // no whole block among the span's bytes
        if (n >= have && file_end) return fail("the stream ends inside a deflate block");
        if (n >= comp_cap)
          return fail("a single deflate block is larger than the ingest's buffers: raise BC_INGEST_CHUNK, or read this file through "
                      "zlib with BC_GZ_DEVICE=1", BC_ERR_UNSUPPORTED);
        target = std::min(comp_cap, 2 * target);
        continue;
      }
      target = span_bytes;
      stats->segments += res.segments;
      cur += (size_t)res.text_bytes;
      member_crc = (uint32_t)crc32_combine(member_crc, res.crc32, (z_off_t)res.text_bytes);
      member_len += res.text_bytes;
      consume((size_t)(res.end_bit >> 3));
      bit = (uint32_t)(res.end_bit & 7u);
      if (res.member_end) {
        if (bit) consume(1);
        bit = 0;
        if ((rc = top_up(std::max<size_t>(8, std::min(have, target)))) != BC_OK) return rc;
        if (have < 8) return fail("the file ends before the member's trailer");
        const uint32_t want_crc = (uint32_t)pin[0] | ((uint32_t)pin[1] << 8) | ((uint32_t)pin[2] << 16) | ((uint32_t)pin[3] << 24);
        const uint32_t want_len = (uint32_t)pin[4] | ((uint32_t)pin[5] << 8) | ((uint32_t)pin[6] << 16) | ((uint32_t)pin[7] << 24);
        if (want_crc != member_crc) return fail("CRC32 mismatch");
        if (want_len != (uint32_t)member_len) return fail("ISIZE mismatch");
        consume(8);
        in_member = false;
      }
    }
    if (head) {
      head->resize(std::min<size_t>(cur, 1u << 20));
      if (!head->empty() && hipMemcpyAsync(head->data(), d_text, head->size(), hipMemcpyDeviceToHost, st) != hipSuccess)
        return fail("reading the first text back failed", BC_ERR_HIP);
    }
    if (stream_end && cur) {  // the gz rule for an unterminated last character (see the caller)
      uint8_t c = '\n';
      if (hipMemcpyAsync(&c, d_text + cur - 1, 1, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail("reading the last character back failed", BC_ERR_HIP);
      if (c != '\n') {
        if (bgzf_patch_newline_launch(st, d_text, cur - 1) != (int)hipSuccess) return fail("patching the last character failed", BC_ERR_HIP);
        *patched = true;
      }
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail("the device refused the gzip stage", BC_ERR_HIP);
    *text = cur;
    *last = stream_end;
    return BC_OK;
  }
};

// What the environment asks for, read in one place (read_options, at the start of a call).
struct Options {
  enum class GzDevice { Never, Bgzf, All };  // BC_GZ_DEVICE: "0" | anything else, or unset | "all"
  GzDevice gz_device = GzDevice::Bgzf;
  bool verbose = false;   // BC_INGEST_VERBOSE
  unsigned threads = 4;   // BC_INGEST_THREADS: the reader team
  size_t chunk = 0;       // BC_INGEST_CHUNK (0: by the bytes ahead)
  size_t gz_span = 0;     // BC_GZ_SPAN_BYTES (0: an eighth of the chunk)
  size_t gz_part = 32768; // BC_GZ_PART_BYTES
};
// The buffer sizes of one call, from the options once the input path and the bytes ahead are known.
struct Sizes {
  size_t chunk;     // bytes per slot
  size_t fill_cap;  // text bytes per BGZF chunk
  size_t gz_span;   // compressed bytes per span of the gzip-device path
};
Sizes sizes_for(const Options& o, InputPath kind, unsigned long long bytes) {
  // chunk size: a multiple of 16 (the device reads the text 16 bytes at a time), no larger than the file needs;
  // BC_INGEST_CHUNK is for tests, which want records to straddle chunks in small files
  // (BGZF and BAM alike: one wavefront inflates one block, so a chunk should hold a few thousand blocks)
  size_t chunk = kind == InputPath::Plain || bgzf_blocks(kind) ? (size_t)std::min<unsigned long long>(128u << 20, ((bytes >> 20) + 1) << 20)
                                                               : (32u << 20);
  if (o.chunk) chunk = o.chunk;
  // (a deflate block's text has to fit the text buffer: zlib's blocks hold 16 Ki symbols, a few hundred KiB of FASTQ)
  if (kind == InputPath::GzipDevice) chunk = std::max<size_t>(chunk, 1u << 20);
  chunk = (chunk + 15) & ~(size_t)15;
  Sizes z = {chunk, chunk, o.gz_span ? o.gz_span : chunk / 8};
  // BGZF chunks are cut at block boundaries: text of at most `fill_cap` bytes, but always a whole block, so the
  // buffers hold at least the largest block there can be
  if (bgzf_blocks(kind)) z.chunk = std::max<size_t>(chunk, 65536 + 16);
  return z;
}

Options read_options() {
  Options o;
  if (const char* ev = getenv("BC_GZ_DEVICE"))
    o.gz_device = ev[0] == '0' && !ev[1] ? Options::GzDevice::Never : !strcmp(ev, "all") ? Options::GzDevice::All : Options::GzDevice::Bgzf;
  if (const char* ev = getenv("BC_INGEST_VERBOSE")) o.verbose = ev[0] && !(ev[0] == '0' && !ev[1]);
  o.threads = std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
  if (const char* ev = getenv("BC_INGEST_THREADS")) o.threads = (unsigned)std::min(64, std::max(1, atoi(ev)));
  if (const char* ev = getenv("BC_INGEST_CHUNK")) o.chunk = (size_t)std::max(4096L, atol(ev));
  if (const char* ev = getenv("BC_GZ_SPAN_BYTES")) o.gz_span = (size_t)std::min(128L << 20, std::max(1024L, atol(ev)));
  if (const char* ev = getenv("BC_GZ_PART_BYTES")) o.gz_part = (size_t)std::min(1L << 20, std::max(64L, atol(ev))) & ~(size_t)7;
  return o;
}

// A .gz file that is BGZF through and through is inflated on the device, block by block (BC_GZ_DEVICE=0: never); every
// other one is a single zlib stream on the host, or with BC_GZ_DEVICE=all goes to the device as well, span by span.
// A *.bam file always goes the device way, whatever BC_GZ_DEVICE says (that switch is about .gz names); one that is not
// BGZF, or cannot be read, leaves the reason in *bam_error.
// false: the name is none of *.fastq, *.fastq.gz and *.bam (input.rs:34-39).
bool decide_path(const std::string& path, Options::GzDevice mode, std::vector<BgzfMember>* members, uint64_t* inflated, InputPath* kind,
                 std::string* bam_error) {
  *kind = InputPath::Plain;
  std::string why;
  if (ends_with(path, ".bam")) {
    *kind = InputPath::BamDevice;
    const int rc = bgzf_index(path, members, inflated, &why);
    if (rc < 0) *bam_error = "Failed to open file: " + path;
    if (rc > 0) *bam_error = "not a BAM file: " + path + " is not BGZF: " + why;
    return true;
  }
  if (!ends_with(path, "fastq.gz")) return ends_with(path, "fastq");
  if (mode != Options::GzDevice::Never && bgzf_index(path, members, inflated, &why) == 0)
    *kind = InputPath::BgzfDevice;
  else
    *kind = mode == Options::GzDevice::All ? InputPath::GzipDevice : InputPath::Zlib;
  return true;
}

// One shard of several (one per GPU of a job): the records that START inside this shard's share of the bytes.
struct ShardPlan {
  bool nothing = false;  // a gz stream cannot be entered in the middle: its first shard takes all of it, the others this
  // BGZF: the shard's share of the INFLATED bytes [text_a, text_b), both ends on record starts, and the blocks that
  // cover it; the text of a shared first block before text_a is skipped by the framing (the device state starts there)
  unsigned long long text_a = 0, text_b = 0;
  size_t first_member = 0, end_member = 0;
  size_t last_text_member = (size_t)-1;  // last shard: the file's last block that holds text ...
  bool patch_last = false;               // ... and whether that text lacks its final newline
};
// (a plain file's share goes into src.pos / src.size.)  false: no record boundary found near a shard boundary
bool plan_shard(InputPath kind, Source& src, const std::vector<BgzfMember>& members, uint64_t inflated, uint32_t shard, uint32_t n_shards,
                ShardPlan* p) {
  const bool last_shard = shard + 1 == n_shards;
  p->text_b = inflated;
  p->end_member = members.size();
  if (kind == InputPath::BamDevice) {
    // (text_a: the first record's offset, set by the caller.)  The blocks from the one that holds it on; a BAM file
    // cannot be entered in the middle without walking its records, so its first shard takes all of it
    p->nothing = shard != 0;
    p->first_member = members.empty() ? 0 : bgzf_shard_members(members, p->text_a, p->text_b, 1, 2).first_member;  // (as a last shard's)
  } else if (kind == InputPath::BgzfDevice) {
    if (n_shards > 1) {
      BgzfHostReader hr;
      hr.fd = src.fd;
      hr.members = &members;
      hr.inflated = inflated;
      const long long a = gz_record_start_at_or_after(hr, inflated / n_shards * shard);
      const long long b = last_shard ? (long long)inflated : gz_record_start_at_or_after(hr, inflated / n_shards * (shard + 1));
      if (a < 0 || b < 0) return false;
      p->text_a = (unsigned long long)a;
      p->text_b = (unsigned long long)std::max(a, b);
      const BgzfShard blocks = bgzf_shard_members(members, p->text_a, p->text_b, shard, n_shards);
      p->first_member = blocks.first_member;
      p->end_member = blocks.end_member;
    }
    if (last_shard) {
      for (size_t k = members.size(); k-- > p->first_member;)
        if (members[k].isize) {
          p->last_text_member = k;
          break;
        }
      // (a damaged block is the device's to report: here it only means "nothing to patch")
      std::vector<uint8_t> last_text;
      p->patch_last = p->last_text_member != (size_t)-1 && bgzf_inflate_host(src.fd, members[p->last_text_member], &last_text) &&
                      !last_text.empty() && last_text.back() != '\n';
    }
  } else if (n_shards > 1 && gz_line_rules(kind)) {
    p->nothing = shard != 0;
  } else if (n_shards > 1) {
    const unsigned long long size = src.size;
    const long long a = record_start_at_or_after(plain_reader(src.fd), size / n_shards * shard, size);
    const long long b = last_shard ? (long long)size : record_start_at_or_after(plain_reader(src.fd), size / n_shards * (shard + 1), size);
    if (a < 0 || b < 0) return false;
    src.pos = (unsigned long long)a;
    src.size = (unsigned long long)std::max(a, b);
  }
  return true;
}

std::unique_ptr<Producer> make_producer(Ingest& in, Source& src, const std::vector<BgzfMember>& members, const ShardPlan& sp,
                                        const Options& opt, const Sizes& sz, int device, GzDevStats* gzs) {
  if (bgzf_blocks(in.kind)) {
    auto p = std::make_unique<BgzfProducer>(src, members, in.path);
    p->fill_cap = sz.fill_cap;
    p->chunk = in.chunk;
    p->blk_cap = in.blk_cap;
    p->first_member = sp.first_member;
    p->end_member = sp.end_member;
    p->text_b = sp.text_b;
    p->patch_last = sp.patch_last;
    p->last_text_member = sp.last_text_member;
    return p;
  }
  if (in.kind != InputPath::GzipDevice) return std::make_unique<ReaderProducer>(src, in.chunk, in.path);
  auto p = std::make_unique<GzDevProducer>();
  p->in = &in;
  p->fd = src.fd;
  p->device = device;
  p->st = in.st_gz;
  p->pin = in.gz_pin;
  p->d_comp = in.d_gz_comp;
  p->comp_cap = in.comp_cap;
  p->span_bytes = sz.gz_span;
  p->part_bytes = (uint32_t)opt.gz_part;
  p->path = in.path;
  p->stats = gzs;
  return p;
}

// The pinned and device buffers of the last call are kept for the next one on the same device with the same chunk size
// (pinning a few hundred MiB costs more than reading a small file); one call at a time per process: a call holds g_mu
// from before it acquires the buffers until it returns.
std::mutex g_mu;
Ingest* g_cached = nullptr;
int g_device = -1;

void drop_cached() {
  g_cached->release();
  delete g_cached;
  g_cached = nullptr;
}

// The cached set when it fits, a new one otherwise; a set that has not seen BGZF or gzip-device input yet gets the
// buffers only those need.  On failure nothing stays cached.
int acquire_buffers(int device, size_t chunk, InputPath kind, size_t gz_comp_cap, Ingest** out) {
  *out = nullptr;
  if (g_cached && (g_device != device || g_cached->chunk != chunk)) drop_cached();
  int rc = BC_OK;
  if (!g_cached) {
    g_cached = new Ingest();
    g_cached->chunk = chunk;
    g_device = device;
    if (hipStreamCreateWithFlags(&g_cached->st, hipStreamNonBlocking) != hipSuccess) {
      set_error("bc_fastq_count: could not create a stream");
      rc = BC_ERR_HIP;
    }
    if (rc == BC_OK) rc = g_cached->alloc();
  }
  if (rc == BC_OK && bgzf_blocks(kind)) rc = g_cached->alloc_bgzf();
  if (rc == BC_OK && kind == InputPath::BamDevice) rc = g_cached->alloc_bam();
  if (rc == BC_OK && kind == InputPath::GzipDevice) rc = g_cached->alloc_gzdev(gz_comp_cap);
  if (rc != BC_OK) {
    drop_cached();
    return rc;
  }
  *out = g_cached;
  return BC_OK;
}

// First record only (input.rs:139-142, parse.rs:377-394), on the text of the stream's first chunk (slot s).
int check_first_record(const Ingest& in, int fd, const Slot& s, bool eof) {
  const char* t = (const char*)s.pin;
  size_t tlen = s.len;  // the text the check may look at
  std::vector<uint8_t> head;
  if (in.kind == InputPath::BgzfDevice) {
    // the pinned buffer holds compressed bytes; the chunk's first blocks are inflated on the host, as far as the check
    // looks.  A damaged block is the device's to report.
    std::vector<uint8_t> one;
    size_t lines = 0;
    for (size_t k = s.first_blk; k < s.first_blk + s.nblk && lines < 5; ++k) {
      if (!bgzf_inflate_host(fd, (*in.members)[k], &one)) break;
      lines += (size_t)std::count(one.begin(), one.end(), (uint8_t)'\n');
      head.insert(head.end(), one.begin(), one.end());
    }
    if (head.size() > s.len) head.resize(s.len);
    t = (const char*)head.data();
    tlen = head.size();
  } else if (in.kind == InputPath::GzipDevice) {
    t = (const char*)in.gz_head.data();
    tlen = in.gz_head.size();
  }
  switch (first_record_check(t, tlen, eof, gz_line_rules(in.kind))) {
    case FirstRecord::FirstLineIsSequence:
      set_error("The first line within the FASTQ contains DNA sequences.  Check the FASTQ format");
      return BC_ERR_INVALID;
    case FirstRecord::SecondLineNotSequence:
      set_error("The second line within the FASTQ file is not a sequence. Check the FASTQ format");
      return BC_ERR_INVALID;
    default:
      return BC_OK;
  }
}

// The partial record at the end of a gz stream (stream_tail().post_partial_record): the three lines behind the last whole
// record of `slot`.  The record's second line, fetched back from the device text, goes through the engine as one read
// with a quality line of length 0.
int post_partial_record(Ingest& in, int slot, bc_engine* e) {
  const unsigned long long from = in.slot[slot].stats->end_pos, upto = in.s_text_len[slot];
  std::vector<char> tail((size_t)(upto > from ? upto - from : 0));
  if (!tail.empty() && hipMemcpy(tail.data(), in.s_text[slot] + from, tail.size(), hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("bc_fastq_count: reading the stream's last lines back failed");
    return BC_ERR_HIP;
  }
  const char* l1 = (const char*)memchr(tail.data(), '\n', tail.size());
  const char* l2 = l1 ? (const char*)memchr(l1 + 1, '\n', tail.size() - (size_t)(l1 + 1 - tail.data())) : nullptr;
  if (!l1 || !l2) return BC_OK;
  const size_t n = (size_t)(l2 - (l1 + 1));
  if (n > 65535) {
    set_error("a FASTQ line is longer than 65535 bytes (not supported by the engine)");
    return BC_ERR_UNSUPPORTED;
  }
  const uint32_t one_stride = std::max<uint32_t>(16u, (uint32_t)((n + 15) & ~(size_t)15));
  uint8_t* d_one = nullptr;
  if (hipMalloc((void**)&d_one, (size_t)one_stride * 2 + 32) != hipSuccess) {
    (void)hipGetLastError();
    set_error("bc_fastq_count: out of device memory");
    return BC_ERR_NOMEM;
  }
  std::vector<uint8_t> host((size_t)one_stride * 2 + 32, (uint8_t)'\n');
  memcpy(host.data(), l1 + 1, n);
  const uint16_t len16 = (uint16_t)n, qlen16 = 0;
  memcpy(host.data() + 2 * (size_t)one_stride, &len16, 2);
  memcpy(host.data() + 2 * (size_t)one_stride + 16, &qlen16, 2);
  int rc = hipMemcpy(d_one, host.data(), host.size(), hipMemcpyHostToDevice) == hipSuccess ? BC_OK : BC_ERR_HIP;
  if (rc == BC_OK)
    rc = bc_engine_submit_device_q(e, d_one, d_one + one_stride, d_one + 2 * (size_t)one_stride, d_one + 2 * (size_t)one_stride + 16,
                                   one_stride, 1);
  if (rc == BC_OK) rc = bc_engine_sync(e);
  (void)hipFree(d_one);
  return rc;
}

}  // namespace

static int fastq_count_impl(bc_engine* e, const char* fastq_path, uint32_t shard, uint32_t n_shards, uint64_t* total_reads,
                            bc_progress_fn progress, void* user);

// where bc_fastq_count_shard would start a shard that nominally begins at byte `offset` (host logic only, no GPU)
extern "C" int bc_fastq_record_start(const char* fastq_path, uint64_t offset, uint64_t* start) {
  *start = 0;
  const int fd = open(fastq_path ? fastq_path : "", O_RDONLY);
  if (fd < 0) {
    set_error(std::string("Failed to open file: ") + (fastq_path ? fastq_path : ""));
    return BC_ERR_INVALID;
  }
  const off_t end = lseek(fd, 0, SEEK_END);
  const long long at = record_start_at_or_after(plain_reader(fd), offset, end > 0 ? (unsigned long long)end : 0ull);
  close(fd);
  if (at < 0) {
    set_error("no FASTQ record boundary found (read error, or not 4-line FASTQ)");
    return BC_ERR_INVALID;
  }
  *start = (uint64_t)at;
  return BC_OK;
}

extern "C" int bc_fastq_gz_record_start(const char* path, uint64_t inflated_offset, uint64_t* start) {
  *start = 0;
  const std::string p = path ? path : "";
  std::vector<BgzfMember> members;
  BgzfHostReader hr;
  std::string why;
  const int rc = bgzf_index(p, &members, &hr.inflated, &why);
  if (rc < 0) {
    set_error("Failed to open file: " + p);
    return BC_ERR_INVALID;
  }
  if (rc > 0) {
    set_error("not BGZF: " + why);
    return BC_ERR_UNSUPPORTED;
  }
  hr.fd = open(p.c_str(), O_RDONLY);
  hr.members = &members;
  const long long at = hr.fd < 0 ? -1 : gz_record_start_at_or_after(hr, inflated_offset);
  if (hr.fd >= 0) close(hr.fd);
  if (at < 0) {
    set_error("no FASTQ record boundary found (read error, damaged block, or not 4-line FASTQ)");
    return BC_ERR_INVALID;
  }
  *start = (uint64_t)at;
  return BC_OK;
}

extern "C" int bc_fastq_count(bc_engine* e, const char* fastq_path, uint64_t* total_reads, bc_progress_fn progress,
                              void* user) {
  return fastq_count_impl(e, fastq_path, 0, 1, total_reads, progress, user);
}

extern "C" int bc_fastq_count_shard(bc_engine* e, const char* fastq_path, uint32_t shard, uint32_t n_shards,
                                    uint64_t* total_reads, bc_progress_fn progress, void* user) {
  if (n_shards == 0 || shard >= n_shards) {
    set_error("bc_fastq_count_shard: shard outside 0 .. n_shards-1");
    return BC_ERR_INVALID;
  }
  return fastq_count_impl(e, fastq_path, shard, n_shards, total_reads, progress, user);
}

static int fastq_count_impl(bc_engine* e, const char* fastq_path, uint32_t shard, uint32_t n_shards, uint64_t* total_reads,
                            bc_progress_fn progress, void* user) {
  if (total_reads) *total_reads = 0;
  const std::string path = fastq_path ? fastq_path : "";
  const Options opt = read_options();
  std::vector<BgzfMember> members;
  uint64_t inflated = 0;
  InputPath kind;
  std::string bam_error;
  if (!decide_path(path, opt.gz_device, &members, &inflated, &kind, &bam_error)) {
    set_error("This program only works with *.fastq files and *.fastq.gz files.  The latter is still experimental");
    return BC_ERR_INVALID;
  }
  if (!bam_error.empty()) {
    set_error(bam_error);
    return BC_ERR_INVALID;
  }
  Source src;
  if (!src.open(path, kind)) {
    set_error("Failed to open file: " + path);
    return BC_ERR_INVALID;
  }
  // The file is open: every return from here on goes through finish(), which drains the streams once buffers are in use,
  // closes the file and prints the verbose line.
  Ingest* in = nullptr;
  GzDevStats gzs;
  uint64_t total = 0;
  auto finish = [&](int code) {
    if (in) {
      if (in->st_gz) (void)hipStreamSynchronize(in->st_gz);
      (void)hipStreamSynchronize(in->st);
      (void)bc_engine_sync(e);  // the match kernels read the batch arrays, which the next call reuses
    }
    src.close();
    const char* failed = code == BC_OK ? "" : " (failed)";
    if (opt.verbose && kind == InputPath::GzipDevice)
      fprintf(stderr, "[bc ingest] %s: path gzip-device, shard %u/%u, %llu spans, %llu segments, %llu candidates rejected, %llu retries, "
              "%llu records counted%s\n", path.c_str(), shard, n_shards, (unsigned long long)gzs.spans, (unsigned long long)gzs.segments,
              (unsigned long long)gzs.rejected, (unsigned long long)gzs.retries, (unsigned long long)total, failed);
    else if (opt.verbose)
      fprintf(stderr, "[bc ingest] %s: path %s, shard %u/%u, %llu BGZF blocks inflated on the device, %llu records counted%s\n",
              path.c_str(), input_path_name(kind), shard, n_shards, (unsigned long long)(in ? in->blocks_inflated : 0),
              (unsigned long long)total, failed);
    return code;
  };
  if (kind == InputPath::Plain) {  // (a BGZF file is read by its index: `size` stays 0)
    const off_t end = lseek(src.fd, 0, SEEK_END);
    src.size = end > 0 ? (unsigned long long)end : 0ull;
  }
  const bool last_shard = shard + 1 == n_shards;
  ShardPlan sp;
  uint32_t n_ref = 0;
  if (kind == InputPath::BamDevice) {  // the header is the host's: the framing starts behind it
    uint64_t first_record = 0;
    std::string why;
    if (!bam_header(src.fd, members, inflated, &n_ref, &first_record, &why)) {
      set_error("not a BAM file: " + path + ": " + why);
      return finish(BC_ERR_INVALID);
    }
    sp.text_a = first_record;
  }
  if (!plan_shard(kind, src, members, inflated, shard, n_shards, &sp)) {
    set_error("no FASTQ record boundary found near a shard boundary of " + path + " (read error, or not 4-line FASTQ)");
    return finish(BC_ERR_INVALID);
  }
  if (sp.nothing) return finish(BC_OK);
  src.threads = opt.threads;
  const Sizes sz = sizes_for(opt, kind, bgzf_blocks(kind) ? sp.text_b - sp.text_a : src.size);

  std::unique_lock<std::mutex> whole_call(g_mu);
  const int device = bc_engine_device(e);
  if (hipSetDevice(device) != hipSuccess) {
    set_error("bc_fastq_count: no HIP device");
    return finish(BC_ERR_HIP);
  }
  int rc = acquire_buffers(device, sz.chunk, kind, sz.chunk + sz.gz_span + 65536, &in);
  if (rc != BC_OK) return finish(rc);
  in->begin_call(e, kind, &members, path);
  in->n_ref = n_ref;
  if ((rc = in->set_start(sp.text_a)) != BC_OK) return finish(rc);  // (text_a: a BGZF shard's first record, 0 otherwise)

  // the producer runs ahead of the device by the slots that are free: its thread fills, this thread frames
  const std::unique_ptr<Producer> producer = make_producer(*in, src, members, sp, opt, sz, device, &gzs);
  Handoff h;
  std::thread producer_thread([&] { produce(*producer, in->slot, h); });

  uint64_t lines_after_last_record = 0;
  bool test = shard == 0 && kind != InputPath::BamDevice;  // (the file's first record is the first shard's)
  unsigned long long bam_left = 0;  // BAM: bytes behind the last whole record of the last chunk counted
  int pending = -1;  // chunk framed but not yet submitted
  int last_counted_slot = -1;  // slot of the last chunk whose records were counted (its text is still on the device)
  // the pending chunk: its stats are in (or about to be); its records go to the engine and into the total
  auto count_pending = [&]() -> int {
    const int b = pending % kSlots;
    uint64_t n_rec = 0;
    const int r = in->submit(b, &n_rec);
    if (r != BC_OK) return r;
    total += n_rec;
    if (progress && n_rec) progress(total - total % 10000, user);  // the reference prints every 10,000 reads (input.rs:54-57)
    const ChunkStats& cs = *in->slot[b].stats;
    lines_after_last_record = cs.n_lines - 4 * cs.n_rec;
    bam_left = in->s_text_len[b] - cs.end_pos;
    last_counted_slot = b;
    pending = -1;
    return BC_OK;
  };
  for (int i = 0;; ++i) {
    {
      std::unique_lock<std::mutex> lk(h.mu);
      h.cv.wait(lk, [&] { return h.filled_upto > i; });
      if (h.rc != BC_OK) {
        set_error(h.error);
        rc = h.rc;
      }
    }
    if (rc != BC_OK) break;
    Slot& s = in->slot[i % kSlots];
    const bool eof = s.eof;
    if (s.len) {
      if (test) {
        test = false;
        if ((rc = check_first_record(*in, src.fd, s, eof)) != BC_OK) break;
      }
      // (on the device paths the unterminated last character of the stream becomes the missing newline after the
      // inflate: s.patch_at)
      if (!text_on_device(kind) && eof && s.pin[s.len - 1] != '\n') {
        if (!gz_line_rules(kind)) {  // lines() hands the last line over without its newline (input.rs:44): framing-wise it has one
          s.pin[s.len++] = '\n';
        } else {
          // read_line hands the unterminated last line over as it is, and post() pops the record's last character
          // whatever it is (input.rs:137): when that line is a record's fourth, the record is scored with a quality
          // line one character short.  Turning the character into the missing newline is exactly that; when the line is
          // a record's first, second or third, no record comes of it and only the line count matters.
          s.pin[s.len - 1] = '\n';
        }
      }
      rc = in->frame(i % kSlots, i > 0 ? &in->slot[(i - 1) % kSlots] : nullptr);
      if (rc != BC_OK) break;
    } else if (bgzf_blocks(kind) && s.nblk) {
      if (!eof) {  // (thousands of empty blocks in a row, in the middle of the file)
        set_error("a BGZF chunk of " + path + " holds no text: not supported by the engine");
        rc = BC_ERR_UNSUPPORTED;
        break;
      }
      rc = in->inflate_only(i % kSlots);
      if (rc != BC_OK) break;
    }
    // the chunk before this one: count it while this one is being framed
    if (pending >= 0) {
      if ((rc = count_pending()) != BC_OK) break;
      std::lock_guard<std::mutex> lk(h.mu);
      h.released_upto = i + kSlots - 1;  // slot (i - 1) % kSlots may be refilled once its upload event has fired
      h.cv.notify_all();
    }
    if (s.len) pending = i;
    if (eof) {
      if (pending >= 0) rc = count_pending();
      break;
    }
  }
  {
    std::lock_guard<std::mutex> lk(h.mu);
    h.stop = true;
  }
  h.cv.notify_all();
  producer_thread.join();
  if (kind == InputPath::GzipDevice) engine_add_gz_segments(e, gzs.segments);
  if (rc != BC_OK) return finish(rc);
  if (kind == InputPath::BamDevice) {  // every whole record is one read; the file has to end with one
    if (bam_left) {
      set_error("read error in " + path + ": the file ends inside a BAM record (" + std::to_string(bam_left) + " bytes behind the last whole one)");
      return finish(BC_ERR_INVALID);
    }
    if (total_reads) *total_reads = total;
    return finish(BC_OK);
  }

  // what is left after the last whole record: fewer than four complete lines, the ones the reference's reader would have
  // been handed (gz without a final newline: the unterminated last line was given its newline above, so it is among the
  // lines the device counted)
  const size_t seen = (size_t)lines_after_last_record;
  if (!last_shard && !((kind == InputPath::Zlib || kind == InputPath::GzipDevice) && shard == 0) && seen != 0) {
    // a shard that does not end the file ends on a record boundary; lines left over mean the file's lines do not
    // come in fours from where this shard started -- the reference, framing from the file's first line, would read
    // it differently from here on
    set_error("the lines of " + path + " do not come in records of four: run it on one GPU");
    return finish(BC_ERR_INVALID);
  }
  // (the end of the stream is the last shard's: a BGZF file's other shards end on a record boundary)
  const StreamTail tail = stream_tail(seen, gz_line_rules(kind) && (kind != InputPath::BgzfDevice || last_shard));
  if (tail.post_partial_record && last_counted_slot >= 0 && (rc = post_partial_record(*in, last_counted_slot, e)) != BC_OK) return finish(rc);
  total += tail.extra_total;
  if (total_reads) *total_reads = total;
  return finish(BC_OK);
}
