// bc_bam.hip -- unaligned BAM on the device: the launches of the framing and gather kernels (bc_bam_kernels.h; the
// per-record logic is bc_bam.h) for the ingest, the header parse on the host, and the C ABI around them: bc_bam_scan and
// bc_bam_frame_device.  A BAM file is a BGZF container: its blocks are indexed and inflated by bc_inflate.hip, and
// bc_ingest.hip moves them; only what the inflated bytes MEAN is decided here.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>

#include "bc_bam_kernels.h"
#include "bc_bgzf.hpp"
#include "bc_fastq_host.hpp"
#include "bc_plan.hpp"

namespace bc {

uint32_t bam_levels(uint32_t cap) {
  uint32_t levels = 1;
  while (bam_level_used(levels, cap)) ++levels;
  return levels;
}

size_t bam_count_blocks(uint64_t len_max, uint32_t cap) {
  return (size_t)std::max<uint64_t>((len_max + kBamScanBlock - 1) / kBamScanBlock, ((uint64_t)cap + 255) / 256) + 1;
}

int bam_frame_launch(void* stream, const uint8_t* d_text, uint64_t len, uint32_t n_ref, const unsigned long long* d_next_off,
                     unsigned long long buf_file_off, long long start, uint32_t skip_flags, const BamWork& w, const BamTables& out,
                     BamStats* fs) {
  hipStream_t st = (hipStream_t)stream;
  const uint32_t n_blk = (uint32_t)((len + kBamScanBlock - 1) / kBamScanBlock);
  const uint32_t n_blk_rec = (w.cap + 255u) / 256u;
  const dim3 strided(kBamStrideBlocks), one(1), group(256);
  hipLaunchKernelGGL(bam_begin_kernel, one, one, 0, st, d_next_off, buf_file_off, start, fs);
  if (n_blk) {
    hipLaunchKernelGGL(bam_count_kernel, dim3(n_blk), group, 0, st, d_text, (unsigned long long)len, n_ref, fs, w.blk_cnt);
    hipLaunchKernelGGL(bam_scan_kernel, one, dim3(1024), 0, st, w.blk_cnt, n_blk, w.blk_off, &fs->n_cand, (unsigned long long)w.cap, fs);
    hipLaunchKernelGGL(bam_positions_kernel, dim3(n_blk), group, 0, st, d_text, (unsigned long long)len, n_ref, fs, w.blk_off, w.cand,
                       (unsigned long long)w.cap);
  }
  hipLaunchKernelGGL(bam_successor_kernel, strided, group, 0, st, d_text, (unsigned long long)len, n_ref, fs, w.cand, w.link, w.jump, w.mark);
  hipLaunchKernelGGL(bam_mark_start_kernel, one, one, 0, st, d_text, (unsigned long long)len, n_ref, fs, w.cand, w.mark);
  for (uint32_t k = 1; k < w.levels; ++k) hipLaunchKernelGGL(bam_jump_kernel, strided, group, 0, st, fs, w.jump, w.cap, k);
  for (uint32_t k = w.levels; k-- > 0;) hipLaunchKernelGGL(bam_mark_kernel, strided, group, 0, st, fs, w.jump, w.cap, k, w.mark);
  hipLaunchKernelGGL(bam_rec_count_kernel, dim3(n_blk_rec), group, 0, st, d_text, fs, w.cand, w.link, w.mark, skip_flags, w.blk_cnt);
  hipLaunchKernelGGL(bam_scan_kernel, one, dim3(1024), 0, st, w.blk_cnt, n_blk_rec, w.blk_off, &fs->n_rec, (unsigned long long)w.cap, fs);
  hipLaunchKernelGGL(bam_rec_table_kernel, dim3(n_blk_rec), group, 0, st, d_text, fs, w.cand, w.link, w.mark, skip_flags, w.blk_off, out);
  return (int)hipGetLastError();
}

int bam_gather_launch(void* stream, const uint8_t* d_text, const uint32_t* d_seq_at, const uint32_t* d_qual_at, const uint16_t* d_lens,
                      uint64_t first, uint64_t n, uint32_t stride, uint8_t* d_out_seq, uint8_t* d_out_qual) {
  if (n == 0) return (int)hipSuccess;
  hipLaunchKernelGGL(bam_gather_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_text, d_seq_at, d_qual_at, d_lens,
                     (unsigned long long)first, (unsigned long long)n, stride, d_out_seq, d_out_qual);
  return (int)hipGetLastError();
}

bool bam_header(int fd, const std::vector<BgzfMember>& members, uint64_t inflated, uint32_t* n_ref, uint64_t* first_record,
                std::string* why) {
  BgzfHostReader hr;
  hr.fd = fd;
  hr.members = &members;
  hr.inflated = inflated;
  const BamHeader h = bam_parse_header([&hr](char* dst, size_t n, unsigned long long at) { return hr.read_at(dst, n, at); }, inflated);
  *n_ref = h.n_ref;
  *first_record = h.first_record;
  if (h.error) *why = h.error;
  return h.error == nullptr;
}

}  // namespace bc

using namespace bc;

extern "C" int bc_bam_scan(const char* path, uint32_t* n_ref, uint64_t* first_record_offset, uint64_t* inflated_bytes) {
  if (n_ref) *n_ref = 0;
  if (first_record_offset) *first_record_offset = 0;
  if (inflated_bytes) *inflated_bytes = 0;
  const std::string p = path ? path : "";
  std::vector<BgzfMember> members;
  uint64_t inflated = 0, first = 0;
  uint32_t refs = 0;
  std::string why;
  const int rc = bgzf_index(p, &members, &inflated, &why);
  if (rc < 0) {
    set_error("Failed to open file: " + p);
    return BC_ERR_INVALID;
  }
  if (rc > 0) {
    set_error("not a BAM file: " + p + " is not BGZF: " + why);
    return BC_ERR_INVALID;
  }
  const int fd = open(p.c_str(), O_RDONLY);
  const bool ok = fd >= 0 && bam_header(fd, members, inflated, &refs, &first, &why);
  if (fd >= 0) close(fd);
  if (fd < 0) why = "the file cannot be opened";
  if (!ok) {
    set_error("not a BAM file: " + p + ": " + why);
    return BC_ERR_INVALID;
  }
  if (n_ref) *n_ref = refs;
  if (first_record_offset) *first_record_offset = first;
  if (inflated_bytes) *inflated_bytes = inflated;
  return BC_OK;
}

#define HIP_TRY(expr)                                               \
  do {                                                              \
    hipError_t _e = (expr);                                         \
    if (_e != hipSuccess) {                                         \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
      rc = BC_ERR_HIP;                                              \
      goto done;                                                    \
    }                                                               \
  } while (0)

extern "C" int bc_bam_frame_device(int device_id, void* hip_stream, const void* d_text, uint64_t len, uint64_t start, uint32_t n_ref,
                                   uint32_t* d_rec_at, uint32_t* d_rec_len, uint32_t* d_rec_flag, uint64_t capacity,
                                   bc_bam_frame_result* result) {
  if (!result) {
    set_error("bc_bam_frame_device: null result");
    return BC_ERR_INVALID;
  }
  *result = bc_bam_frame_result{};
  result->end_pos = start;
  if (start > len || len >= (1ull << 31) || capacity == 0 || capacity >= (1ull << 31) || ((uintptr_t)d_text & 15u) ||
      (len && !d_text) || !d_rec_at || !d_rec_len || !d_rec_flag) {
    set_error("bc_bam_frame_device: null or unaligned buffer, start beyond the text, or a text or capacity of 2 GiB or more");
    return BC_ERR_INVALID;
  }
  int rc = BC_OK;
  hipStream_t st = (hipStream_t)hip_stream;
  BamWork w = {};
  w.cap = (uint32_t)capacity;
  w.levels = bam_levels(w.cap);
  const size_t n_blk = bam_count_blocks(len, w.cap);
  uint32_t* d_words = nullptr;  // cand | link | mark | blk_cnt | blk_off | jump levels
  BamStats* d_stats = nullptr;
  BamStats fs = {};
  const BamTables out = {d_rec_at, d_rec_len, d_rec_flag, nullptr, nullptr, nullptr, nullptr};
  HIP_TRY(hipSetDevice(device_id));
  HIP_TRY(hipMalloc((void**)&d_words, ((size_t)w.cap * (3 + w.levels) + 2 * n_blk) * sizeof(uint32_t)));
  HIP_TRY(hipMalloc((void**)&d_stats, sizeof(BamStats)));
  w.cand = d_words;
  w.link = w.cand + w.cap;
  w.mark = w.link + w.cap;
  w.blk_cnt = w.mark + w.cap;
  w.blk_off = w.blk_cnt + n_blk;
  w.jump = w.blk_off + n_blk;
  HIP_TRY((hipError_t)bam_frame_launch(st, (const uint8_t*)d_text, len, n_ref, nullptr, 0, (long long)start, 0, w, out, d_stats));
  HIP_TRY(hipMemcpyAsync(&fs, d_stats, sizeof fs, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  result->status = fs.status;
  result->n_records = fs.n_rec;
  result->n_candidates = fs.n_cand;
  result->end_pos = fs.end_pos;
done:
  if (rc != BC_OK) (void)hipStreamSynchronize(st);
  if (d_words) (void)hipFree(d_words);
  if (d_stats) (void)hipFree(d_stats);
  return rc;
}
