// bc_strand.hip -- the strand setting of a plan (bc_plan_set_strand): reads counted as their reverse complement, or as
// they stand first and reversed when the constant region fails.  Orientation is decided here, around the match kernels
// as they are (DESIGN.md "Reverse strand"): submit_strand() is what every submit of an engine whose strand is not
// BC_STRAND_FORWARD goes through, chunk by chunk --
//   reverse: orient(all) into the engine's scratch batch, then the ordinary launch on that batch;
//   both:    pass 1 with per-read outcomes recorded, select, the host reads the number m of constant-region failures
//            (one wait per chunk), then fix-up, orient(list), pass 2 on the m reads, and their trace scattered back.
// The kernels are bc_strand_kernels.h; bc_strand_orient_device is the orient kernel on its own.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "bc_strand_kernels.h"
#include "bc_engine_impl.h"

using namespace bc;

namespace {

// the orient kernel over n_out output reads: as many lanes to a line as it has slots (a power of two, 64 at most)
hipError_t orient_launch(hipStream_t st, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens, uint32_t stride,
                         uint32_t read_len, const uint32_t* d_index, uint64_t n_out, void* d_seq_out, void* d_qual_out, void* d_lens_out,
                         void* d_qlens_out) {
  if (n_out == 0) return hipSuccess;
  const uint32_t slots = 1u + (stride + 3u) / 4u;
  uint32_t shift = 1;
  while (shift < 6u && (1u << shift) < slots) ++shift;
  const uint64_t rows = kStrandTPB >> shift;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_out + rows - 1) / rows, 1ull << 16);
  hipLaunchKernelGGL(strand_orient_kernel, dim3(blocks), dim3(kStrandTPB), 0, st, (const uint8_t*)d_seq, (const uint8_t*)d_qual,
                     (const uint16_t*)d_lens, (const uint16_t*)d_qlens, stride, read_len, d_index, (unsigned long long)n_out,
                     (uint8_t*)d_seq_out, d_qual ? (uint8_t*)d_qual_out : nullptr, (uint16_t*)d_lens_out, (uint16_t*)d_qlens_out, shift);
  return hipGetLastError();
}

constexpr uint32_t kSelectMaxBlocks = 1024;

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

// the engine's scratch for chunks of up to `cap` reads of one batch form, cut from one allocation
struct StrandScratch {
  uint8_t *seq = nullptr, *qual = nullptr;
  uint16_t *lens = nullptr, *qlens = nullptr;
  uint32_t *list = nullptr, *blk_cnt = nullptr, *count = nullptr;
  uint8_t* outcome = nullptr;
  uint64_t* idx = nullptr;
};

// Grows on demand, never shrinks, freed with the engine.  For a chunk of C reads at stride S: the scratch batch,
// C * (2 * S + 4) bytes at most (both lines, both length arrays); with `both` also the list (4 C), the outcome bytes (C)
// and the index array the traced match kernels write beside them (8 C), and 4 KB for select.
int ensure_scratch(bc_engine* e, uint64_t cap, uint32_t stride, bool with_qual, bool with_lens, bool with_qlens, bool both,
                   StrandScratch* s) {
  cap = (cap + 255) & ~255ull;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += round256(bytes);
    return at;
  };
  const size_t a_seq = take((size_t)cap * stride), a_qual = take(with_qual ? (size_t)cap * stride : 0),
               a_lens = take(with_lens ? cap * 2 : 0), a_qlens = take(with_qlens ? cap * 2 : 0), a_list = take(both ? cap * 4 : 0),
               a_blk = take(both ? kSelectMaxBlocks * 4 : 0), a_count = take(both ? 4 : 0), a_idx = take(both ? cap * 8 : 0),
               a_out = take(both ? cap : 0);
  if (off > e->strand_bytes) {
    if (e->d_strand) {
      HIP_TRY(hipStreamSynchronize(e->stream));  // the last reverse pass may still read it
      HIP_TRY(hipFree(e->d_strand));
      e->d_strand = nullptr;
      e->strand_bytes = 0;
    }
    HIP_TRY(hipMalloc((void**)&e->d_strand, off));
    e->strand_bytes = off;
  }
  uint8_t* b = e->d_strand;
  s->seq = b + a_seq;
  s->qual = with_qual ? b + a_qual : nullptr;
  s->lens = with_lens ? (uint16_t*)(b + a_lens) : nullptr;
  s->qlens = with_qlens ? (uint16_t*)(b + a_qlens) : nullptr;
  s->list = (uint32_t*)(b + a_list);
  s->blk_cnt = (uint32_t*)(b + a_blk);
  s->count = (uint32_t*)(b + a_count);
  s->idx = (uint64_t*)(b + a_idx);
  s->outcome = b + a_out;
  if (!e->d_strand_stats) {
    HIP_TRY(hipMalloc((void**)&e->d_strand_stats, 3 * 8));
    HIP_TRY(hipMemsetAsync(e->d_strand_stats, 0, 3 * 8, e->stream));
  }
  if (both && !e->strand_count_pin) HIP_TRY(hipHostMalloc((void**)&e->strand_count_pin, 64, hipHostMallocDefault));
  return BC_OK;
}

}  // namespace

void bc::strand_free(bc_engine* e) {
  if (e->d_strand) (void)hipFree(e->d_strand);
  if (e->d_strand_stats) (void)hipFree(e->d_strand_stats);
  if (e->strand_count_pin) (void)hipHostFree(e->strand_count_pin);
}

int bc::submit_strand(bc_engine* e, const void* d_seq, const void* d_qual, const void* d_lens, const void* d_qlens, uint32_t stride,
                      uint32_t read_len, uint64_t n_reads, uint64_t trace_off) {
  HIP_TRY(hipSetDevice(e->device));
  const bool both = e->strand == BC_STRAND_BOTH;
  const bool user_trace = e->trace_outcome != nullptr;
  StrandScratch s;
  {
    const int rc = ensure_scratch(e, std::min<uint64_t>(n_reads, e->strand_chunk), stride, d_qual != nullptr, d_lens != nullptr,
                                  d_qlens != nullptr, both, &s);
    if (rc != BC_OK) return rc;
  }
  hipStream_t st = e->stream;
  for (uint64_t c0 = 0; c0 < n_reads; c0 += e->strand_chunk) {
    const uint64_t n_c = std::min<uint64_t>(e->strand_chunk, n_reads - c0);
    const uint8_t* a_seq = (const uint8_t*)d_seq + c0 * stride;
    const uint8_t* a_qual = d_qual ? (const uint8_t*)d_qual + c0 * stride : nullptr;
    const uint16_t* a_lens = d_lens ? (const uint16_t*)d_lens + c0 : nullptr;
    const uint16_t* a_qlens = d_qlens ? (const uint16_t*)d_qlens + c0 : nullptr;
    uint8_t* u_out = user_trace ? e->trace_outcome + trace_off + c0 : nullptr;
    uint64_t* u_idx = user_trace && e->trace_idx ? e->trace_idx + trace_off + c0 : nullptr;
    const uint32_t* list = nullptr;
    uint64_t m = n_c;
    if (both) {
      // pass 1, every read's outcome recorded: at the reads' own positions of the caller's trace, else in scratch
      uint8_t* out1 = user_trace ? u_out : s.outcome;
      int rc = submit_forward(e, a_seq, a_qual, a_lens, a_qlens, stride, read_len, n_c, out1, user_trace ? u_idx : s.idx);
      if (rc != BC_OK) return rc;
      const uint32_t span = std::max<uint32_t>(256u, (uint32_t)(((n_c + kSelectMaxBlocks - 1) / kSelectMaxBlocks + 255) & ~255ull));
      const uint32_t n_blk = (uint32_t)((n_c + span - 1) / span);
      hipLaunchKernelGGL(strand_select_count_kernel, dim3(n_blk), dim3(kStrandTPB), 0, st, out1, (uint32_t)n_c, span, s.blk_cnt);
      hipLaunchKernelGGL(strand_select_write_kernel, dim3(n_blk), dim3(kStrandTPB), 0, st, out1, (uint32_t)n_c, span, s.blk_cnt, s.list,
                         s.count);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(e->strand_count_pin, s.count, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));  // the one host wait per chunk: the grid and the key table's growth need m
      m = *e->strand_count_pin;
      if (m == 0) continue;
      list = s.list;
    }
    hipLaunchKernelGGL(strand_before_kernel, dim3(1), dim3(1), 0, st, e->d_counters, e->d_strand_stats, (unsigned long long)m, both ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    HIP_TRY(orient_launch(st, a_seq, a_qual, a_lens, a_qlens, stride, read_len, list, m, s.seq, s.qual, s.lens, s.qlens));
    // the reverse pass: the kernel shape of pass 1 (same stride, same form of lengths).  `both`: traced only for a
    // caller's trace, into scratch (pass 1's outcome bytes live in the caller's array then), and scattered back
    uint8_t* out2 = both ? (user_trace ? s.outcome : nullptr) : u_out;
    uint64_t* idx2 = both ? (user_trace ? s.idx : nullptr) : u_idx;
    const int rc = submit_forward(e, s.seq, s.qual, s.lens, s.qlens, stride, read_len, m, out2, idx2);
    if (rc != BC_OK) return rc;
    hipLaunchKernelGGL(strand_after_kernel, dim3(1), dim3(1), 0, st, e->d_counters, e->d_strand_stats);
    if (both && user_trace)
      hipLaunchKernelGGL(strand_scatter_kernel, dim3((uint32_t)std::min<uint64_t>((m + kStrandTPB - 1) / kStrandTPB, 4096)),
                         dim3(kStrandTPB), 0, st, list, (uint32_t)m, s.outcome, s.idx, u_out, u_idx);
    HIP_TRY(hipGetLastError());
  }
  return BC_OK;
}

extern "C" {

int bc_engine_strand_reads(const bc_engine* e, uint64_t* retried, uint64_t* matched_reverse) {
  unsigned long long v[3] = {0, 0, 0};
  if (e->d_strand_stats) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(v, e->d_strand_stats, sizeof v, hipMemcpyDeviceToHost));
  }
  if (retried) *retried = v[0];
  if (matched_reverse) *matched_reverse = v[1];
  return BC_OK;
}

int bc_strand_orient_device(int device_id, void* hip_stream, const void* d_seq, const void* d_qual, const void* d_lens,
                            const void* d_qlens, uint32_t stride, uint32_t read_len, const uint32_t* d_index, uint64_t n_out,
                            void* d_seq_out, void* d_qual_out, void* d_lens_out, void* d_qlens_out) {
  if (n_out == 0) return BC_OK;
  if (!d_seq || !d_seq_out || stride == 0 || (d_qual && !d_qual_out) || (d_lens && !d_lens_out) || (d_qlens && !d_qlens_out)) {
    set_error("bc_strand_orient_device: null buffer (every input given needs its output) or zero stride");
    return BC_ERR_INVALID;
  }
  if ((((uintptr_t)d_seq | (uintptr_t)d_qual | (uintptr_t)d_seq_out | (uintptr_t)d_qual_out) & 15u) ||
      (((uintptr_t)d_lens | (uintptr_t)d_qlens | (uintptr_t)d_lens_out | (uintptr_t)d_qlens_out) & 1u) || ((uintptr_t)d_index & 3u)) {
    set_error("bc_strand_orient_device: buffers must be 16-byte aligned");
    return BC_ERR_INVALID;
  }
  if (!d_lens && read_len > stride) {
    set_error("bc_strand_orient_device: read_len exceeds stride");
    return BC_ERR_INVALID;
  }
  if (d_seq_out == d_seq || (d_qual && d_qual_out == d_qual)) {
    set_error("bc_strand_orient_device: a line cannot be reversed in place");
    return BC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device_id));
  HIP_TRY(orient_launch((hipStream_t)hip_stream, d_seq, d_qual, d_lens, d_qlens, stride, read_len, d_index, n_out, d_seq_out, d_qual_out,
                        d_lens_out, d_qlens_out));
  return BC_OK;
}

}  // extern "C"
