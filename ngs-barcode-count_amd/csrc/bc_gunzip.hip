// bc_gunzip.hip -- ordinary gzip on the device: the kernels of the span inflater (the lane code is bc_gunzip.h), their
// launcher with the chain walk between the measure and the decode stage, and the C ABI: bc_gunzip_span_device.
#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "../../include/barcode_count_hip.h"
#include "bc_bgzf.hpp"
#include "bc_gunzip.h"
#include "bc_plan.hpp"

namespace bc {

namespace {

constexpr uint32_t kWavesPerGroup = 4;
constexpr uint32_t kSeqThreads = 1024;

__global__ __launch_bounds__(64 * kWavesPerGroup) void gunzip_find_kernel(const uint8_t* __restrict__ src, uint32_t src_len,
                                                                          uint32_t start_bit, uint32_t part_bytes, uint32_t n_parts,
                                                                          uint32_t* __restrict__ cand) {
  __shared__ InflateTables s_tab[kWavesPerGroup];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t p = blockIdx.x * kWavesPerGroup + wave;
  if (p >= n_parts) return;
  const uint32_t at = gunzip_find((const BC_GLOBAL uint8_t*)src, src_len, start_bit, p * part_bytes, (p + 1u) * part_bytes, s_tab[wave], lane);
  if (lane == 0) cand[p] = at;
}

// wave 0: the anchor; wave 1 + p: partition p's candidate
__global__ __launch_bounds__(64 * kWavesPerGroup) void gunzip_measure_kernel(const uint8_t* __restrict__ src, uint32_t src_len,
                                                                             uint32_t start_bit, uint32_t part_bytes, uint32_t n_parts,
                                                                             const uint32_t* __restrict__ cand, uint32_t budget,
                                                                             GzMeasure* __restrict__ meas) {
  __shared__ InflateTables s_tab[kWavesPerGroup];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t w = blockIdx.x * kWavesPerGroup + wave;
  if (w > n_parts) return;
  const uint32_t from = w == 0 ? start_bit : cand[w - 1u];
  GzMeasure m;
  m.end_bit = from;
  m.out_bytes = 0;
  m.reason = kGzEndError;
  m.link = kGzNone;
  m.status = kInfOk;
  if (from != kGzNone) m = gunzip_measure((const BC_GLOBAL uint8_t*)src, src_len, from, cand, n_parts, part_bytes, budget, s_tab[wave], lane);
  if (lane == 0) meas[w] = m;
}

__global__ __launch_bounds__(64 * kWavesPerGroup) void gunzip_decode_kernel(const uint8_t* __restrict__ src, uint32_t src_len,
                                                                            const GzSegment* __restrict__ segs, uint32_t n_segs,
                                                                            const uint8_t* __restrict__ hist, uint32_t hist_len,
                                                                            uint16_t* __restrict__ sym,
                                                                            uint32_t* __restrict__ status) {
  __shared__ InflateTables s_tab[kWavesPerGroup];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * kWavesPerGroup + wave;
  if (s >= n_segs) return;
  const GzSegment seg = segs[s];
  const uint32_t st = gunzip_decode((const BC_GLOBAL uint8_t*)src, src_len, seg, (BC_GLOBAL uint16_t*)(sym + seg.out_off),
                                    (const BC_GLOBAL uint8_t*)hist, hist_len, s_tab[wave], lane);
  if (lane == 0) status[s] = st;
}

// one workgroup, segment after segment: a segment's tail reads the tails before it
__global__ __launch_bounds__(kSeqThreads) void gunzip_resolve_tails_kernel(const GzSegment* __restrict__ segs, uint32_t n_segs,
                                                                           const uint16_t* sym, uint8_t* text, const uint8_t* hist,
                                                                           uint32_t hist_len, uint32_t* __restrict__ bad) {
  uint32_t mine = 0;
  for (uint32_t s = 0; s < n_segs; ++s) {
    gunzip_resolve_tail((const BC_GLOBAL uint16_t*)sym, (BC_GLOBAL uint8_t*)text, (const BC_GLOBAL uint8_t*)hist, hist_len, segs[s], threadIdx.x,
                        kSeqThreads, &mine);
    __threadfence_block();
    __syncthreads();
  }
  if (mine) atomicOr(bad, 1u);
}

__global__ __launch_bounds__(64 * kWavesPerGroup) void gunzip_resolve_kernel(const GzSegment* __restrict__ segs,
                                                                             const GzSlice* __restrict__ slices, uint32_t n_slices,
                                                                             const uint16_t* sym, uint8_t* text, const uint8_t* hist,
                                                                             uint32_t hist_len, uint32_t* __restrict__ seg_crc, uint32_t* __restrict__ bad) {
  __shared__ uint32_t s_red[kWavesPerGroup][64];
  __shared__ uint32_t s_crc[256];
  s_crc[threadIdx.x] = crc32_table_entry(threadIdx.x);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * kWavesPerGroup + wave;
  if (i >= n_slices) return;
  const GzSlice sl = slices[i];
  const GzSegment seg = segs[sl.seg];
  uint32_t mine = 0;
  const uint32_t term = gunzip_resolve_slice((const BC_GLOBAL uint16_t*)sym, (BC_GLOBAL uint8_t*)text, (const BC_GLOBAL uint8_t*)hist, hist_len, seg, sl,
                                             s_red[wave], s_crc, lane, &mine);
  if (lane == 0) atomicXor(&seg_crc[sl.seg], term);
  if (mine) atomicOr(bad, 1u);
}

// Device and pinned buffers of the launcher, kept between calls (one call at a time per process) and grown on demand,
// like the ingest's own cached buffers: they belong to the process and go with it (a static destructor would run after
// the HIP runtime may have shut down); a call for another device lets go of the previous device's set first.
struct Work {
  int device = -1;
  uint32_t parts = 0, segs = 0, slices = 0;
  uint64_t sym = 0;
  uint32_t* d_cand = nullptr;
  GzMeasure* d_meas = nullptr;
  GzSegment* d_segs = nullptr;
  GzSlice* d_slices = nullptr;
  uint32_t* d_status = nullptr;  // per segment: decode status, then CRC; one more word: the resolve's flag
  uint16_t* d_sym = nullptr;
  uint32_t* h_cand = nullptr;    // pinned
  GzMeasure* h_meas = nullptr;
  uint32_t* h_status = nullptr;
};
std::mutex g_mu;
Work g_work;

#define HIP_TRY(expr)                                               \
  do {                                                              \
    hipError_t _e = (expr);                                         \
    if (_e != hipSuccess) {                                         \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
      return BC_ERR_HIP;                                            \
    }                                                               \
  } while (0)

template <typename T>
int grow(T** p, uint64_t n, bool pinned) {
  if (*p) HIP_TRY(pinned ? hipHostFree(*p) : hipFree(*p));
  *p = nullptr;
  HIP_TRY(pinned ? hipHostMalloc((void**)p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)p, n * sizeof(T)));
  return BC_OK;
}

int reserve_parts(Work& w, uint32_t n_parts) {
  if (n_parts <= w.parts) return BC_OK;
  const uint32_t n = n_parts + n_parts / 2 + 64;
  w.parts = 0;
  int rc;
  if ((rc = grow(&w.d_cand, n, false)) || (rc = grow(&w.d_meas, n + 1, false)) || (rc = grow(&w.h_cand, n, true)) ||
      (rc = grow(&w.h_meas, n + 1, true)))
    return rc;
  w.parts = n;
  return BC_OK;
}

int reserve_segs(Work& w, uint32_t n_segs, uint32_t n_slices, uint64_t n_sym) {
  int rc;
  if (n_segs > w.segs) {
    const uint32_t n = n_segs + n_segs / 2 + 64;
    w.segs = 0;
    if ((rc = grow(&w.d_segs, n, false)) || (rc = grow(&w.d_status, 2ull * n + 1, false)) || (rc = grow(&w.h_status, 2ull * n + 1, true)))
      return rc;
    w.segs = n;
  }
  if (n_slices > w.slices) {
    const uint32_t n = n_slices + n_slices / 2 + 64;
    w.slices = 0;
    if ((rc = grow(&w.d_slices, n, false))) return rc;
    w.slices = n;
  }
  if (n_sym > w.sym) {
    w.sym = 0;
    if ((rc = grow(&w.d_sym, n_sym + 64, false))) return rc;
    w.sym = n_sym;
  }
  return BC_OK;
}

}  // namespace

int gunzip_span(int device_id, void* hip_stream, const void* d_src, uint64_t src_bytes, uint64_t start_bit, const void* d_history,
                uint32_t history_bytes, void* d_text, uint64_t text_capacity, uint32_t part_bytes, bc_gunzip_result* res) {
  memset(res, 0, sizeof *res);
  res->end_bit = start_bit;
  if (part_bytes == 0) part_bytes = 32768;
  if (part_bytes < 64 || (part_bytes & 7u)) {
    set_error("bc_gunzip_span_device: part_bytes must be a multiple of 8, at least 64");
    return BC_ERR_INVALID;
  }
  if (src_bytes >= (1ull << 28) || start_bit > 8 * src_bytes) {
    set_error("bc_gunzip_span_device: a span holds less than 256 MiB and starts inside its bytes");
    return BC_ERR_INVALID;
  }
  if (!d_history) history_bytes = 0;
  if (history_bytes > kGzHistory) history_bytes = kGzHistory;
  if ((src_bytes && !d_src) || (text_capacity && !d_text)) {
    set_error("bc_gunzip_span_device: null buffer");
    return BC_ERR_INVALID;
  }
  const uint32_t src_len = (uint32_t)src_bytes, capacity = (uint32_t)std::min<uint64_t>(text_capacity, 0x7FFFFFFFull);
  const uint32_t n_parts = (src_len + part_bytes - 1) / part_bytes;
  hipStream_t st = (hipStream_t)hip_stream;
  std::lock_guard<std::mutex> lk(g_mu);
  Work& w = g_work;
  HIP_TRY(hipSetDevice(device_id));
  if (w.device != device_id) {  // (buffers of another device: let go of them)
    if (w.device >= 0 && hipSetDevice(w.device) == hipSuccess) {
      for (void* p : {(void*)w.d_cand, (void*)w.d_meas, (void*)w.d_segs, (void*)w.d_slices, (void*)w.d_status, (void*)w.d_sym})
        if (p) (void)hipFree(p);
      for (void* p : {(void*)w.h_cand, (void*)w.h_meas, (void*)w.h_status})
        if (p) (void)hipHostFree(p);
      HIP_TRY(hipSetDevice(device_id));
    }
    w = Work();
    w.device = device_id;
  }
  int rc = reserve_parts(w, n_parts);
  if (rc != BC_OK) return rc;
  const uint32_t groups = (n_parts + 1 + kWavesPerGroup - 1) / kWavesPerGroup;
  if (n_parts)
    hipLaunchKernelGGL(gunzip_find_kernel, dim3((n_parts + kWavesPerGroup - 1) / kWavesPerGroup), dim3(64 * kWavesPerGroup), 0, st,
                       (const uint8_t*)d_src, src_len, (uint32_t)start_bit, part_bytes, n_parts, w.d_cand);
  hipLaunchKernelGGL(gunzip_measure_kernel, dim3(groups), dim3(64 * kWavesPerGroup), 0, st, (const uint8_t*)d_src, src_len,
                     (uint32_t)start_bit, part_bytes, n_parts, w.d_cand, capacity, w.d_meas);
  HIP_TRY(hipGetLastError());
  if (n_parts) HIP_TRY(hipMemcpyAsync(w.h_cand, w.d_cand, n_parts * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(w.h_meas, w.d_meas, (n_parts + 1ull) * sizeof(GzMeasure), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));

  GzChain c = gunzip_chain((uint32_t)start_bit, w.h_cand, n_parts, w.h_meas, capacity);
  res->status = c.status;
  res->detail = c.detail;
  res->text_bytes = c.text_bytes;
  res->end_bit = c.end_bit;
  res->member_end = c.member_end;
  res->segments = (uint32_t)c.segs.size();
  res->rejected = c.rejected;
  if (c.status != kGzOk || c.segs.empty()) return BC_OK;  // (output full: nothing is written; the caller cuts the span)

  const uint32_t n_segs = (uint32_t)c.segs.size(), n_slices = (uint32_t)c.slices.size();
  if ((rc = reserve_segs(w, n_segs, n_slices, c.text_bytes)) != BC_OK) return rc;
  uint32_t* d_crc = w.d_status + n_segs;
  uint32_t* d_bad = w.d_status + 2ull * n_segs;
  HIP_TRY(hipMemcpyAsync(w.d_segs, c.segs.data(), n_segs * sizeof(GzSegment), hipMemcpyHostToDevice, st));
  if (n_slices) HIP_TRY(hipMemcpyAsync(w.d_slices, c.slices.data(), n_slices * sizeof(GzSlice), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(w.d_status, 0, (2ull * n_segs + 1) * sizeof(uint32_t), st));
  hipLaunchKernelGGL(gunzip_decode_kernel, dim3((n_segs + kWavesPerGroup - 1) / kWavesPerGroup), dim3(64 * kWavesPerGroup), 0, st,
                     (const uint8_t*)d_src, src_len, w.d_segs, n_segs, (const uint8_t*)d_history, history_bytes, w.d_sym, w.d_status);
  hipLaunchKernelGGL(gunzip_resolve_tails_kernel, dim3(1), dim3(kSeqThreads), 0, st, w.d_segs, n_segs, w.d_sym, (uint8_t*)d_text,
                     (const uint8_t*)d_history, history_bytes, d_bad);
  if (n_slices)
    hipLaunchKernelGGL(gunzip_resolve_kernel, dim3((n_slices + kWavesPerGroup - 1) / kWavesPerGroup), dim3(64 * kWavesPerGroup), 0, st,
                       w.d_segs, w.d_slices, n_slices, w.d_sym, (uint8_t*)d_text, (const uint8_t*)d_history, history_bytes, d_crc, d_bad);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(w.h_status, w.d_status, (2ull * n_segs + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  uint32_t crc = 0;
  for (uint32_t s = 0; s < n_segs; ++s) {
    if (w.h_status[s] != kInfOk && res->status == kGzOk) {
      res->status = kGzBadStream;
      res->detail = w.h_status[s];
    }
    crc = gunzip_crc_combine(crc, w.h_status[n_segs + s], c.segs[s].out_bytes);
  }
  if (w.h_status[2ull * n_segs] && res->status == kGzOk) {
    res->status = kGzBadStream;
    res->detail = kInfBadSymbol;
  }
  res->crc32 = crc;
  if (res->status != kGzOk) {
    res->text_bytes = 0;
    res->end_bit = start_bit;
    res->member_end = 0;
    res->segments = 0;
    res->crc32 = 0;
  }
  return BC_OK;
}

}  // namespace bc

extern "C" int bc_gunzip_span_device(int device_id, void* hip_stream, const void* d_src, uint64_t src_bytes, uint64_t start_bit,
                                     const void* d_history, void* d_text, uint64_t text_capacity, uint32_t part_bytes,
                                     bc_gunzip_result* result) {
  if (!result) {
    bc::set_error("bc_gunzip_span_device: null result");
    return BC_ERR_INVALID;
  }
  return bc::gunzip_span(device_id, hip_stream, d_src, src_bytes, start_bit, d_history, d_history ? bc::kGzHistory : 0u, d_text, text_capacity,
                         part_bytes, result);
}
