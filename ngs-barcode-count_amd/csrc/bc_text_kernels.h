// bc_text_kernels.h -- the kernels that turn a key space into text lines, for every view that has lane code for it
// (bc_render.h: the counts files; bc_enrich_render.h: the Single / Double files; bc_raw_render.h: the counts files of a
// raw-key plan; bc_wide_render.h: those of a wide-key plan; bc_raw_enrich_render.h: the Single / Double files of a
// raw-key plan -- all five written with bc_line.h).  A view V gives, in namespace bc,
//     text_keys(v)                         the number of keys
//     text_line_len(v, k)                  bytes of key k's line, 0: no line
//     text_line_write(v, k, len, dst, at, win)   the part of the line inside a window
// Device code and its launchers, all enqueueing on `stream`; included by bc_text.hip, which instantiates them for the
// five views.
//
// A workgroup of four wavefronts owns a block of 1024 consecutive keys, a wavefront four chunks of 64 (one key per
// lane, so every column's read is coalesced).  Chunks without a line are skipped by ballot.
//   pass 1 (text_sizes_kernel)  lines and text bytes per block; the host scans them and cuts the key space at block
//                               boundaries into ranges whose text fits one staging buffer.
//   pass 2 (text_write_kernel)  per range: a wavefront's chunk totals -> LDS, so every chunk knows where its text
//                               starts (block start from the host's scan + the chunks before it); a lane writes its
//                               line into the wavefront's LDS window at its scanned offset, then the wavefront copies
//                               the window out with lanes on consecutive dwords.  The window is laid out with the
//                               destination's alignment (text starts at byte `dst & 3` of it), so whole dwords go
//                               LDS -> global and only the first and last few bytes are byte stores.  A chunk whose
//                               text exceeds the window (long IDs) takes several windows.
// LDS: 4 x 4 KB windows + 64 B of chunk totals per workgroup.
#ifndef BC_TEXT_KERNELS_H
#define BC_TEXT_KERNELS_H

#include <algorithm>

#include "bc_intrin.h"

namespace bc {

constexpr uint32_t kRenderBlock = 1024;       // a block: as many consecutive keys
constexpr uint32_t kWaves = 4, kChunks = 4;   // wavefronts per workgroup, chunks per wavefront
constexpr uint32_t kWinBytes = 4096;           // one wavefront's staging window
static_assert(kWaves * kChunks * 64 == kRenderBlock, "a workgroup owns one block");

__device__ __forceinline__ uint32_t wave_sum32(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
  return x;
}

// exclusive prefix sum over the wavefront's lanes
__device__ __forceinline__ uint32_t wave_excl32(uint32_t x, uint32_t lane) {
  uint32_t s = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)s, o);
    if (lane >= (uint32_t)o) s += y;
  }
  return s - x;
}

template <class View>
__global__ __launch_bounds__(256) void text_sizes_kernel(View v, uint64_t n_blocks, uint32_t* __restrict__ rows,
                                                         unsigned long long* __restrict__ bytes) {
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
#pragma unroll
    for (uint32_t k = 0; k < kChunks; ++k) {
      const uint64_t t = b * kRenderBlock + (uint64_t)(wave * kChunks + k) * 64 + lane;
      const uint32_t len = t < text_keys(v) ? text_line_len(v, t) : 0u;
      const unsigned long long m = __ballot(len != 0u);
      if (m == 0ull) continue;
      const uint32_t tot = wave_sum32(len);
      if (lane == 0) {
        atomicAdd(rows + b, (uint32_t)__popcll(m));
        atomicAdd(bytes + b, (unsigned long long)tot);
      }
    }
  }
}

template <class View>
__global__ __launch_bounds__(256) void text_lens_kernel(View v, uint64_t lo, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = lo + i < text_keys(v) ? text_line_len(v, lo + i) : 0u;
}

template <class View>
__global__ __launch_bounds__(256) void text_write_kernel(View v, uint64_t b0, uint64_t lo, uint64_t hi,
                                                         const uint32_t* __restrict__ rows,
                                                         const unsigned long long* __restrict__ prefix, uint64_t sub,
                                                         uint8_t* __restrict__ out, uint64_t out_cap) {
  __shared__ uint32_t chunk_total[kWaves * kChunks];
  __shared__ uint32_t window[kWaves][kWinBytes / 4];
  const uint64_t b = b0 + blockIdx.x;
  if (rows[b] == 0u) return;  // (the whole workgroup)
  const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
  uint32_t len[kChunks];
#pragma unroll
  for (uint32_t k = 0; k < kChunks; ++k) {
    const uint64_t t = b * kRenderBlock + (uint64_t)(wave * kChunks + k) * 64 + lane;
    len[k] = t >= lo && t < hi ? text_line_len(v, t) : 0u;
    const uint32_t tot = wave_sum32(len[k]);
    if (lane == 0) chunk_total[wave * kChunks + k] = tot;
  }
  __syncthreads();
  uint64_t off = prefix[b] - sub;  // where this wavefront's text starts in `out`
  for (uint32_t c = 0; c < wave * kChunks; ++c) off += chunk_total[c];
  uint8_t* wb = (uint8_t*)window[wave];
  const uint32_t* wd = window[wave];
#pragma unroll
  for (uint32_t k = 0; k < kChunks; ++k) {
    const uint32_t L = len[k];
    const uint32_t tot = chunk_total[wave * kChunks + k];
    if (tot == 0u) continue;
    const uint64_t t = b * kRenderBlock + (uint64_t)(wave * kChunks + k) * 64 + lane;
    // window coordinates: byte q of the chunk's text sits at pad + q, so that it and out[off + q] agree modulo 4
    const uint32_t pad = (uint32_t)(off & 3u);
    const uint64_t gbase = off - pad;                  // out position of window coordinate 0: a multiple of 4
    const uint32_t start = pad + wave_excl32(L, lane);  // of this lane's line
    const uint32_t end_all = pad + tot;
    for (uint32_t w0 = 0; w0 < end_all; w0 += kWinBytes) {
      if (L && start < w0 + kWinBytes && start + L > w0) text_line_write(v, t, L, wb, (int64_t)start - (int64_t)w0, kWinBytes);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint32_t a = w0 > pad ? w0 : pad, e = end_all < w0 + kWinBytes ? end_all : w0 + kWinBytes;
      const uint32_t a4 = (a + 3u) & ~3u, e4 = e & ~3u;
      if (a4 >= e4) {
        for (uint32_t j = a + lane; j < e; j += 64)
          if (gbase + j < out_cap) out[gbase + j] = wb[j - w0];
      } else {
        if (a + lane < a4 && gbase + a + lane < out_cap) out[gbase + a + lane] = wb[a + lane - w0];
        uint32_t* out32 = (uint32_t*)(out + gbase);
        for (uint32_t q = (a4 >> 2) + lane; q < (e4 >> 2); q += 64)
          if (gbase + 4ull * q + 4 <= out_cap) out32[q] = wd[q - (w0 >> 2)];
        if (e4 + lane < e && gbase + e4 + lane < out_cap) out[gbase + e4 + lane] = wb[e4 + lane - w0];
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    off += tot;
  }
}

// pass 1: lines and text bytes of every block (both arrays zeroed by the caller)
template <class View>
hipError_t text_sizes_launch(const View& v, uint64_t n_blocks, uint32_t* d_rows, unsigned long long* d_bytes,
                             hipStream_t stream) {
  if (n_blocks == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(n_blocks, 256ull * 32);
  hipLaunchKernelGGL(text_sizes_kernel<View>, dim3(grid), dim3(256), 0, stream, v, n_blocks, d_rows, d_bytes);
  return hipGetLastError();
}

// the line length of keys lo .. lo + n - 1 (0: no line), for a block whose text has to be cut inside
template <class View>
hipError_t text_lens_launch(const View& v, uint64_t lo, uint32_t n, uint32_t* d_len, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(text_lens_kernel<View>, dim3((n + 255) / 256), dim3(256), 0, stream, v, lo, n, d_len);
  return hipGetLastError();
}

// pass 2: the lines of keys [lo, hi) inside blocks b0 .. b0 + n_blocks - 1 into d_out; the text of block b starts at
// d_prefix[b] - sub (d_prefix: exclusive scan of pass 1's bytes; keys outside [lo, hi) take no room), nothing is stored
// at or beyond out_cap
template <class View>
hipError_t text_write_launch(const View& v, uint64_t b0, uint64_t n_blocks, uint64_t lo, uint64_t hi,
                             const uint32_t* d_rows, const unsigned long long* d_prefix, uint64_t sub, uint8_t* d_out,
                             uint64_t out_cap, hipStream_t stream) {
  // (a grid dimension holds 2^31 - 1 workgroups: longer ranges go in slices)
  const uint64_t slice = 1ull << 30;
  for (uint64_t s = 0; s < n_blocks; s += slice) {
    const uint32_t grid = (uint32_t)std::min(slice, n_blocks - s);
    hipLaunchKernelGGL(text_write_kernel<View>, dim3(grid), dim3(256), 0, stream, v, b0 + s, lo, hi, d_rows, d_prefix, sub, d_out,
                       out_cap);
    const hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}

}  // namespace bc

#endif
