// bc_raw_render.hip -- the counts files of a raw-key plan as CSV text, written on the device
// (bc_engine_render_raw_counts, bc_engine_render_raw_merged; the order, the line format and the lane-level code are
// bc_raw_render.h, the kernels bc_text_kernels.h), and the re-key step in front of the sort that makes the order.
#include "bc_raw_render.h"
#include "bc_text_kernels.h"

namespace bc {

// key = s * t_space + T  ->  T * S + s: the same digits, the sample's moved to the least significant place
__global__ __launch_bounds__(256) void raw_rekey_kernel(unsigned long long* __restrict__ keys, uint64_t n, uint64_t t_space,
                                                        uint32_t S) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const unsigned long long k = keys[i];
    const unsigned long long s = k / t_space;
    keys[i] = (k - s * t_space) * S + s;
  }
}

}  // namespace bc

hipError_t bc_raw_rekey_launch(uint64_t* d_keys, uint64_t n, uint64_t t_space, uint32_t S, hipStream_t stream) {
  if (n == 0 || S <= 1 || t_space == 0) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, 256ull * 32);
  hipLaunchKernelGGL(bc::raw_rekey_kernel, dim3(grid), dim3(256), 0, stream, (unsigned long long*)d_keys, n, t_space, S);
  return hipGetLastError();
}

hipError_t bc_raw_render_sizes_launch(const bc::RawRenderView& v, uint64_t n_blocks, uint32_t* d_rows,
                                      unsigned long long* d_bytes, hipStream_t stream) {
  return bc::text_sizes_launch(v, n_blocks, d_rows, d_bytes, stream);
}

hipError_t bc_raw_render_lens_launch(const bc::RawRenderView& v, uint64_t lo, uint32_t n, uint32_t* d_len, hipStream_t stream) {
  return bc::text_lens_launch(v, lo, n, d_len, stream);
}

hipError_t bc_raw_render_write_launch(const bc::RawRenderView& v, uint64_t b0, uint64_t n_blocks, uint64_t lo, uint64_t hi,
                                      const uint32_t* d_rows, const unsigned long long* d_prefix, uint64_t sub, uint8_t* d_out,
                                      uint64_t out_cap, hipStream_t stream) {
  return bc::text_write_launch(v, b0, n_blocks, lo, hi, d_rows, d_prefix, sub, d_out, out_cap, stream);
}
