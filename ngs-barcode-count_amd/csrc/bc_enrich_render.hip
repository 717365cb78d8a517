// bc_enrich_render.hip -- the Single and Double enrichment files of a dense plan as CSV text, written on the device
// (bc_engine_render_enriched, bc_engine_render_enriched_merged; the line format and the lane-level code are
// bc_enrich_render.h, the kernels bc_text_kernels.h), and the fold of keys that share their IDs.
#include "bc_enrich_render.h"
#include "bc_text_kernels.h"

namespace {

// One key per lane, grid-stride over S * K entries.  A key that is not canonical moves its sum to the canonical one: an
// entry is either only added to (canonical) or only read and zeroed by its own lane (the others), so no order matters.
__global__ __launch_bounds__(256) void enrich_fold_kernel(bc::EnrichRenderView v, uint64_t n_samples) {
  unsigned long long* sums = const_cast<unsigned long long*>(v.sums);
  const uint64_t total = n_samples * v.K, step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
    const unsigned long long x = sums[e];
    if (!x) continue;
    const uint64_t s = e / v.K, k = e - s * v.K;
    const uint64_t t = bc::enrich_fold_target(v, k);
    if (t == k) continue;
    atomicAdd(sums + s * v.K + t, x);
    sums[e] = 0ull;
  }
}

}  // namespace

hipError_t bc_enrich_render_sizes_launch(const bc::EnrichRenderView& v, uint64_t n_blocks, uint32_t* d_rows,
                                         unsigned long long* d_bytes, hipStream_t stream) {
  return bc::text_sizes_launch(v, n_blocks, d_rows, d_bytes, stream);
}

hipError_t bc_enrich_render_lens_launch(const bc::EnrichRenderView& v, uint64_t lo, uint32_t n, uint32_t* d_len,
                                        hipStream_t stream) {
  return bc::text_lens_launch(v, lo, n, d_len, stream);
}

hipError_t bc_enrich_render_write_launch(const bc::EnrichRenderView& v, uint64_t b0, uint64_t n_blocks, uint64_t lo, uint64_t hi,
                                         const uint32_t* d_rows, const unsigned long long* d_prefix, uint64_t sub, uint8_t* d_out,
                                         uint64_t out_cap, hipStream_t stream) {
  return bc::text_write_launch(v, b0, n_blocks, lo, hi, d_rows, d_prefix, sub, d_out, out_cap, stream);
}

hipError_t bc_enrich_fold_launch(const bc::EnrichRenderView& v, uint64_t n_samples, hipStream_t stream) {
  const uint64_t total = n_samples * v.K;
  if (total == 0 || !v.canon) return hipSuccess;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255) / 256, 256ull * 32);
  hipLaunchKernelGGL(enrich_fold_kernel, dim3(grid), dim3(256), 0, stream, v, n_samples);
  return hipGetLastError();
}
