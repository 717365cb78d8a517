// bc_render.hip -- the counts files of a dense plan as CSV text, written on the device (bc_engine_render_counts,
// bc_engine_render_merged; the line format and the lane-level code are bc_render.h, the kernels bc_text_kernels.h).
#include "bc_text_kernels.h"

hipError_t bc_render_sizes_launch(const bc::RenderView& v, uint64_t n_blocks, uint32_t* d_rows, unsigned long long* d_bytes,
                                  hipStream_t stream) {
  return bc::text_sizes_launch(v, n_blocks, d_rows, d_bytes, stream);
}

hipError_t bc_render_lens_launch(const bc::RenderView& v, uint64_t lo, uint32_t n, uint32_t* d_len, hipStream_t stream) {
  return bc::text_lens_launch(v, lo, n, d_len, stream);
}

hipError_t bc_render_write_launch(const bc::RenderView& v, uint64_t b0, uint64_t n_blocks, uint64_t lo, uint64_t hi,
                                  const uint32_t* d_rows, const unsigned long long* d_prefix, uint64_t sub, uint8_t* d_out,
                                  uint64_t out_cap, hipStream_t stream) {
  return bc::text_write_launch(v, b0, n_blocks, lo, hi, d_rows, d_prefix, sub, d_out, out_cap, stream);
}
