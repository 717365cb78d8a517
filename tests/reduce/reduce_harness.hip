// TEST-ONLY: the run reduction (csrc/bc_reduce.h) on buffers the caller owns, through the entry point the engine uses
// (bc::reduce_runs_launch).  Built and bound by tests/test_gpu_reduce.py; every pointer is a device pointer (torch tensors).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_reduce.h"

extern "C" {

// the reduction's constants, so that the tests cannot drift from the header
void reduce_harness_constants(uint64_t out[4]) {
  out[0] = bc::kReduceTile;
  out[1] = bc::kReduceWaves;
  out[2] = bc::kReduceChunks;
  out[3] = 0;
}

uint64_t reduce_harness_scratch_words(uint64_t n) { return bc::reduce_scratch_words(n); }

// one reduction on the null stream, then waits for it.  Returns the hipError_t.
int reduce_harness_run(const void* keys, const void* vals, uint64_t n, void* out_keys, void* out_sums, void* n_runs,
                       void* scratch) {
  const hipError_t rc = bc::reduce_runs_launch(nullptr, static_cast<const uint64_t*>(keys), static_cast<const uint32_t*>(vals), n,
                                               static_cast<uint64_t*>(out_keys), static_cast<uint64_t*>(out_sums),
                                               static_cast<uint32_t*>(n_runs), static_cast<uint32_t*>(scratch));
  if (rc != hipSuccess) return (int)rc;
  return (int)hipDeviceSynchronize();
}

}  // extern "C"
