// TEST-ONLY: the count-log fold (csrc/bc_fold.h) on buffers the caller owns, through the launch sequence the engine's
// fold_log() uses.  Built and bound by tests/test_gpu_fold.py; every pointer is a device pointer (torch tensors).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_kernel.h"
#include "bc_fold.h"

extern "C" {

// the fold's constants, so that the tests cannot drift from the header
void fold_harness_constants(uint64_t out[8]) {
  out[0] = bc::kLogNone;
  out[1] = bc::kFoldBucketShift;
  out[2] = bc::kFoldQuarterShift;
  out[3] = bc::kFoldMaxBuckets;
  out[4] = bc::kFoldTile;
  out[5] = bc::kFoldChunk;
  out[6] = 0;
  out[7] = 0;
}

// one fold of log[0, n) on the null stream, then waits for it.  scatter_grid / apply_grid: 0 = the engine's sizing.
// Returns the hipError_t.
int fold_harness_run(const void* log, uint64_t n, void* grouped, void* meta, uint32_t nb, void* bits, uint64_t n_words,
                     void* table, void* dirty, uint32_t scatter_grid, uint32_t apply_grid) {
  int dev = 0;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return (int)rc;
  int n_cus = 0;
  rc = hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (rc != hipSuccess) return (int)rc;
  rc = bc::fold_launch(nullptr, static_cast<const uint32_t*>(log), n, static_cast<uint32_t*>(grouped), static_cast<uint32_t*>(meta),
                       nb, static_cast<uint32_t*>(bits), n_words, static_cast<uint32_t*>(table), static_cast<uint8_t*>(dirty),
                       (uint32_t)n_cus, scatter_grid, apply_grid);
  if (rc != hipSuccess) return (int)rc;
  return (int)hipDeviceSynchronize();
}

}  // extern "C"
