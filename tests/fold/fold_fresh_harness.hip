// TEST-ONLY: the count-log fold (csrc/bc_fold.h) in its fresh mode -- the bit map counts as all zero whatever memory
// holds, and the fold writes every word of it -- on buffers the caller owns.  Built and bound by
// tests/test_gpu_fold_fresh.py; every pointer is a device pointer (torch tensors).  The ordinary mode:
// tests/fold/fold_harness.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_kernel.h"
#include "bc_fold.h"

extern "C" {

// one fold of log[0, n) on the null stream, then waits for it.  scatter_grid / apply_grid: 0 = the engine's sizing;
// fresh: 0 = the ordinary fold.  Returns the hipError_t.
int fold_fresh_harness_run(const void* log, uint64_t n, void* grouped, void* meta, uint32_t nb, void* bits, uint64_t n_words,
                           void* table, void* dirty, uint32_t scatter_grid, uint32_t apply_grid, int fresh) {
  int dev = 0;
  hipError_t rc = hipGetDevice(&dev);
  if (rc != hipSuccess) return (int)rc;
  int n_cus = 0;
  rc = hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (rc != hipSuccess) return (int)rc;
  rc = bc::fold_launch(nullptr, static_cast<const uint32_t*>(log), n, static_cast<uint32_t*>(grouped), static_cast<uint32_t*>(meta),
                       nb, static_cast<uint32_t*>(bits), n_words, static_cast<uint32_t*>(table), static_cast<uint8_t*>(dirty),
                       (uint32_t)n_cus, scatter_grid, apply_grid, fresh != 0);
  if (rc != hipSuccess) return (int)rc;
  return (int)hipDeviceSynchronize();
}

}  // extern "C"
