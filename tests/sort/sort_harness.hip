// TEST-ONLY: the pair sort (csrc/bc_sort.h) on buffers the caller owns, through the entry point the engine uses
// (bc::sort_pairs_launch).  Built and bound by tests/test_gpu_sort.py; every pointer is a device pointer (torch tensors).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_sort.h"

extern "C" {

// the sort's constants, so that the tests cannot drift from the header
void sort_harness_constants(uint64_t out[4]) {
  out[0] = bc::kSortTile;
  out[1] = bc::kSortBits;
  out[2] = bc::kSortMaxPasses;
  out[3] = 0;
}

uint64_t sort_harness_scratch_words(uint64_t n) { return bc::sort_scratch_words(n); }

// one sort on the null stream, then waits for it: the sorted pairs are in keys / vals.  Returns the hipError_t.
int sort_harness_run(void* keys, void* vals, void* keys_tmp, void* vals_tmp, uint64_t n, uint32_t key_bits, void* scratch,
                     uint32_t* live_passes) {
  const hipError_t rc = bc::sort_pairs_launch(nullptr, static_cast<uint64_t*>(keys), static_cast<uint32_t*>(vals),
                                              static_cast<uint64_t*>(keys_tmp), static_cast<uint32_t*>(vals_tmp), n, key_bits,
                                              static_cast<uint32_t*>(scratch), live_passes);
  if (rc != hipSuccess) return (int)rc;
  return (int)hipDeviceSynchronize();
}

}  // extern "C"
