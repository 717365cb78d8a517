// TEST-ONLY: the order of multi-word keys (csrc/bc_sort.h, bc::sort_words_launch) on buffers the caller owns, through the
// entry point the wide-key renderer uses.  Built and bound by tests/test_gpu_sort_words.py; every pointer is a device
// pointer (torch tensors).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_sort.h"

extern "C" {

uint64_t sort_words_harness_tile(void) { return bc::kSortTile; }

uint64_t sort_words_harness_scratch_words(uint64_t n) { return bc::sort_scratch_words(n); }

// one sort on the null stream, then waits for it: perm holds the order.  words: K columns of n u64.  Returns the
// hipError_t.
int sort_words_harness_run(const void* words, uint32_t K, uint64_t n, void* perm, void* col, void* col_tmp, void* perm_tmp,
                           void* scratch, uint32_t* live_passes) {
  const hipError_t rc = bc::sort_words_launch(nullptr, static_cast<const uint64_t*>(words), K, n, static_cast<uint32_t*>(perm),
                                              static_cast<uint64_t*>(col), static_cast<uint64_t*>(col_tmp),
                                              static_cast<uint32_t*>(perm_tmp), static_cast<uint32_t*>(scratch), live_passes);
  if (rc != hipSuccess) return (int)rc;
  return (int)hipDeviceSynchronize();
}

}  // extern "C"
