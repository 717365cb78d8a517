// TEST-ONLY: bc::fold_apply_unit (csrc/bc_fold.h), the walk of bc_fold_apply's workgroups over (item, quarter), on the
// host.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run by tests/test_fold_unit_map.py.
// For every grid in 1..600 and every number of items of the list below: each workgroup walks its steps until a unit is
// not valid, as the kernel does; every (item < n_items, quarter < kFoldQuarters) must come up exactly once and nothing
// else; a workgroup's items rise with its steps (the kernel stops at the first unit that is not valid); and for a grid
// that is a multiple of 32 the four quarters of an item sit on blocks congruent mod 8, in the same step.
// Prints one line per failure and "ok <grids> <cases>" at the end; exit status 1 on any failure.
#include <stdio.h>

#include <vector>

#include "bc_fold.h"

int main() {
  const uint32_t items_list[] = {0, 1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 1400};
  const uint32_t kQ = bc::kFoldQuarters;
  unsigned long failures = 0, cases = 0;
  auto fail = [&](const char* what, uint32_t grid, uint32_t n_items, uint32_t a, uint32_t b) {
    if (++failures <= 20) printf("FAIL %s: grid %u items %u (%u, %u)\n", what, grid, n_items, a, b);
  };
  for (uint32_t grid = 1; grid <= 600; ++grid) {
    for (uint32_t n_items : items_list) {
      ++cases;
      std::vector<uint32_t> seen((size_t)n_items * kQ, 0u), block_of((size_t)n_items * kQ, 0u), step_of((size_t)n_items * kQ, 0u);
      for (uint32_t block = 0; block < grid; ++block) {
        uint32_t last_item = 0;
        for (uint32_t step = 0;; ++step) {
          const bc::FoldUnit u = bc::fold_apply_unit(block, grid, step, n_items);
          if (!u.valid) {
            // nothing valid may follow: the kernel has stopped here
            for (uint32_t more = 1; more <= 3; ++more)
              if (bc::fold_apply_unit(block, grid, step + more, n_items).valid) fail("valid after the end", grid, n_items, block, step + more);
            break;
          }
          if (u.item >= n_items || u.quarter >= kQ) {
            fail("outside", grid, n_items, u.item, u.quarter);
            break;
          }
          if (step && u.item < last_item) fail("items fall", grid, n_items, block, step);
          last_item = u.item;
          const size_t at = (size_t)u.item * kQ + u.quarter;
          ++seen[at];
          block_of[at] = block;
          step_of[at] = step;
          if (step > n_items * kQ + 1u) {
            fail("no end", grid, n_items, block, step);
            break;
          }
        }
      }
      for (uint32_t item = 0; item < n_items; ++item)
        for (uint32_t q = 0; q < kQ; ++q) {
          const size_t at = (size_t)item * kQ + q;
          if (seen[at] != 1u) fail("not exactly once", grid, n_items, item, q);
          if (grid % 32u == 0u && seen[at] == 1u && seen[(size_t)item * kQ] == 1u) {
            if (block_of[at] % 8u != block_of[(size_t)item * kQ] % 8u) fail("siblings not congruent mod 8", grid, n_items, item, q);
            if (step_of[at] != step_of[(size_t)item * kQ]) fail("siblings in different steps", grid, n_items, item, q);
          }
        }
    }
  }
  printf("ok %u %lu\n", 600u, cases);
  return failures ? 1 : 0;
}
