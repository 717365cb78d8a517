// bc_enrich.h -- single and double barcode enrichment (bc_engine_enrich, ResultsEnrichment of info.rs:811-904) as
// marginal sums of the dense (sample, barcode tuple) table: the launcher bc_finish.hip calls, the kernel is
// bc_enrich.hip.
#ifndef BC_ENRICH_H
#define BC_ENRICH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_device_plan.h"

constexpr int kEnrichMaxG = bc::kMaxGroups;  // counted barcodes: as many as a plan may have groups
constexpr int kEnrichMaxPairs = kEnrichMaxG * (kEnrichMaxG - 1) / 2;

// The table's shape and the outputs' layout (include/barcode_count_hip.h, bc_engine_enrich).  Entry
// s * inner + sum_g d_g * prod_{k>g} n_k holds the count of sample s and digits d_0 .. d_{G-1} (the last counted barcode
// is the innermost axis, as bc_engine_decode_index reads it).
struct EnrichShape {
  uint32_t G;                              // counted barcodes, 1 .. kEnrichMaxG
  uint32_t n[kEnrichMaxG];                 // N_g: size of known set g
  uint64_t inner;                          // prod N_g: entries per sample
  uint64_t sum_n;                          // sum N_g: singles per sample
  uint64_t pairs;                          // P = sum_{g<h} N_g * N_h: doubles per sample
  uint64_t single_off[kEnrichMaxG];        // off_g = sum_{k<g} N_k
  uint64_t pair_off[kEnrichMaxPairs];      // poff of pair p, pairs in add_double's order (0,1), (0,2), .., (1,2), ..
};

// the number of pair (g, h), g < h, in that order
__host__ __device__ constexpr int enrich_pair_index(int G, int g, int h) { return g * (2 * G - g - 1) / 2 + (h - g - 1); }

// Adds the marginals of table (+ bit map, when two-level counting has not been folded; may be NULL) to single[] and,
// when d_double is not NULL, to double[] (both zeroed by the caller, u64).  Enqueued on `stream`.
hipError_t bc_enrich_launch(const EnrichShape& sh, const uint32_t* d_table, const uint32_t* d_bits, uint64_t entries,
                            unsigned long long* d_single, unsigned long long* d_double, hipStream_t stream);

#endif
