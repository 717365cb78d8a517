// bc_enrich.hip -- single and double barcode enrichment on the device (bc_engine_enrich).
//
// Every single and pair count of ResultsEnrichment (info.rs:811-904) is a marginal sum of the dense table, so one
// streaming pass over it computes them all.  One wavefront takes 64 consecutive entries at a time (one per lane,
// coalesced); chunks whose 64 counts are all zero are skipped by ballot, as compact_range_kernel does.  64 consecutive
// entries share every digit but the innermost one unless the innermost digit wraps inside the chunk, so in a chunk
// without a wrap the targets that do not involve the innermost group -- the singles of groups 0..G-2 and the pairs
// among them -- get ONE atomic per wavefront with the chunk's sum; only the innermost single and the G-1 pairs
// (g, G-1) take an atomic per non-zero entry, and those land on consecutive addresses.  A chunk with a wrap decodes
// every lane and adds per lane.  All atomics are no-return u64 vector atomics; all index arithmetic is 64-bit (tables
// pass 2^32 entries).
#include "bc_enrich.h"

#include <algorithm>

namespace {

constexpr int kUnroll = 8;  // chunks whose loads a wavefront has in flight at once (2 KB of the table)

__device__ __forceinline__ unsigned long long wave_sum(uint32_t x) {
  uint32_t lo = x, hi = 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, o), h2 = (uint32_t)__shfl_xor((int)hi, o);
    const uint32_t s = lo + l2;
    hi += h2 + (s < lo ? 1u : 0u);
    lo = s;
  }
  return ((unsigned long long)hi << 32) | lo;
}

// one chunk of 64 entries starting at `base` (a multiple of 64, < entries); x = this lane's count; some x != 0
template <int G>
__device__ __forceinline__ void enrich_chunk(const EnrichShape& sh, uint64_t base, uint32_t lane, uint32_t x,
                                             unsigned long long* __restrict__ single, unsigned long long* __restrict__ dbl) {
  // (readfirstlane returns int: through uint32_t, or bit 31 of the low word would sign-extend into the high one)
  base = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) |
         (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)base);
  // the chunk's first entry, decoded as bc_engine_decode_index does
  const uint64_t s = base / sh.inner;
  uint64_t r = base - s * sh.inner;
  uint32_t d[G];
#pragma unroll
  for (int g = G - 1; g >= 0; --g) {
    const uint64_t q = r / sh.n[g];
    d[g] = (uint32_t)(r - q * sh.n[g]);
    r = q;
  }
  const uint32_t ni = sh.n[G - 1];
  if (d[G - 1] + 63u < ni) {
    // no wrap: the lanes differ in the innermost digit alone
    unsigned long long* srow = single + s * sh.sum_n;
    const uint32_t di = d[G - 1] + lane;
    if (x) {
      atomicAdd(srow + sh.single_off[G - 1] + di, (unsigned long long)x);
      if (dbl) {
        unsigned long long* drow = dbl + s * sh.pairs;
#pragma unroll
        for (int g = 0; g < G - 1; ++g)
          atomicAdd(drow + sh.pair_off[enrich_pair_index(G, g, G - 1)] + (uint64_t)d[g] * ni + di, (unsigned long long)x);
      }
    }
    if (G >= 2) {
      const unsigned long long sum = wave_sum(x);
      if (lane == 0) {
#pragma unroll
        for (int g = 0; g < G - 1; ++g) atomicAdd(srow + sh.single_off[g] + d[g], sum);
        if (dbl) {
          unsigned long long* drow = dbl + s * sh.pairs;
#pragma unroll
          for (int g = 0; g < G - 2; ++g)
#pragma unroll
            for (int h = g + 1; h < G - 1; ++h)
              atomicAdd(drow + sh.pair_off[enrich_pair_index(G, g, h)] + (uint64_t)d[g] * sh.n[h] + d[h], sum);
        }
      }
    }
    return;
  }
  // the innermost digit wraps inside the chunk: every lane carries its own offset through the digits
  if (!x) return;
  uint32_t dl[G];
  uint32_t carry = lane;
#pragma unroll
  for (int g = G - 1; g >= 0; --g) {
    const uint32_t t = d[g] + carry;
    carry = t / sh.n[g];
    dl[g] = t - carry * sh.n[g];
  }
  const uint64_t sl = s + carry;  // (< S: x != 0 only for entries inside the table)
  unsigned long long* srow = single + sl * sh.sum_n;
#pragma unroll
  for (int g = 0; g < G; ++g) atomicAdd(srow + sh.single_off[g] + dl[g], (unsigned long long)x);
  if (dbl) {
    unsigned long long* drow = dbl + sl * sh.pairs;
#pragma unroll
    for (int g = 0; g < G - 1; ++g)
#pragma unroll
      for (int h = g + 1; h < G; ++h)
        atomicAdd(drow + sh.pair_off[enrich_pair_index(G, g, h)] + (uint64_t)dl[g] * sh.n[h] + dl[h], (unsigned long long)x);
  }
}

// Persistent grid-stride pass: wavefront w takes chunks w*kUnroll .. w*kUnroll+kUnroll-1, then jumps by the grid.  The
// count of entry i is table[i] + bit i of the bit map (two-level counting, read as it stands, like compact_range_kernel).
template <int G>
__global__ __launch_bounds__(256) void enrich_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ bits,
                                                     uint64_t entries, EnrichShape sh, unsigned long long* __restrict__ single,
                                                     unsigned long long* __restrict__ dbl) {
  const uint32_t lane = __lane_id();
  const uint64_t n_chunks = (entries + 63) >> 6;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t step = (uint64_t)gridDim.x * (blockDim.x >> 6) * kUnroll;
  // (every lane of a wavefront runs the same number of rounds: the ballot and the shuffles need them all)
  for (uint64_t c0 = wave * kUnroll; c0 < n_chunks; c0 += step) {
    uint32_t v[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const uint64_t i = ((c0 + k) << 6) + lane;
      v[k] = 0u;
      if (i < entries) v[k] = table[i] + (bits ? (bits[i >> 5] >> (i & 31)) & 1u : 0u);
    }
#pragma unroll 1
    for (int k = 0; k < kUnroll; ++k) {
      const uint32_t x = v[0];
#pragma unroll
      for (int j = 0; j + 1 < kUnroll; ++j) v[j] = v[j + 1];  // (a shift, not v[k]: no dynamic register indexing)
      if (__ballot(x != 0u) == 0ull) continue;
      enrich_chunk<G>(sh, (c0 + k) << 6, lane, x, single, dbl);
    }
  }
}

template <int G>
hipError_t launch_g(const EnrichShape& sh, const uint32_t* table, const uint32_t* bits, uint64_t entries,
                    unsigned long long* single, unsigned long long* dbl, hipStream_t stream) {
  const uint64_t per_block = 256ull * kUnroll;  // entries a workgroup of four wavefronts takes per round
  const uint32_t grid = (uint32_t)std::min<uint64_t>((entries + per_block - 1) / per_block, 256ull * 32);
  hipLaunchKernelGGL(enrich_kernel<G>, dim3(grid), dim3(256), 0, stream, table, bits, entries, sh, single, dbl);
  return hipGetLastError();
}

template <int G>
hipError_t dispatch(const EnrichShape& sh, const uint32_t* table, const uint32_t* bits, uint64_t entries,
                    unsigned long long* single, unsigned long long* dbl, hipStream_t stream) {
  if ((int)sh.G == G) return launch_g<G>(sh, table, bits, entries, single, dbl, stream);
  if constexpr (G < kEnrichMaxG) return dispatch<G + 1>(sh, table, bits, entries, single, dbl, stream);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t bc_enrich_launch(const EnrichShape& sh, const uint32_t* d_table, const uint32_t* d_bits, uint64_t entries,
                            unsigned long long* d_single, unsigned long long* d_double, hipStream_t stream) {
  if (entries == 0 || sh.G == 0) return hipSuccess;
  return dispatch<1>(sh, d_table, d_bits, entries, d_single, sh.G >= 3 ? d_double : nullptr, stream);
}
