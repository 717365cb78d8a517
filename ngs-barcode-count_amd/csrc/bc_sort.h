// bc_sort.h -- stable LSD radix sort of (u64 key, u32 value) pairs on the device: the order of a raw-key plan's counts
// files (bc_raw_render.h).  Plain HIP kernels, compiled with whoever includes this header (the engine, and the test
// harness tests/sort/sort_harness.hip); one entry point, bc::sort_pairs_launch -- and, built on it at the end of this
// file, bc::sort_words_launch: the order of keys several u64 wide (bc_wide_render.h; tests/sort/sort_words_harness.hip).
//
// Eight bits per pass, least significant byte first; only the passes below key_bits run.
//   before the passes  sort_ghist_kernel   the global digit histogram of EVERY pass in one sweep of the keys (the
//                                          multiset of keys never changes).  The host reads the 8 x 256 counters back:
//                                          a pass in which one digit holds all n keys would move nothing relative to
//                                          anything, and is skipped -- no launch, no data movement, no buffer swap.
//   per live pass      sort_hist_kernel    digit histogram of every tile -> hist[digit * n_tiles + tile]
//                      sort_scan_kernel    one workgroup per digit: exclusive scan over its tiles, on top of the
//                                          digit's base (the exclusive scan of the global histogram).  hist then holds
//                                          where the first key of (digit, tile) goes.
//                      sort_scatter_kernel the tile's keys ranked and written to their places in the other buffer.
// The pairs ping-pong between *_in and *_tmp; after an odd number of live passes the result is copied back, so the
// sorted pairs are ALWAYS in keys_in / vals_in when the stream has drained.
//
// Stability (what makes LSD correct) in the scatter: a tile is kSortTile consecutive pairs, a wavefront owns
// kSortChunks consecutive chunks of 64, one pair per lane.  Inside a chunk the lanes that hold the same digit find each
// other by eight ballots (match-any over the digit's bits); a pair's rank among them is the number of lower lanes in
// that mask.  The lowest lane of each mask stores the mask's population to cnt[chunk][digit] in LDS -- a plain store,
// one writer per cell, no LDS atomics, whose order would be arbitrary.  One thread per digit then turns its column into
// an exclusive prefix over the chunks in tile order.  Place of a pair = hist[digit][tile] + cnt[chunk][digit] + rank:
// ascending in (tile, chunk, lane) for equal digits, which is the order the pairs came in.
// (The histograms only count, so sort_ghist_kernel / sort_hist_kernel may use LDS atomics.)
//
// Keys are compared as unsigned 64-bit numbers (bit 63 is a digit bit like any other).  n == 0 and n == 1 launch
// nothing.  n must stay below 2^32 - kSortTile (hipErrorInvalidValue otherwise): counters and places are u32.
//
// Device memory, n pairs:  2 x 12 n bytes (the caller's two pairs of buffers)
//                        + 1024 x n_tiles bytes of tile histograms (256 u32 per tile of 2048 pairs: n / 2 bytes)
//                        + 8 KiB of global histograms         = 24.5 n bytes + 8 KiB; sort_scratch_words(n) u32 of
// scratch hold the last two.
// Per workgroup (256 threads): 17,408 B of LDS in the scatter (32 chunks x 256 u16 + 256 u32 of bases; 14 pieces of
// 1,280 B = 17,920 B allocated, so LDS never limits residency below the 8 wavefronts a SIMD holds), 1 KiB in the tile
// histogram, 8 KiB in the global histogram.  No scratch memory (DESIGN.md section 7 records the code object's figures).
#ifndef BC_SORT_H
#define BC_SORT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bc {

constexpr uint32_t kSortBits = 8, kSortDigits = 1u << kSortBits;
constexpr uint32_t kSortWaves = 4, kSortChunks = 8;              // wavefronts per workgroup, chunks per wavefront
constexpr uint32_t kSortTile = kSortWaves * kSortChunks * 64;    // 2048 pairs
constexpr uint32_t kSortMaxPasses = 8;
static_assert(kSortWaves * 64 == kSortDigits, "one thread per digit in the prefix step");
static_assert(kSortTile <= 0xFFFFu, "a tile's prefix fits the u16 cells");

inline uint64_t sort_tiles(uint64_t n) { return (n + kSortTile - 1) / kSortTile; }
// u32 words of scratch for n pairs: the tile histograms, then the global histograms of all passes
inline uint64_t sort_scratch_words(uint64_t n) { return (uint64_t)kSortDigits * sort_tiles(n) + kSortMaxPasses * kSortDigits; }
inline uint32_t sort_passes(uint32_t key_bits) {
  const uint32_t p = (key_bits + kSortBits - 1) / kSortBits;
  return p > kSortMaxPasses ? kSortMaxPasses : p;
}

__device__ __forceinline__ uint32_t sort_digit(unsigned long long key, uint32_t pass) {
  return (uint32_t)(key >> (pass * kSortBits)) & (kSortDigits - 1u);
}

// ghist[pass * 256 + digit] += the keys with that digit, for pass < n_passes (ghist zeroed by the caller)
__global__ __launch_bounds__(256) void sort_ghist_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t n_passes,
                                                         uint32_t* __restrict__ ghist) {
  __shared__ uint32_t bins[kSortMaxPasses * kSortDigits];
  for (uint32_t i = threadIdx.x; i < n_passes * kSortDigits; i += blockDim.x) bins[i] = 0u;
  __syncthreads();
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const unsigned long long k = keys[i];
    for (uint32_t p = 0; p < n_passes; ++p) atomicAdd(&bins[p * kSortDigits + sort_digit(k, p)], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_passes * kSortDigits; i += blockDim.x)
    if (bins[i]) atomicAdd(&ghist[i], bins[i]);
}

// hist[digit * n_tiles + tile] = the tile's keys with that digit; one workgroup per tile
__global__ __launch_bounds__(256) void sort_hist_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t pass,
                                                        uint32_t n_tiles, uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[kSortDigits];
  const uint32_t tile = blockIdx.x;
  bins[threadIdx.x] = 0u;
  __syncthreads();
  const uint64_t t0 = (uint64_t)tile * kSortTile;
#pragma unroll
  for (uint32_t c = 0; c < kSortTile / 256; ++c) {
    const uint64_t i = t0 + c * 256u + threadIdx.x;
    if (i < n) atomicAdd(&bins[sort_digit(keys[i], pass)], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * n_tiles + tile] = bins[threadIdx.x];
}

// workgroup d: hist[d][0 .. n_tiles) -> exclusive scan + the keys with a smaller digit (from the global histogram)
__global__ __launch_bounds__(256) void sort_scan_kernel(uint32_t* __restrict__ hist, uint32_t n_tiles,
                                                        const uint32_t* __restrict__ ghist_pass) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t carry_s;
  const uint32_t d = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // the digit's base: every thread sums its share of the smaller digits' totals, then the workgroup adds up
  uint32_t part = threadIdx.x < d ? ghist_pass[threadIdx.x] : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += (uint32_t)__shfl_xor((int)part, o);
  if (lane == 0) wsum[wave] = part;
  __syncthreads();
  if (threadIdx.x == 0) carry_s = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  uint32_t* row = hist + (uint64_t)d * n_tiles;
  uint32_t carry = carry_s;  // (every thread keeps the running total itself)
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256u) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t x = t < n_tiles ? row[t] : 0u;
    uint32_t s = x;  // inclusive scan inside the wavefront
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)s, o);
      if (lane >= (uint32_t)o) s += y;
    }
    __syncthreads();  // (everyone has read the wsum of the round before)
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t w = 0; w < wave; ++w) before += wsum[w];
    if (t < n_tiles) row[t] = before + s - x;
    carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
  }
}

// the tile's pairs to their places: hist as sort_scan_kernel left it
__global__ __launch_bounds__(256) void sort_scatter_kernel(const unsigned long long* __restrict__ keys_in,
                                                           const uint32_t* __restrict__ vals_in,
                                                           unsigned long long* __restrict__ keys_out,
                                                           uint32_t* __restrict__ vals_out, uint32_t n, uint32_t pass,
                                                           uint32_t n_tiles, const uint32_t* __restrict__ hist) {
  __shared__ __attribute__((aligned(16))) uint16_t cnt[kSortWaves * kSortChunks][kSortDigits];
  __shared__ uint32_t base[kSortDigits];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  {
    uint32_t* z = (uint32_t*)&cnt[0][0];
    for (uint32_t i = threadIdx.x; i < kSortWaves * kSortChunks * kSortDigits / 2; i += 256u) z[i] = 0u;
  }
  base[threadIdx.x] = hist[(uint64_t)threadIdx.x * n_tiles + tile];
  __syncthreads();
  const uint64_t w0 = (uint64_t)tile * kSortTile + (uint64_t)wave * kSortChunks * 64u;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long key[kSortChunks];
  uint32_t rank[kSortChunks];  // rank among the chunk's equal digits | digit << 8 | valid << 16
#pragma unroll
  for (uint32_t c = 0; c < kSortChunks; ++c) {
    const uint64_t i = w0 + c * 64u + lane;
    const bool valid = i < n;
    key[c] = valid ? keys_in[i] : 0ull;
    const uint32_t d = sort_digit(key[c], pass);
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < kSortBits; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    // (an invalid lane's mask is the valid lanes with digit 0: it is not in it, and stores nothing)
    if (valid && (peers & below) == 0ull) cnt[wave * kSortChunks + c][d] = (uint16_t)__popcll(peers);
    rank[c] = (uint32_t)__popcll(peers & below) | (d << 8) | (valid ? 1u << 16 : 0u);
  }
  __syncthreads();
  {
    uint32_t run = 0;
#pragma unroll 8
    for (uint32_t ch = 0; ch < kSortWaves * kSortChunks; ++ch) {
      const uint32_t x = cnt[ch][threadIdx.x];
      cnt[ch][threadIdx.x] = (uint16_t)run;
      run += x;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t c = 0; c < kSortChunks; ++c) {
    if (!(rank[c] >> 16)) continue;
    const uint32_t d = (rank[c] >> 8) & 0xFFu;
    const uint32_t pos = base[d] + cnt[wave * kSortChunks + c][d] + (rank[c] & 0xFFu);
    if (pos < n) {  // (always: the places of a pass are a permutation of 0 .. n-1)
      keys_out[pos] = key[c];
      vals_out[pos] = vals_in[w0 + c * 64u + lane];
    }
  }
}

// Sorts the n pairs (keys_in[i], vals_in[i]) by ascending key, stably; keys below 2^key_bits (key_bits 1 .. 64; bits at
// and above key_bits are not looked at).  *_tmp: n entries each; scratch: sort_scratch_words(n) u32.  Enqueues on
// `stream`, and waits for it once (the global histogram comes back to the host).  The result is in keys_in / vals_in.
// live_passes (may be NULL): the passes that moved data.
inline hipError_t sort_pairs_launch(hipStream_t stream, uint64_t* keys_in, uint32_t* vals_in, uint64_t* keys_tmp,
                                    uint32_t* vals_tmp, uint64_t n, uint32_t key_bits, uint32_t* scratch,
                                    uint32_t* live_passes = nullptr) {
  if (live_passes) *live_passes = 0;
  if (n < 2) return hipSuccess;
  if (n >= 0xFFFFFFFFull - kSortTile || key_bits == 0 || key_bits > 64) return hipErrorInvalidValue;
  const uint32_t n32 = (uint32_t)n, n_tiles = (uint32_t)sort_tiles(n), n_passes = sort_passes(key_bits);
  uint32_t* hist = scratch;
  uint32_t* ghist = scratch + (uint64_t)kSortDigits * n_tiles;
  hipError_t rc = hipMemsetAsync(ghist, 0, kSortMaxPasses * kSortDigits * 4, stream);
  if (rc != hipSuccess) return rc;
  const uint32_t ggrid = n_tiles < 2048u ? n_tiles : 2048u;
  hipLaunchKernelGGL(sort_ghist_kernel, dim3(ggrid), dim3(256), 0, stream, (const unsigned long long*)keys_in, n32, n_passes, ghist);
  if ((rc = hipGetLastError()) != hipSuccess) return rc;
  uint32_t h_ghist[kSortMaxPasses * kSortDigits];
  if ((rc = hipMemcpyAsync(h_ghist, ghist, sizeof h_ghist, hipMemcpyDeviceToHost, stream)) != hipSuccess) return rc;
  if ((rc = hipStreamSynchronize(stream)) != hipSuccess) return rc;
  unsigned long long* kin = (unsigned long long*)keys_in;
  unsigned long long* kout = (unsigned long long*)keys_tmp;
  uint32_t *vin = vals_in, *vout = vals_tmp;
  uint32_t live = 0;
  for (uint32_t p = 0; p < n_passes; ++p) {
    bool single = false;
    for (uint32_t d = 0; d < kSortDigits; ++d) single |= h_ghist[p * kSortDigits + d] == n32;
    if (single) continue;  // every key has the same digit here: the order stands, and so does the buffer
    hipLaunchKernelGGL(sort_hist_kernel, dim3(n_tiles), dim3(256), 0, stream, kin, n32, p, n_tiles, hist);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(kSortDigits), dim3(256), 0, stream, hist, n_tiles, ghist + p * kSortDigits);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(n_tiles), dim3(256), 0, stream, kin, vin, kout, vout, n32, p, n_tiles, hist);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    unsigned long long* tk = kin;
    kin = kout;
    kout = tk;
    uint32_t* tv = vin;
    vin = vout;
    vout = tv;
    ++live;
  }
  if (live & 1u) {  // the data sits in *_tmp
    if ((rc = hipMemcpyAsync(keys_in, keys_tmp, n * 8, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return rc;
    if ((rc = hipMemcpyAsync(vals_in, vals_tmp, n * 4, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return rc;
  }
  if (live_passes) *live_passes = live;
  return hipSuccess;
}

// ---- keys of several words (bc_wide_render.h) ----

__global__ __launch_bounds__(256) void sort_iota_kernel(uint32_t* __restrict__ perm, uint32_t n) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) perm[i] = (uint32_t)i;
}

// col[j] = word[perm[j]]: one word of every key, in the order the passes before have made
__global__ __launch_bounds__(256) void sort_column_kernel(const unsigned long long* __restrict__ word,
                                                          const uint32_t* __restrict__ perm, uint32_t n,
                                                          unsigned long long* __restrict__ col) {
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += step) {
    const uint32_t i = perm[j];
    col[j] = i < n ? word[i] : 0ull;  // (always: perm is a permutation of 0 .. n-1)
  }
}

// The order of n keys of K u64 words each, compared word by word as unsigned numbers with word K-1 the most significant:
// perm[j] = the index of the key that comes j-th, keys equal in every word in ascending index (the sort is stable).
// words: K columns of n entries, word w of key i at words[w * n + i]; they are only read.
// LSD over the words, least significant first: per word, its column gathered in the order made so far and sorted with the
// permutation as the value by sort_pairs_launch -- whose stability is what carries the lower words' order through, and
// whose skipped passes make a word that all keys share cost one histogram sweep.
// col, col_tmp: n u64 each; perm_tmp: n u32; scratch: sort_scratch_words(n) u32.  Enqueues on `stream` and waits for it
// once per word.  n == 0 launches nothing; n at or above 2^32 - kSortTile: hipErrorInvalidValue.
// Device memory beside the keys' K x 8 n bytes: 4 n (perm) + 16 n + 4 n + n / 2 + 8 KiB = 24.5 n bytes + 8 KiB.
// live_passes (may be NULL): the passes that moved data, over all words.
inline hipError_t sort_words_launch(hipStream_t stream, const uint64_t* words, uint32_t K, uint64_t n, uint32_t* perm,
                                    uint64_t* col, uint64_t* col_tmp, uint32_t* perm_tmp, uint32_t* scratch,
                                    uint32_t* live_passes = nullptr) {
  if (live_passes) *live_passes = 0;
  if (n == 0) return hipSuccess;
  if (n >= 0xFFFFFFFFull - kSortTile || K == 0) return hipErrorInvalidValue;
  const uint32_t n32 = (uint32_t)n;
  const uint32_t grid = (uint32_t)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(sort_iota_kernel, dim3(grid), dim3(256), 0, stream, perm, n32);
  hipError_t rc = hipGetLastError();
  if (rc != hipSuccess || n < 2) return rc;
  for (uint32_t w = 0; w < K; ++w) {
    hipLaunchKernelGGL(sort_column_kernel, dim3(grid), dim3(256), 0, stream, (const unsigned long long*)words + (uint64_t)w * n,
                       (const uint32_t*)perm, n32, (unsigned long long*)col);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    uint32_t live = 0;
    if ((rc = sort_pairs_launch(stream, col, perm, col_tmp, perm_tmp, n, 64, scratch, &live)) != hipSuccess) return rc;
    if (live_passes) *live_passes += live;
  }
  return hipSuccess;
}

}  // namespace bc

#endif
