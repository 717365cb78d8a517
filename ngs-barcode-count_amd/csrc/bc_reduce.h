// bc_reduce.h -- run reduction of sorted (u64 key, u32 value) pairs on the device: one (key, u64 sum of the values) per
// run of equal keys, in the input's order, and the number of runs.  What turns a raw-key plan's sorted, projected
// tuples into the sums of its Single and Double files (bc_raw_enrich_render.h).  Plain HIP kernels, compiled with
// whoever includes this header (the engine, and the test harness tests/reduce/reduce_harness.hip); one entry point,
// bc::reduce_runs_launch.  No library.
//
// A tile is kReduceTile consecutive pairs (the sort's tile), a wavefront owns kReduceChunks consecutive chunks of 64,
// one pair per lane.  A head is position 0, or a position whose key differs from its predecessor's; the run number of
// a pair is the number of heads at or before it, minus one.
//   reduce_heads_kernel  the heads of every tile -> tile_heads[tile]
//   reduce_scan_kernel   one workgroup: exclusive scan over the tiles in place, the total -> *d_n_runs
//   reduce_sum_kernel    every pair learns its run number (heads before the tile + before the chunk + ballot), a head
//                        stores its key to out_keys[run], and the values are summed:
// inside a chunk by an inclusive scan over the lanes (shuffles, u64) from which the last lane of every segment takes
// its segment's sum -- scan[last] - scan[lane before the segment's first] -- so no lane ever walks a run; from chunk to
// chunk the sum of the segment that is still open travels in a wavefront-uniform carry.  A sum leaves the wavefront
// when its run ends inside the wavefront's 512 pairs, or at their end: ONE no-return global_atomic_add_x2 per
// (wavefront, run) into out_sums, which this header zeroes first.  A run of a million pairs costs about 2000 atomics,
// not a million; integer adds make the result independent of their order.
//
// Keys are compared as unsigned 64-bit numbers (bit 63 is a key bit like any other); sums are u64 (values near 2^32 add
// past 2^32).  n == 0 and n == 1 launch no kernel (memsets and copies only).  n must stay below 2^32 - kReduceTile
// (hipErrorInvalidValue otherwise, as the sort): run numbers and tile counters are u32.
//
// Device memory, n pairs: the caller's out_keys and out_sums (n entries each: there may be n runs), 4 bytes at
// d_n_runs and reduce_scratch_words(n) u32 of scratch (one per tile).  Per workgroup (256 threads) 16 B of LDS.  No
// scratch memory, only vector stores and vector atomics (DESIGN.md section 7 records the code object's figures).
#ifndef BC_REDUCE_H
#define BC_REDUCE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bc {

constexpr uint32_t kReduceWaves = 4, kReduceChunks = 8;                // wavefronts per workgroup, chunks per wavefront
constexpr uint32_t kReduceTile = kReduceWaves * kReduceChunks * 64;    // 2048 pairs

inline uint64_t reduce_tiles(uint64_t n) { return (n + kReduceTile - 1) / kReduceTile; }
// u32 words of scratch for n pairs: the heads of every tile (never none, so that n == 0 may allocate it too)
inline uint64_t reduce_scratch_words(uint64_t n) { return n ? reduce_tiles(n) : 1; }

// The heads among the 64 pairs from position i - lane on, as a lane mask; key: the lane's own key (0 beyond n).
__device__ __forceinline__ unsigned long long reduce_heads(const unsigned long long* __restrict__ keys, uint64_t i, uint32_t n,
                                                           uint32_t lane, unsigned long long& key) {
  const bool valid = i < n;
  key = valid ? keys[i] : 0ull;
  unsigned long long prev = __shfl_up(key, 1);
  if (lane == 0) prev = valid && i > 0 ? keys[i - 1] : ~key;  // (position 0 differs from what is before it)
  return __ballot(valid && key != prev);
}

// tile_heads[tile] = the heads among the tile's pairs; one workgroup per tile
__global__ __launch_bounds__(256) void reduce_heads_kernel(const unsigned long long* __restrict__ keys, uint32_t n,
                                                           uint32_t* __restrict__ tile_heads) {
  __shared__ uint32_t wsum[kReduceWaves];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t w0 = (uint64_t)tile * kReduceTile + (uint64_t)wave * kReduceChunks * 64u;
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t c = 0; c < kReduceChunks; ++c) {
    unsigned long long key;
    mine += (uint32_t)__popcll(reduce_heads(keys, w0 + c * 64u + lane, n, lane, key));
  }
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) tile_heads[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: tile_heads[0 .. n_tiles) -> its exclusive scan, in place; *n_runs = the total
__global__ __launch_bounds__(256) void reduce_scan_kernel(uint32_t* __restrict__ tile_heads, uint32_t n_tiles,
                                                          uint32_t* __restrict__ n_runs) {
  __shared__ uint32_t wsum[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry = 0;  // (every thread keeps the running total itself)
  for (uint32_t t0 = 0; t0 < n_tiles; t0 += 256u) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t x = t < n_tiles ? tile_heads[t] : 0u;
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
    if (t < n_tiles) tile_heads[t] = before + s - x;
    carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
  }
  if (threadIdx.x == 0) *n_runs = carry;
}

// the tile's pairs into their runs: tile_base as reduce_scan_kernel left it, out_sums zeroed
__global__ __launch_bounds__(256) void reduce_sum_kernel(const unsigned long long* __restrict__ keys,
                                                         const uint32_t* __restrict__ vals, uint32_t n,
                                                         const uint32_t* __restrict__ tile_base,
                                                         unsigned long long* __restrict__ out_keys,
                                                         unsigned long long* __restrict__ out_sums) {
  __shared__ uint32_t wave_heads[kReduceWaves];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t w0 = (uint64_t)tile * kReduceTile + (uint64_t)wave * kReduceChunks * 64u;
  unsigned long long key[kReduceChunks], heads[kReduceChunks];
  uint32_t mine = 0;
#pragma unroll
  for (uint32_t c = 0; c < kReduceChunks; ++c) {
    heads[c] = reduce_heads(keys, w0 + c * 64u + lane, n, lane, key[c]);
    mine += (uint32_t)__popcll(heads[c]);
  }
  if (lane == 0) wave_heads[wave] = mine;
  __syncthreads();
  uint32_t base = tile_base[tile];  // the heads before this wavefront's pairs
  for (uint32_t w = 0; w < wave; ++w) base += wave_heads[w];
  const unsigned long long upto = (2ull << lane) - 1ull;  // the lanes up to and including this one
  // the segment still open at the end of the chunk before: its sum so far and its run (wavefront-uniform)
  unsigned long long carry = 0ull;
  uint32_t carry_run = 0u;
  bool open = false;
#pragma unroll
  for (uint32_t c = 0; c < kReduceChunks; ++c) {
    const uint64_t i = w0 + c * 64u + lane;
    const bool valid = i < n;
    const unsigned long long V = __ballot(valid);
    if (V == 0ull) break;  // (the valid pairs are a prefix: nothing follows either)
    const unsigned long long H = heads[c];
    const uint32_t run = base + (uint32_t)__popcll(H & upto) - 1u;
    const bool head = (H >> lane) & 1ull;
    // (run < n and carry_run < n always: there are no more heads than pairs.  The tests below only keep a store or an
    // atomic inside the caller's n entries whatever the keys hold, as the sort's `pos < n` does.)
    if (head && run < n) out_keys[run] = key[c];
    unsigned long long x = valid ? (unsigned long long)vals[i] : 0ull;  // -> inclusive scan over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = __shfl_up(x, o);
      if (lane >= (uint32_t)o) x += y;
    }
    // the lane's segment starts at lane a: the highest head at or below it, or lane 0 when the run came in from before
    const uint32_t a = 63u - (uint32_t)__clzll((long long)((H | 1ull) & upto));
    const unsigned long long before = __shfl(x, a ? (int)a - 1 : 0);
    unsigned long long seg = x - (a ? before : 0ull);  // the segment's sum, on its last lane
    const uint32_t last = (uint32_t)__popcll(V) - 1u;  // the last valid lane
    if (!(H & 1ull)) {
      if (a == 0u) seg += carry;  // the open segment goes on (carry is 0 when it began in another wavefront)
    } else if (open && lane == 0 && carry_run < n) {
      atomicAdd(out_sums + carry_run, carry);  // it ended with the chunk before
    }
    if (lane < last && ((H >> (lane + 1u)) & 1ull) && run < n) atomicAdd(out_sums + run, seg);  // ends inside the chunk
    carry = __shfl(seg, (int)last);
    carry_run = (uint32_t)__shfl((int)run, (int)last);
    open = true;
    base += (uint32_t)__popcll(H);
  }
  if (open && lane == 0 && carry_run < n) atomicAdd(out_sums + carry_run, carry);
}

// Reduces the n pairs (keys[i], vals[i]), sorted by key, to one (key, sum) per run of equal keys, in the input's order:
// out_keys[r], out_sums[r] for r < *d_n_runs.  out_keys, out_sums: n entries each (out_sums is zeroed here); d_n_runs: one
// u32 on the device; scratch: reduce_scratch_words(n) u32.  Enqueues on `stream` and does not wait for it.
inline hipError_t reduce_runs_launch(hipStream_t stream, const uint64_t* keys, const uint32_t* vals, uint64_t n,
                                     uint64_t* out_keys, uint64_t* out_sums, uint32_t* d_n_runs, uint32_t* scratch) {
  if (n >= 0xFFFFFFFFull - kReduceTile) return hipErrorInvalidValue;
  hipError_t rc;
  if (n == 0) return hipMemsetAsync(d_n_runs, 0, 4, stream);
  if ((rc = hipMemsetAsync(out_sums, 0, n * 8, stream)) != hipSuccess) return rc;
  if (n == 1) {  // one run: the pair itself, moved by copies (the value into the low half of its zeroed sum)
    if ((rc = hipMemcpyAsync(out_keys, keys, 8, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return rc;
    if ((rc = hipMemcpyAsync(out_sums, vals, 4, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return rc;
    return hipMemsetD32Async((hipDeviceptr_t)d_n_runs, 1, 1, stream);
  }
  const uint32_t n32 = (uint32_t)n, n_tiles = (uint32_t)reduce_tiles(n);
  hipLaunchKernelGGL(reduce_heads_kernel, dim3(n_tiles), dim3(256), 0, stream, (const unsigned long long*)keys, n32, scratch);
  hipLaunchKernelGGL(reduce_scan_kernel, dim3(1), dim3(256), 0, stream, scratch, n_tiles, d_n_runs);
  hipLaunchKernelGGL(reduce_sum_kernel, dim3(n_tiles), dim3(256), 0, stream, (const unsigned long long*)keys, vals, n32,
                     (const uint32_t*)scratch, (unsigned long long*)out_keys, (unsigned long long*)out_sums);
  return hipGetLastError();
}

}  // namespace bc

#endif
