// bc_bam_kernels.h -- the device side of the BAM ingest: candidate scan (count, prefix sum, positions: the pattern of
// the newline kernels), successors, jump pointers, marks, the record table, and the gather that unpacks nibbles and
// Phred bytes into the fixed-stride batch.  The per-element logic and why the marks are right: bc_bam.h.  Included by
// bc_bam.hip only.
//
// How many candidates a text holds is known on the device only, so every kernel behind the scan is launched with a
// grid that does not depend on it and strides over fs->n_cand; the levels a short chain does not need return at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_bam.h"
#include "bc_bgzf.hpp"

namespace bc {
namespace {

constexpr uint32_t kBamScanBlock = 4096;  // text bytes per 256-thread block of the candidate kernels (16 per thread)
constexpr uint32_t kBamStrideBlocks = 512;  // blocks of the kernels that stride over the candidates

__global__ void bam_begin_kernel(const unsigned long long* next_off, unsigned long long buf_file_off, long long start_given,
                                 BamStats* fs) {
  const long long start = next_off ? (long long)*next_off - (long long)buf_file_off : start_given;
  fs->start = start;
  fs->n_cand = 0;
  fs->n_rec = 0;
  fs->end_pos = start < 0 ? 0ull : (unsigned long long)start;
  fs->min_len = 0xFFFFFFFFu;
  fs->max_len = 0;
  fs->status = kBamOk;
  fs->pad = 0;
}

// bit i set: a record may start at text[p + i] (p a multiple of 16), start <= p + i <= len - 36
__device__ __forceinline__ uint32_t bam_mask16(const uint8_t* __restrict__ text, unsigned long long len, unsigned long long start,
                                               unsigned long long p, uint32_t n_ref) {
  if (len < kBamFixed || p > len - kBamFixed || p + 16 <= start) return 0;
  // the thread's 16 bytes and the 36 behind them: 13 words
  uint32_t d[13];
  if (p + 52 <= len) {
    const uint4 a = *reinterpret_cast<const uint4*>(text + p), b = *reinterpret_cast<const uint4*>(text + p + 16),
                c = *reinterpret_cast<const uint4*>(text + p + 32);
    d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w, d[4] = b.x, d[5] = b.y, d[6] = b.z, d[7] = b.w;
    d[8] = c.x, d[9] = c.y, d[10] = c.z, d[11] = c.w;
    d[12] = *reinterpret_cast<const uint32_t*>(text + p + 48);
  } else {  // (the text's last bytes: nothing is read behind them)
#pragma unroll
    for (uint32_t k = 0; k < 13; ++k) {
      uint32_t w = 0;
      for (uint32_t b = 0; b < 4; ++b)
        if (p + 4u * k + b < len) w |= (uint32_t)text[p + 4u * k + b] << (8u * b);
      d[k] = w;
    }
  }
  uint32_t m = 0;
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    const unsigned long long q = p + i;
    if (q < start || q > len - kBamFixed) continue;
    uint32_t w[9];
#pragma unroll
    for (uint32_t k = 0; k < 9; ++k) w[k] = alignbyte(d[(i >> 2) + k + 1], d[(i >> 2) + k], i & 3u);
    if (bam_header_check(w, n_ref) == 1u && bam_name_ok(text, len, q, bam_l_read_name(w))) m |= 1u << i;
  }
  return m;
}

// candidates per block of kBamScanBlock bytes
__global__ __launch_bounds__(256) void bam_count_kernel(const uint8_t* __restrict__ text, unsigned long long len, uint32_t n_ref,
                                                        const BamStats* __restrict__ fs, uint32_t* __restrict__ blk_cnt) {
  __shared__ uint32_t s_sum[4];
  const unsigned long long start = fs->start < 0 ? len : (unsigned long long)fs->start;
  const unsigned long long p = (unsigned long long)blockIdx.x * kBamScanBlock + threadIdx.x * 16u;
  uint32_t c = __popc(bam_mask16(text, len, start, p, n_ref));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// exclusive prefix sum of block counts (one workgroup); the total goes to *total, or (above `cap`) 0 with the status
// kBamCapacity: nothing further is framed then
__global__ __launch_bounds__(1024) void bam_scan_kernel(const uint32_t* __restrict__ blk_cnt, uint32_t n_blk, uint32_t* __restrict__ blk_off,
                                                        unsigned long long* total, unsigned long long cap, BamStats* fs) {
  __shared__ unsigned long long s_part[1024];
  const uint32_t per = (n_blk + 1023u) / 1024u;
  const uint32_t a = min(n_blk, threadIdx.x * per), b = min(n_blk, a + per);
  unsigned long long sum = 0;
  for (uint32_t i = a; i < b; ++i) sum += blk_cnt[i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan
    const unsigned long long v = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0ull;
    __syncthreads();
    s_part[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned long long run = s_part[threadIdx.x] - sum;
  for (uint32_t i = a; i < b; ++i) {
    blk_off[i] = (uint32_t)(run > cap ? cap : run);
    run += blk_cnt[i];
  }
  if (threadIdx.x == 1023) {
    const unsigned long long all = s_part[1023];
    if (all > cap) fs->status = kBamCapacity;
    *total = all > cap ? 0ull : all;
  }
}

// offset of every candidate, in order
__global__ __launch_bounds__(256) void bam_positions_kernel(const uint8_t* __restrict__ text, unsigned long long len, uint32_t n_ref,
                                                            const BamStats* __restrict__ fs, const uint32_t* __restrict__ blk_off,
                                                            uint32_t* __restrict__ cand, unsigned long long cap) {
  __shared__ uint32_t s_wave[4];
  const unsigned long long start = fs->start < 0 ? len : (unsigned long long)fs->start;
  const unsigned long long p = (unsigned long long)blockIdx.x * kBamScanBlock + threadIdx.x * 16u;
  uint32_t m = bam_mask16(text, len, start, p, n_ref);
  const uint32_t c = __popc(m);
  uint32_t incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
    if ((threadIdx.x & 63) >= (uint32_t)o) incl += t;
  }
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  if (fs->n_cand == 0) return;  // none, or more than the arrays hold
  unsigned long long rank = blk_off[blockIdx.x];
  for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) rank += s_wave[w];
  rank += incl - c;
  while (m) {
    const uint32_t i = __ffs(m) - 1u;
    m &= m - 1u;
    if (rank < cap) cand[rank] = (uint32_t)(p + i);
    ++rank;
  }
}

// one thread per candidate: its link, level 0 of its jump pointers; no marks yet
__global__ __launch_bounds__(256) void bam_successor_kernel(const uint8_t* __restrict__ text, unsigned long long len, uint32_t n_ref,
                                                            const BamStats* __restrict__ fs, const uint32_t* __restrict__ cand,
                                                            uint32_t* __restrict__ link, uint32_t* __restrict__ jump0,
                                                            uint32_t* __restrict__ mark) {
  const uint32_t n = (uint32_t)fs->n_cand;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t how;
    jump0[i] = bam_successor(text, len, cand, n, i, n_ref, &how);
    link[i] = how;
    mark[i] = 0;
  }
}

// the chain's first link: the candidate at `start`, or the reason there is none
__global__ void bam_mark_start_kernel(const uint8_t* __restrict__ text, unsigned long long len, uint32_t n_ref, BamStats* fs,
                                      const uint32_t* __restrict__ cand, uint32_t* __restrict__ mark) {
  if (fs->status != kBamOk || fs->start < 0) return;
  uint32_t status;
  if (bam_chain_start(text, len, (unsigned long long)fs->start, cand, (uint32_t)fs->n_cand, n_ref, &status))
    mark[0] = 1;
  else
    fs->status = status;
}

__global__ __launch_bounds__(256) void bam_jump_kernel(const BamStats* __restrict__ fs, uint32_t* __restrict__ jump, uint32_t cap,
                                                       uint32_t level) {
  const uint32_t n = (uint32_t)fs->n_cand;
  if (!bam_level_used(level, n)) return;
  const uint32_t* below = jump + (size_t)(level - 1u) * cap;
  uint32_t* here = jump + (size_t)level * cap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) here[i] = bam_jump_step(below, i);
}

// Every marked candidate marks its 2^level-th successor.  A mark set by another thread of this launch may or may not
// be seen here; either way only candidates of the chain are marked, and the lower levels reach the rest (bc_bam.h).
__global__ __launch_bounds__(256) void bam_mark_kernel(const BamStats* __restrict__ fs, const uint32_t* __restrict__ jump, uint32_t cap,
                                                       uint32_t level, uint32_t* mark) {
  const uint32_t n = (uint32_t)fs->n_cand;
  if (!bam_level_used(level, n)) return;
  const uint32_t* here = jump + (size_t)level * cap;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    if (__hip_atomic_load(&mark[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&mark[here[i]], 1u);
}

// candidate i is a record to hand on: on the chain, whole, none of the `skip` flags
__device__ __forceinline__ bool bam_is_record(const uint8_t* __restrict__ text, const uint32_t* __restrict__ cand,
                                              const uint32_t* __restrict__ link, const uint32_t* __restrict__ mark, uint32_t i,
                                              uint32_t skip) {
  if (!mark[i] || link[i] == kLinkPartial) return false;
  const uint32_t p = cand[i];
  const uint32_t flag = (uint32_t)text[p + 18] | ((uint32_t)text[p + 19] << 8);
  return (flag & skip) == 0u;
}

// records per 256 candidates; the one marked candidate that ends the chain says where and how
__global__ __launch_bounds__(256) void bam_rec_count_kernel(const uint8_t* __restrict__ text, BamStats* fs, const uint32_t* __restrict__ cand,
                                                            const uint32_t* __restrict__ link, const uint32_t* __restrict__ mark,
                                                            uint32_t skip, uint32_t* __restrict__ blk_cnt) {
  __shared__ uint32_t s_sum[4];
  const uint32_t n = (uint32_t)fs->n_cand;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t c = 0;
  if (i < n) {
    c = bam_is_record(text, cand, link, mark, i, skip) ? 1u : 0u;
    const uint32_t how = link[i];
    if (mark[i] && how != kLinkNext) {
      uint32_t status;
      fs->end_pos = bam_chain_end(text, cand[i], how, &status);
      if (status != kBamOk) fs->status = status;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// one thread per candidate, the records among them in order: where the record, its packed sequence and its qualities
// are, how many bases it has, its flag
__global__ __launch_bounds__(256) void bam_rec_table_kernel(const uint8_t* __restrict__ text, BamStats* fs, const uint32_t* __restrict__ cand,
                                                            const uint32_t* __restrict__ link, const uint32_t* __restrict__ mark,
                                                            uint32_t skip, const uint32_t* __restrict__ blk_off, BamTables out) {
  __shared__ uint32_t s_wave[4];
  const uint32_t n = (uint32_t)fs->n_cand;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool rec = i < n && bam_is_record(text, cand, link, mark, i, skip);
  uint32_t incl = rec ? 1u : 0u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
    if ((threadIdx.x & 63) >= (uint32_t)o) incl += t;
  }
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t mn = 0xFFFFFFFFu, mx = 0;
  if (rec) {
    uint32_t r = blk_off[blockIdx.x] + incl - 1u;
    for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) r += s_wave[w];
    const uint32_t p = cand[i];
    const uint32_t l_name = text[p + 12], n_cigar = (uint32_t)text[p + 16] | ((uint32_t)text[p + 17] << 8);
    const uint32_t flag = (uint32_t)text[p + 18] | ((uint32_t)text[p + 19] << 8), l_seq = bam_u32(text + p + 20);
    const uint32_t seq_off = p + kBamFixed + l_name + 4u * n_cigar;
    if (out.rec_at) out.rec_at[r] = p;
    if (out.rec_len) out.rec_len[r] = l_seq;
    if (out.rec_flag) out.rec_flag[r] = flag;
    if (out.seq_at) {
      out.seq_at[r] = seq_off | ((flag & 0x10u) << 27);  // bit 31: reverse strand
      out.qual_at[r] = seq_off + (l_seq + 1u) / 2u;
      out.lens[r] = out.qlens[r] = (uint16_t)(l_seq > 65535u ? 65535u : l_seq);
    }
    mn = mx = l_seq;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
  }
  if ((threadIdx.x & 63) == 0 && mn != 0xFFFFFFFFu) {
    atomicMin(&fs->min_len, mn);
    atomicMax(&fs->max_len, mx);
  }
}

// records [first, first + n) -> fixed-stride batch: one wavefront per record, lanes 0-31 unpack the sequence's nibbles
// to letters, lanes 32-63 turn the Phred bytes into characters, a dword out per lane and step; a reverse-strand record
// is read from its far end, its bases complemented.  Padding is 'N' and '!'.
__global__ __launch_bounds__(256) void bam_gather_kernel(const uint8_t* __restrict__ text, const uint32_t* __restrict__ seq_at,
                                                         const uint32_t* __restrict__ qual_at, const uint16_t* __restrict__ lens,
                                                         unsigned long long first, unsigned long long n, uint32_t stride,
                                                         uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual) {
  const unsigned long long r = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= n) return;
  const uint32_t lane = threadIdx.x & 63u;
  const bool is_qual = lane >= 32u;
  const uint32_t j0 = lane & 31u;
  const uint32_t at = seq_at[first + r];
  const bool rev = (at >> 31) != 0u;
  const uint32_t full = lens[first + r];
  const uint32_t len = full > stride ? stride : full;
  const uint8_t* src = text + (is_qual ? qual_at[first + r] : (at & 0x7FFFFFFFu));
  const bool no_qual = is_qual && len && src[0] == 0xFFu;
  uint32_t* dst = reinterpret_cast<uint32_t*>((is_qual ? out_qual : out_seq) + r * (unsigned long long)stride);
  const uint32_t pad = is_qual ? (uint32_t)'!' : (uint32_t)'N';
  for (uint32_t d = j0; d < stride / 4u; d += 32u) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t i = 4u * d + k;
      uint32_t c = pad;
      if (i < len) {
        const uint32_t j = rev ? full - 1u - i : i;
        if (is_qual) {
          c = bam_qual_ascii(src[j], no_qual);
        } else {
          const uint32_t b = src[j >> 1];
          c = bam_base_ascii((j & 1u) ? (b & 15u) : (b >> 4), rev);
        }
      }
      w |= c << (8u * k);
    }
    dst[d] = w;
  }
}

}  // namespace
}  // namespace bc
