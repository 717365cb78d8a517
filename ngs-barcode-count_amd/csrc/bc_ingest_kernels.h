// bc_ingest_kernels.h -- the device side of the FASTQ ingest: newline scan, record table, gather into the fixed-stride
// batch, overlap copy.  Included by bc_ingest.hip only (its header comment tells how they fit together).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bc_bgzf.hpp"

namespace {

constexpr uint32_t kScanBlock = 4096;  // text bytes per 256-thread block of the newline kernels (16 per thread)

// what the device reports per chunk (pinned host memory)
struct ChunkStats {
  unsigned long long n_lines;  // newlines in [start, len)
  unsigned long long n_rec;    // whole records among them
  unsigned long long end_pos;  // buffer offset just past the last whole record (= start when there is none)
  long long start;             // buffer offset of the first unframed byte; < 0: the overlap was too short
  unsigned int min_len, max_len;  // sequence-line lengths over the chunk's records
  unsigned int max_qlen;
  unsigned int qual_differs;   // some record's quality line is not as long as its sequence line
  unsigned int last_is_newline;
  unsigned int pad;            // BAM: the framing's status (kBam* of bc_bam.h)
};

struct DevState {
  unsigned long long next_off;  // file offset of the first byte no record has been made of yet
};

__device__ __forceinline__ uint32_t newline_mask16(const uint4& v, uint32_t first_valid, uint32_t n_valid) {
  // bit i set: byte i of the 16 is '\n' and first_valid <= i < n_valid
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = w[k] ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 where the byte is '\n'
    m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * k);
  }
  uint32_t keep = n_valid >= 16u ? 0xFFFFu : ((1u << n_valid) - 1u);
  keep &= ~((1u << (first_valid > 16u ? 16u : first_valid)) - 1u);
  return m & keep;
}

__global__ void ingest_begin_kernel(DevState* st, unsigned long long buf_file_off, unsigned long long len, ChunkStats* cs,
                                    const uint8_t* text) {
  const long long start = (long long)st->next_off - (long long)buf_file_off;
  cs->start = start;
  cs->n_lines = 0;
  cs->n_rec = 0;
  cs->end_pos = start < 0 ? 0ull : (unsigned long long)start;
  cs->min_len = 0xFFFFFFFFu;
  cs->max_len = 0;
  cs->max_qlen = 0;
  cs->qual_differs = 0;
  cs->last_is_newline = len ? (text[len - 1] == '\n') : 1u;
}

// newlines per block of kScanBlock bytes
__global__ __launch_bounds__(256) void ingest_count_kernel(const uint8_t* __restrict__ text, unsigned long long len,
                                                           const ChunkStats* __restrict__ cs, uint32_t* __restrict__ blk_cnt) {
  __shared__ uint32_t s_sum[4];
  const long long start = cs->start < 0 ? (long long)len : cs->start;
  const unsigned long long p = (unsigned long long)blockIdx.x * kScanBlock + threadIdx.x * 16u;
  uint32_t c = 0;
  if (p < len && p + 16 > (unsigned long long)start) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + p);
    const uint32_t first = (unsigned long long)start > p ? (uint32_t)((unsigned long long)start - p) : 0u;
    const uint32_t valid = len - p >= 16 ? 16u : (uint32_t)(len - p);
    c = __popc(newline_mask16(v, first, valid));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// exclusive prefix sum of the block counts (one workgroup), totals into the stats
__global__ __launch_bounds__(1024) void ingest_scan_kernel(const uint32_t* __restrict__ blk_cnt, uint32_t n_blk,
                                                           uint32_t* __restrict__ blk_off, ChunkStats* cs, uint64_t line_cap) {
  __shared__ uint32_t s_part[1024];
  const uint32_t per = (n_blk + 1023u) / 1024u;
  const uint32_t a = threadIdx.x * per, b = min(n_blk, a + per);
  uint32_t sum = 0;
  for (uint32_t i = a; i < b; ++i) sum += blk_cnt[i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan
    const uint32_t v = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0u;
    __syncthreads();
    s_part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = s_part[threadIdx.x] - sum;
  for (uint32_t i = a; i < b; ++i) {
    blk_off[i] = run;
    run += blk_cnt[i];
  }
  if (threadIdx.x == 1023) {
    unsigned long long lines = s_part[1023];
    if (lines > line_cap) lines = line_cap;  // (never with the caps used: one position slot per two text bytes)
    cs->n_lines = lines;
    cs->n_rec = lines / 4;
  }
}

// position of every newline, in order
__global__ __launch_bounds__(256) void ingest_positions_kernel(const uint8_t* __restrict__ text, unsigned long long len,
                                                               const ChunkStats* __restrict__ cs,
                                                               const uint32_t* __restrict__ blk_off, uint32_t* __restrict__ nl_pos,
                                                               uint64_t line_cap) {
  __shared__ uint32_t s_wave[4];
  const long long start = cs->start < 0 ? (long long)len : cs->start;
  const unsigned long long p = (unsigned long long)blockIdx.x * kScanBlock + threadIdx.x * 16u;
  uint32_t m = 0;
  if (p < len && p + 16 > (unsigned long long)start) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + p);
    const uint32_t first = (unsigned long long)start > p ? (uint32_t)((unsigned long long)start - p) : 0u;
    const uint32_t valid = len - p >= 16 ? 16u : (uint32_t)(len - p);
    m = newline_mask16(v, first, valid);
  }
  const uint32_t c = __popc(m);
  // exclusive scan of c over the block: within the wave by shuffles, across the four waves through LDS
  uint32_t incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
    if ((threadIdx.x & 63) >= (uint32_t)o) incl += t;
  }
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t base = blk_off[blockIdx.x];
  for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) base += s_wave[w];
  uint32_t rank = base + incl - c;
  while (m) {
    const uint32_t i = __ffs(m) - 1u;
    m &= m - 1u;
    if (rank < line_cap) nl_pos[rank] = (uint32_t)(p + i);
    ++rank;
  }
}

// one thread per record: where its sequence and quality lines are, and how long
__global__ __launch_bounds__(256) void ingest_records_kernel(const uint8_t* __restrict__ text, const uint32_t* __restrict__ nl_pos,
                                                             ChunkStats* cs, int strip_cr, uint32_t* __restrict__ seq_at,
                                                             uint32_t* __restrict__ qual_at, uint16_t* __restrict__ lens,
                                                             uint16_t* __restrict__ qlens) {
  const unsigned long long n_rec = cs->n_rec;
  const unsigned long long r = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t sl = 0xFFFFFFFFu, ql = 0, sl_max = 0;
  bool differs = false;
  if (r < n_rec) {
    const uint32_t e0 = nl_pos[4 * r], e1 = nl_pos[4 * r + 1], e2 = nl_pos[4 * r + 2], e3 = nl_pos[4 * r + 3];
    uint32_t s = e1 - (e0 + 1u), q = e3 - (e2 + 1u);
    // BufReader::lines() drops a "\r\n" ending (input.rs:44); the gz path's read_line keeps the '\r' (input.rs:66-68)
    if (strip_cr && s && text[e1 - 1] == '\r') --s;
    if (strip_cr && q && text[e3 - 1] == '\r') --q;
    seq_at[r] = e0 + 1u;
    qual_at[r] = e2 + 1u;
    lens[r] = (uint16_t)(s > 65535u ? 65535u : s);
    qlens[r] = (uint16_t)(q > 65535u ? 65535u : q);
    sl = sl_max = s;
    ql = q;
    differs = s != q;
    if (r == n_rec - 1) cs->end_pos = (unsigned long long)e3 + 1ull;
  }
  // wave-level reduction, then one atomic per wave
  uint32_t mn = sl, mx = sl_max, mq = ql, df = differs ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    mq = max(mq, (uint32_t)__shfl_xor((int)mq, o));
    df |= (uint32_t)__shfl_xor((int)df, o);
  }
  if ((threadIdx.x & 63) == 0 && mn != 0xFFFFFFFFu) {
    atomicMin(&cs->min_len, mn);
    atomicMax(&cs->max_len, mx);
    atomicMax(&cs->max_qlen, mq);
    if (df) atomicOr(&cs->qual_differs, 1u);
  }
}

// records [first, first + n) -> fixed-stride batch: one wavefront per record, lanes 0-31 move the sequence line,
// lanes 32-63 the quality line, a dword (four bytes gathered from the unaligned text) per lane and step
__global__ __launch_bounds__(256) void ingest_gather_kernel(const uint8_t* __restrict__ text, const uint32_t* __restrict__ seq_at,
                                                            const uint32_t* __restrict__ qual_at, const uint16_t* __restrict__ lens,
                                                            const uint16_t* __restrict__ qlens, unsigned long long first,
                                                            unsigned long long n, uint32_t stride, uint8_t* __restrict__ out_seq,
                                                            uint8_t* __restrict__ out_qual) {
  const unsigned long long r = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= n) return;
  const uint32_t lane = threadIdx.x & 63u;
  const bool is_qual = lane >= 32u;
  const uint32_t j0 = lane & 31u;
  const uint32_t at = is_qual ? qual_at[first + r] : seq_at[first + r];
  uint32_t len = is_qual ? (uint32_t)qlens[first + r] : (uint32_t)lens[first + r];
  if (len > stride) len = stride;
  const uint8_t* src = text + at;
  uint32_t* dst = reinterpret_cast<uint32_t*>((is_qual ? out_qual : out_seq) + r * (unsigned long long)stride);
  const uint32_t pad = is_qual ? (uint32_t)'!' : (uint32_t)'N';
  for (uint32_t d = j0; d < stride / 4u; d += 32u) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t i = 4u * d + k;
      w |= (i < len ? (uint32_t)src[i] : pad) << (8u * k);
    }
    dst[d] = w;
  }
}

// the unfinished tail of the previous chunk in front of this chunk's bytes
__global__ void ingest_overlap_kernel(const uint8_t* __restrict__ prev_end, uint8_t* __restrict__ dst_end, uint32_t bytes) {
  // copies the `bytes` bytes that end at prev_end to the `bytes` bytes that end at dst_end
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < bytes) dst_end[-(long long)bytes + i] = prev_end[-(long long)bytes + i];
}

// BAM: what the framing of bc_bam.hip found, as the stats of a chunk whose every record has four lines
__global__ void ingest_from_bam_kernel(const bc::BamStats* fs, ChunkStats* cs) {
  cs->start = fs->start;
  cs->n_rec = fs->n_rec;
  cs->n_lines = 4ull * fs->n_rec;
  cs->end_pos = fs->end_pos;
  cs->min_len = fs->min_len;
  cs->max_len = cs->max_qlen = fs->max_len;
  cs->qual_differs = 0;
  cs->last_is_newline = 1;
  cs->pad = fs->status;
}

__global__ void ingest_advance_kernel(DevState* st, const ChunkStats* cs, unsigned long long buf_file_off) {
  if (cs->start >= 0) st->next_off = buf_file_off + cs->end_pos;
}

}  // namespace
