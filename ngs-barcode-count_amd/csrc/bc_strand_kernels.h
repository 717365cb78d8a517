// bc_strand_kernels.h -- the kernels of the strand setting (bc_strand.hip launches them; DESIGN.md "Reverse strand"):
//   orient   rc() of the listed reads of a batch into a scratch batch of the same form
//   select   the reads of a chunk whose outcome is BC_CONSTANT_REGION, as an ascending list of u32 + their number
//   before / after   the counters' fix-up around the reverse pass and the two u64 of bc_engine_strand_reads
//   scatter  the reverse pass's traced outcomes back to the reads' own positions
// The complement table is host code too (tests/strand/complement_host.cpp checks it under a sanitizer).
#pragma once
#include "bc_intrin.h"
#include "bc_device_plan.h"

namespace bc {

// The complement of one byte: the IUPAC pairs A-T C-G M-K R-Y V-B H-D in either case; W S N and every other byte
// (>= 0x80 included) map to themselves.  What `samtools fastq` writes for a record flagged 0x10 (bc_bam.h kBamComp*).
BC_HD uint8_t strand_complement(uint8_t c) {
  uint8_t t;
  switch (c & 0xDFu) {  // (only a letter and its lower-case form give the letter: 0x41 and 0x61 for 'A')
    case 'A': t = 'T'; break;
    case 'T': t = 'A'; break;
    case 'C': t = 'G'; break;
    case 'G': t = 'C'; break;
    case 'M': t = 'K'; break;
    case 'K': t = 'M'; break;
    case 'R': t = 'Y'; break;
    case 'Y': t = 'R'; break;
    case 'V': t = 'B'; break;
    case 'B': t = 'V'; break;
    case 'H': t = 'D'; break;
    case 'D': t = 'H'; break;
    default: return c;
  }
  return (uint8_t)(t | (c & 0x20u));
}

#if defined(__HIPCC__)

constexpr uint32_t kStrandTPB = 256;

// Bytes [o, o + 4) of the reversed line: byte o + k is source byte len - 1 - (o + k), or the pad from `len` on.  The
// four source bytes end at g + 3 = row + len - 1 - o; they come from the two aligned dwords they straddle, reversed and
// shifted in one v_perm_b32.  A dword is loaded only when it holds a byte of the line itself, so nothing before the
// buffer's first line nor beyond its last is touched (the buffer's base is 4-byte aligned).  comp: the LDS table, or
// NULL for a quality line.
__device__ __forceinline__ uint32_t strand_rev_dword(const uint32_t* __restrict__ src32, uint64_t row, uint32_t len, uint32_t o,
                                                     uint32_t pad4, const uint8_t* comp) {
  if (o >= len) return pad4;
  const long long g = (long long)row + (long long)len - 4ll - (long long)o;  // (>= -3)
  const long long a = g & ~3ll;
  const uint32_t shift = (uint32_t)g & 3u;
  const uint32_t lo = a + 3 >= (long long)row ? src32[a >> 2] : 0u;
  const uint32_t hi = shift ? src32[(a >> 2) + 1] : 0u;
  uint32_t v = perm(hi, lo, 0x00010203u + shift * 0x01010101u);
  if (comp) v = (uint32_t)comp[v & 0xFFu] | ((uint32_t)comp[(v >> 8) & 0xFFu] << 8) | ((uint32_t)comp[(v >> 16) & 0xFFu] << 16) |
                ((uint32_t)comp[v >> 24] << 24);
  const uint32_t nv = len - o;
  if (nv < 4u) {
    const uint32_t keep = (1u << (8u * nv)) - 1u;
    v = (v & keep) | (pad4 & ~keep);
  }
  return v;
}

// nb bytes of v to p: one dword store when nb == 4 (p is then 4-byte aligned), else byte stores
__device__ __forceinline__ void strand_store(uint8_t* __restrict__ p, uint32_t v, uint32_t nb) {
  if (nb == 4u) {
    *reinterpret_cast<uint32_t*>(p) = v;
  } else {
    for (uint32_t k = 0; k < nb; ++k) p[k] = (uint8_t)(v >> (8u * k));
  }
}

// Output read j = rc(read index[j]) (index NULL: read j), both lines at the batch's stride, bytes [len, stride) 'N' and
// '!' as the BAM unpacker pads.  2^lpr_shift lanes share a line; a line is cut into slots: slot 0 the bytes before the
// line's first 4-byte boundary (byte stores; none when stride is a multiple of 4), every other slot one aligned dword,
// the last one byte stores where the line ends inside it.  Nothing outside [j * stride, (j + 1) * stride) is written.
__global__ __launch_bounds__(kStrandTPB) void strand_orient_kernel(
    const uint8_t* __restrict__ seq, const uint8_t* __restrict__ qual, const uint16_t* __restrict__ lens,
    const uint16_t* __restrict__ qlens, uint32_t stride, uint32_t read_len, const uint32_t* __restrict__ index,
    unsigned long long n_out, uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual, uint16_t* __restrict__ out_lens,
    uint16_t* __restrict__ out_qlens, uint32_t lpr_shift) {
  __shared__ uint8_t s_comp[256];
  s_comp[threadIdx.x] = strand_complement((uint8_t)threadIdx.x);
  __syncthreads();
  const uint32_t lpr = 1u << lpr_shift;
  const uint32_t slots = 1u + (stride + 3u) / 4u;
  const uint32_t q0 = threadIdx.x & (lpr - 1u);
  const unsigned long long rows = kStrandTPB >> lpr_shift;
  const uint32_t* seq32 = reinterpret_cast<const uint32_t*>(seq);
  const uint32_t* qual32 = reinterpret_cast<const uint32_t*>(qual);
  for (unsigned long long j = blockIdx.x * rows + (threadIdx.x >> lpr_shift); j < n_out; j += gridDim.x * rows) {
    const unsigned long long i = index ? (unsigned long long)index[j] : j;
    const uint32_t full = lens ? (uint32_t)lens[i] : read_len;
    const uint32_t qfull = qlens ? (uint32_t)qlens[i] : full;
    const uint32_t len = full < stride ? full : stride, qlen = qfull < stride ? qfull : stride;
    const unsigned long long srow = i * stride, drow = j * stride;
    const uint32_t head = (uint32_t)(0ull - drow) & 3u;
    if (q0 == 0u) {
      if (lens && out_lens) out_lens[j] = (uint16_t)full;
      if (qlens && out_qlens) out_qlens[j] = (uint16_t)qfull;
    }
    for (uint32_t q = q0; q < slots; q += lpr) {
      uint32_t o = 0u, nb = head < stride ? head : stride;
      if (q) {
        o = head + 4u * (q - 1u);
        nb = o >= stride ? 0u : (stride - o < 4u ? stride - o : 4u);
      }
      if (!nb) continue;
      strand_store(out_seq + drow + o, strand_rev_dword(seq32, srow, len, o, 0x4E4E4E4Eu /* NNNN */, s_comp), nb);
      if (qual) strand_store(out_qual + drow + o, strand_rev_dword(qual32, srow, qlen, o, 0x21212121u /* !!!! */, nullptr), nb);
    }
  }
}

// ---- select: block b takes reads [b * span, (b + 1) * span) of the chunk (span a multiple of 256) ----

// lanes below this one whose bit is set in m
__device__ __forceinline__ uint32_t strand_rank(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(kStrandTPB) void strand_select_count_kernel(const uint8_t* __restrict__ outcome, uint32_t n, uint32_t span,
                                                                         uint32_t* __restrict__ blk_cnt) {
  __shared__ uint32_t s_w[kStrandTPB / 64];
  const uint32_t first = blockIdx.x * span;
  const uint32_t end = n - first < span ? n : first + span;
  uint32_t c = 0;
  for (uint32_t r0 = first; r0 < end; r0 += kStrandTPB) {
    const uint32_t r = r0 + threadIdx.x;
    c += (uint32_t)__popcll(__ballot(r < end && outcome[r] == (uint8_t)kConstantRegion));
  }
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0u) blk_cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// The list, ascending: a read's place is the blocks before its own (summed here from blk_cnt), the tiles of 256 before
// it in the block, the waves before its own in the tile (a scan of the four wave totals in LDS) and its rank in the
// wave (ballot + mbcnt).  The last block writes the number of entries.
__global__ __launch_bounds__(kStrandTPB) void strand_select_write_kernel(const uint8_t* __restrict__ outcome, uint32_t n, uint32_t span,
                                                                         const uint32_t* __restrict__ blk_cnt,
                                                                         uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
  __shared__ uint32_t s_w[kStrandTPB / 64], s_red[kStrandTPB / 64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t part = 0;
  for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kStrandTPB) part += blk_cnt[b];
  for (int o = 32; o > 0; o >>= 1) part += (uint32_t)__shfl_xor((int)part, o);
  if (lane == 0u) s_red[wave] = part;
  __syncthreads();
  uint32_t running = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  const uint32_t first = blockIdx.x * span;
  const uint32_t end = n - first < span ? n : first + span;
  for (uint32_t r0 = first; r0 < end; r0 += kStrandTPB) {
    const uint32_t r = r0 + threadIdx.x;
    const bool pick = r < end && outcome[r] == (uint8_t)kConstantRegion;
    const unsigned long long m = __ballot(pick);
    if (lane == 0u) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kStrandTPB / 64; ++w) {
      before += w < wave ? s_w[w] : 0u;
      total += s_w[w];
    }
    if (pick) list[running + before + strand_rank(m)] = r;
    running += total;
    __syncthreads();
  }
  if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0u) *count = running;
}

// ---- the fix-up, one thread each.  stats: [0] retried, [1] matched_reverse, [2] counters[BC_MATCHED] as the reverse
// pass found it ----

// ahead of the reverse pass over m reads; take_out: the pass counts reads that pass 1 has counted already (`both`)
__global__ void strand_before_kernel(unsigned long long* __restrict__ counters, unsigned long long* __restrict__ stats,
                                     unsigned long long m, uint32_t take_out) {
  if (blockIdx.x != 0u || threadIdx.x != 0u) return;
  if (take_out) {
    counters[kConstantRegion] -= m;
    counters[kTotalReads] -= m;
  }
  stats[0] += m;
  stats[2] = counters[kMatched];
}

__global__ void strand_after_kernel(const unsigned long long* __restrict__ counters, unsigned long long* __restrict__ stats) {
  if (blockIdx.x != 0u || threadIdx.x != 0u) return;
  stats[1] += counters[kMatched] - stats[2];
}

// the reverse pass's trace (entry j: read list[j] of the chunk) to the reads' own positions
__global__ __launch_bounds__(kStrandTPB) void strand_scatter_kernel(const uint32_t* __restrict__ list, uint32_t m,
                                                                    const uint8_t* __restrict__ outcome2, const uint64_t* __restrict__ idx2,
                                                                    uint8_t* __restrict__ outcome, uint64_t* __restrict__ idx) {
  for (uint32_t j = blockIdx.x * kStrandTPB + threadIdx.x; j < m; j += gridDim.x * kStrandTPB) {
    const uint32_t r = list[j];
    outcome[r] = outcome2[j];
    if (idx) idx[r] = idx2[j];
  }
}

#endif  // __HIPCC__

}  // namespace bc
