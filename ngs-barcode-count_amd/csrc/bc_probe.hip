// bc_probe.hip -- what the C ABI (include/barcode_count_hip.h) offers beside an engine's counting: dense tables packed
// to bytes and summed for the exchange between GPUs, the box diagnostics (atomic rate, shader clock) and bc_fix_error.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/barcode_count_hip.h"
#include "bc_kernel.h"
#include "bc_engine_impl.h"

namespace bc {

// dense u32 counts -> one byte each (what fits) + a list of the rest: the form in which tables travel
// between GPUs (most counts of a DEL run are small, and a quarter of the bytes is a quarter of the time
// on a link)
// (bits, may be NULL: two-level counting not folded -- the count of entry i is table[i] + bit i; reading both here
// spares the exchange a fold pass over the whole table)
__global__ void table_pack_u8_kernel(const uint32_t* __restrict__ table, const uint32_t* __restrict__ bits, uint64_t n,
                                     uint8_t* __restrict__ out, unsigned long long* cursor,
                                     unsigned long long* __restrict__ ovf_idx, uint32_t* __restrict__ ovf_val, uint64_t capacity) {
  const uint64_t n4 = n >> 2;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n4; i += step) {  // four counts in, four bytes out
    const uint4 v = reinterpret_cast<const uint4*>(table)[i];
    const uint32_t four = bits ? (bits[i >> 3] >> ((uint32_t)(i & 7u) * 4u)) & 15u : 0u;
    const uint32_t c[4] = {v.x + (four & 1u), v.y + ((four >> 1) & 1u), v.z + ((four >> 2) & 1u), v.w + (four >> 3)};
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c[k] <= 255u) {
        packed |= c[k] << (8 * k);
      } else {
        const unsigned long long p = atomicAdd(cursor, 1ull);
        if (p < capacity) {
          ovf_idx[p] = i * 4 + k;
          ovf_val[p] = c[k];
        }
      }
    }
    reinterpret_cast<uint32_t*>(out)[i] = packed;
  }
  for (i = (n4 << 2) + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const uint32_t c = table[i] + (bits ? (bits[i >> 5] >> (i & 31)) & 1u : 0u);
    if (c <= 255u) {
      out[i] = (uint8_t)c;
    } else {
      out[i] = 0;
      const unsigned long long p = atomicAdd(cursor, 1ull);
      if (p < capacity) {
        ovf_idx[p] = i;
        ovf_val[p] = c;
      }
    }
  }
}

// the receiving side: out[i] = sum over the `rows` byte slices of row[r][i]  (i < n, n a multiple of 4)
__global__ void table_sum_u8_kernel(const uint8_t* __restrict__ rows, uint32_t n_rows, uint64_t n, uint32_t* __restrict__ out) {
  const uint64_t n4 = n >> 2;
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
  for (; i < n4; i += step) {
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (uint32_t r = 0; r < n_rows; ++r) {
      const uint32_t v = reinterpret_cast<const uint32_t*>(rows + (uint64_t)r * n)[i];
      a0 += v & 0xFFu;
      a1 += (v >> 8) & 0xFFu;
      a2 += (v >> 16) & 0xFFu;
      a3 += v >> 24;
    }
    reinterpret_cast<uint4*>(out)[i] = make_uint4(a0, a1, a2, a3);
  }
}

// box diagnostic: no-return atomic adds of `delta` to random counters of a table -- the rate the memory system
// sustains for the match kernel's counting alone (bc_probe_atomic_rate: one pass of +1, one of -1 over the same
// addresses, so the counts end as they were)
__global__ void atomic_probe_kernel(uint32_t* table, uint64_t entries, uint32_t per, uint64_t seed, uint32_t delta) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t i = 0; i < per; ++i) atomicAdd(&table[hash64(seed + t * per + i) % entries], delta);
}

// shader clock probe: one wave spins for ~0.3 ms and reports (shader clock ticks, 100 MHz reference ticks)
__global__ void sclk_probe_kernel(unsigned long long* out) {
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long c0 = __builtin_readcyclecounter();
  unsigned long long r1 = r0;
  uint32_t x = threadIdx.x;
  while (r1 - r0 < 30000ull) {  // 0.3 ms at 100 MHz
    for (int i = 0; i < 256; ++i) x = x * 1664525u + 1013904223u;
    r1 = __builtin_amdgcn_s_memrealtime();
  }
  const unsigned long long c1 = __builtin_readcyclecounter();
  if (threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = r1 - r0;
    out[2] = x;
  }
}

}  // namespace bc

using namespace bc;

extern "C" {

int bc_table_pack_u8(const void* d_table_u32, uint64_t n, void* d_out_u8, void* d_ovf_idx_u64, void* d_ovf_val_u32,
                     uint64_t ovf_capacity, uint64_t* n_ovf, int device_id, void* hip_stream) {
  return bc_internal_table_pack_u8(d_table_u32, nullptr, n, d_out_u8, d_ovf_idx_u64, d_ovf_val_u32, ovf_capacity, n_ovf, device_id,
                                   hip_stream);
}

// (not part of the documented ABI) the same with the first-occurrence bit map of two-level counting read alongside:
// what travels is table + bit, without a fold pass first (bc_comm.hip)
int bc_internal_table_pack_u8(const void* d_table_u32, const void* d_bits, uint64_t n, void* d_out_u8, void* d_ovf_idx_u64,
                              void* d_ovf_val_u32, uint64_t ovf_capacity, uint64_t* n_ovf, int device_id, void* hip_stream) {
  if (n_ovf) *n_ovf = 0;
  if (n == 0) return BC_OK;
  if (!d_table_u32 || !d_out_u8 || ((uintptr_t)d_table_u32 & 15) || ((uintptr_t)d_out_u8 & 3)) {
    set_error("bc_table_pack_u8: null or misaligned buffer (table 16-byte, output 4-byte aligned)");
    return BC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device_id));
  hipStream_t st = (hipStream_t)hip_stream;
  ScratchGuard g;
  unsigned long long* d_n = nullptr;
  HIP_TRY(g.dmalloc(&d_n, 8));
  HIP_TRY(hipMemsetAsync(d_n, 0, 8, st));
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n / 4 + 255) / 256 + 1, 256ull * 64);
  hipLaunchKernelGGL(table_pack_u8_kernel, dim3(grid), dim3(256), 0, st, (const uint32_t*)d_table_u32, (const uint32_t*)d_bits, n, (uint8_t*)d_out_u8, d_n,
                     (unsigned long long*)d_ovf_idx_u64, (uint32_t*)d_ovf_val_u32, d_ovf_idx_u64 && d_ovf_val_u32 ? ovf_capacity : 0);
  HIP_TRY(hipGetLastError());
  unsigned long long cnt = 0;
  HIP_TRY(hipMemcpyAsync(&cnt, d_n, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (n_ovf) *n_ovf = cnt;
  return BC_OK;
}

int bc_table_sum_u8(const void* d_rows_u8, uint32_t n_rows, uint64_t n, void* d_out_u32, int device_id, void* hip_stream) {
  if (n == 0) return BC_OK;
  if (!d_rows_u8 || !d_out_u32 || (n & 3) || ((uintptr_t)d_rows_u8 & 3) || ((uintptr_t)d_out_u32 & 15)) {
    set_error("bc_table_sum_u8: null or misaligned buffer, or a slice length that is not a multiple of 4");
    return BC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device_id));
  hipStream_t st = (hipStream_t)hip_stream;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n / 4 + 255) / 256, 256ull * 64);
  hipLaunchKernelGGL(table_sum_u8_kernel, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_rows_u8, n_rows, n, (uint32_t*)d_out_u32);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return BC_OK;
}

int bc_probe_atomic_rate(int device_id, void* d_table_u32, uint64_t entries, uint64_t n_atomics, double* atomics_per_s) {
  *atomics_per_s = 0.0;
  if (!d_table_u32 || entries == 0 || n_atomics == 0) {
    set_error("bc_probe_atomic_rate: null table or nothing to do");
    return BC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device_id));
  const uint32_t per = 16;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_atomics / per + 255) / 256, 1u << 20);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, 0));
  hipLaunchKernelGGL(atomic_probe_kernel, dim3(blocks), dim3(256), 0, 0, (uint32_t*)d_table_u32, entries, per, 2ull, 1u);
  HIP_TRY(hipEventRecord(e1, 0));
  hipLaunchKernelGGL(atomic_probe_kernel, dim3(blocks), dim3(256), 0, 0, (uint32_t*)d_table_u32, entries, per, 2ull, 0xFFFFFFFFu);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (ms > 0.f) *atomics_per_s = (double)blocks * 256.0 * per / (ms * 1e-3);
  return BC_OK;
}

int bc_engine_sclk_mhz(bc_engine* e, double* mhz) {
  *mhz = 0.0;
  HIP_TRY(hipSetDevice(e->device));
  unsigned long long* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 24));
  hipLaunchKernelGGL(sclk_probe_kernel, dim3(1), dim3(64), 0, e->stream, d);
  HIP_TRY(hipGetLastError());
  unsigned long long h[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(h, d, 24, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  (void)hipFree(d);
  if (h[1]) *mhz = 100.0 * (double)h[0] / (double)h[1];
  return BC_OK;
}

// classify one ASCII string into planes; returns false if longer than 32
static bool pack_query(const char* s, uint32_t& q1, uint32_t& q2, uint32_t& qn, uint32_t& qx, uint32_t& len) {
  q1 = q2 = qn = qx = 0;
  len = (uint32_t)strlen(s);
  if (len > 32) return false;
  for (uint32_t i = 0; i < len; ++i) {
    const char c = s[i];
    if (c == 'N')
      qn |= 1u << i;
    else if (c == 'A' || c == 'C' || c == 'G' || c == 'T') {
      q1 |= (uint32_t)((c >> 1) & 1) << i;
      q2 |= (uint32_t)((c >> 2) & 1) << i;
    } else {
      qx |= 1u << i;
    }
  }
  return true;
}

int64_t bc_fix_error(const char* mismatch_seq, const char* const* possible_seqs, uint64_t n, uint16_t mismatches,
                     int device_id) {
  uint32_t q1, q2, qn, qx, qlen;
  if (!pack_query(mismatch_seq, q1, q2, qn, qx, qlen)) {
    set_error("bc_fix_error: sequences longer than 32 bases are not supported");
    return BC_ERR_UNSUPPORTED - 1;
  }
  std::vector<uint32_t> r1(n), r2(n), rn(n);
  std::vector<uint8_t> rl(n);
  for (uint64_t j = 0; j < n; ++j) {
    uint32_t x, l;
    if (!pack_query(possible_seqs[j], r1[j], r2[j], rn[j], x, l) || x) {
      set_error("bc_fix_error: candidates must be A,C,G,T,N strings of at most 32 bases");
      return BC_ERR_UNSUPPORTED - 1;
    }
    rl[j] = (uint8_t)l;
  }
  if (hipSetDevice(device_id) != hipSuccess) {
    set_error("bc_fix_error: no HIP device (the engine has no CPU path)");
    return BC_ERR_HIP - 1;
  }
  DevGroup G;
  memset(&G, 0, sizeof G);
  G.len = qlen;
  G.n_refs = (uint32_t)n;
  G.max_err = mismatches;
  void *d1 = nullptr, *d2 = nullptr, *dn = nullptr, *dl = nullptr, *dout = nullptr;
  bool ok = hipMalloc(&d1, n * 4 + 16) == hipSuccess && hipMalloc(&d2, n * 4 + 16) == hipSuccess &&
            hipMalloc(&dn, n * 4 + 16) == hipSuccess && hipMalloc(&dl, n + 16) == hipSuccess &&
            hipMalloc(&dout, 16) == hipSuccess;
  uint32_t out = kFail;
  if (ok && n) {
    ok = hipMemcpy(d1, r1.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d2, r2.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dn, rn.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dl, rl.data(), n, hipMemcpyHostToDevice) == hipSuccess;
  }
  if (ok) {
    G.r1_a = (uint64_t)(uintptr_t)d1;
    G.r2_a = (uint64_t)(uintptr_t)d2;
    G.rn_a = (uint64_t)(uintptr_t)dn;
    G.rlen_a = (uint64_t)(uintptr_t)dl;
    fix_error_launch(G, q1, q2, qn, qx, (uint32_t*)dout);
    ok = hipGetLastError() == hipSuccess && hipMemcpy(&out, dout, 4, hipMemcpyDeviceToHost) == hipSuccess;
  }
  (void)hipFree(d1);
  (void)hipFree(d2);
  (void)hipFree(dn);
  (void)hipFree(dl);
  (void)hipFree(dout);
  if (!ok) {
    set_error(std::string("bc_fix_error: HIP failure: ") + hipGetErrorString(hipGetLastError()));
    return BC_ERR_HIP - 1;
  }
  return out == kFail ? -1 : (int64_t)out;
}

}  // extern "C"
