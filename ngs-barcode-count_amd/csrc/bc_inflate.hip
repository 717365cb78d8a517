// bc_inflate.hip -- BGZF on the device: the block index (host), the inflate kernel (one wavefront per block, the decoder
// is bc_inflate.h) and the C ABI around them: bc_bgzf_scan and bc_bgzf_inflate_device (bc_fastq_gz_record_start lives
// in bc_ingest.hip, next to the record-start rule it shares with the plain path).
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>

#include "bc_bgzf.hpp"
#include "bc_inflate.h"
#include "bc_plan.hpp"

namespace bc {

namespace {

constexpr uint32_t kWavesPerGroup = 4;

__global__ __launch_bounds__(64 * kWavesPerGroup) void bgzf_inflate_kernel(const uint8_t* __restrict__ src,
                                                                           const bc_bgzf_block* __restrict__ blocks,
                                                                           unsigned long long n_blocks, uint8_t* __restrict__ dst,
                                                                           uint32_t* __restrict__ status) {
  __shared__ InflateTables s_tab[kWavesPerGroup];
  __shared__ uint32_t s_crc[256];
  s_crc[threadIdx.x] = crc32_table_entry(threadIdx.x);
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned long long b = (unsigned long long)blockIdx.x * kWavesPerGroup + wave;
  if (b >= n_blocks) return;
  const bc_bgzf_block blk = blocks[b];
  const uint32_t st = inflate_member((const BC_GLOBAL uint8_t*)(src + blk.src_off), blk.src_len, (BC_GLOBAL uint8_t*)(dst + blk.dst_off),
                                     blk.isize, blk.crc32, s_tab[wave], s_crc, lane);
  if (lane == 0) status[b] = st;
}

__global__ void bgzf_patch_newline_kernel(uint8_t* text, unsigned long long at) { text[at] = '\n'; }

uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

}  // namespace

int bgzf_inflate_launch(void* stream, const void* d_src, const bc_bgzf_block* d_blocks, uint64_t n_blocks, void* d_dst,
                        uint32_t* d_status) {
  if (n_blocks == 0) return (int)hipSuccess;
  const uint64_t groups = (n_blocks + kWavesPerGroup - 1) / kWavesPerGroup;
  hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((uint32_t)groups), dim3(64 * kWavesPerGroup), 0, (hipStream_t)stream,
                     (const uint8_t*)d_src, d_blocks, (unsigned long long)n_blocks, (uint8_t*)d_dst, d_status);
  return (int)hipGetLastError();
}

int bgzf_patch_newline_launch(void* stream, void* d_text, uint64_t at) {
  hipLaunchKernelGGL(bgzf_patch_newline_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (uint8_t*)d_text, (unsigned long long)at);
  return (int)hipGetLastError();
}

const char* bgzf_status_name(uint32_t status) { return inflate_status_name(status); }

int bgzf_index(const std::string& path, std::vector<BgzfMember>* members, uint64_t* inflated_bytes, std::string* why) {
  members->clear();
  *inflated_bytes = 0;
  const int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) return -1;
  struct stat sb;
  if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
    close(fd);
    return -1;
  }
  const uint64_t size = (uint64_t)sb.st_size;
  if (size == 0) {
    close(fd);
    *why = "the file is empty";
    return 1;
  }
  void* map = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, fd, 0);
  close(fd);
  if (map == MAP_FAILED) return -1;
  const uint8_t* f = (const uint8_t*)map;
  uint64_t off = 0, out = 0;
  auto broke = [&](const char* what) {
    *why = std::string(what) + " in the member at byte " + std::to_string((unsigned long long)off);
    munmap(map, (size_t)size);
    members->clear();
    return 1;
  };
  while (off < size) {
    if (size - off < 18) return broke("no room for a BGZF header");
    const uint8_t* h = f + off;
    if (h[0] != 0x1F || h[1] != 0x8B) return broke("no gzip magic");
    if (h[2] != 8) return broke("not deflate (CM != 8)");
    if (h[3] != 4) return broke("FLG is not FEXTRA alone");
    const uint32_t xlen = le16(h + 10);
    if (size - off < 12ull + xlen) return broke("the extra field runs past the end of the file");
    uint32_t bsize = 0;
    bool found = false;
    for (uint32_t x = 0; x + 4 <= xlen;) {
      const uint8_t* sf = h + 12 + x;
      const uint32_t slen = le16(sf + 2);
      if (x + 4 + slen > xlen) return broke("a malformed extra subfield");
      if (sf[0] == 'B' && sf[1] == 'C' && slen == 2 && !found) {
        bsize = le16(sf + 4);
        found = true;
      }
      x += 4 + slen;
    }
    if (!found) return broke("no BC subfield");
    const uint32_t total = bsize + 1u;
    if (total < 12u + xlen + 8u) return broke("BSIZE smaller than the header and trailer");
    if (size - off < total) return broke("BSIZE runs past the end of the file");
    BgzfMember m;
    m.file_off = off;
    m.out_off = out;
    m.total = total;
    m.payload_off = 12u + xlen;
    m.payload_len = total - m.payload_off - 8u;
    m.crc32 = le32(h + total - 8);
    m.isize = le32(h + total - 4);
    if (m.isize > 65536u) return broke("ISIZE above 65536");
    members->push_back(m);
    off += total;
    out += m.isize;
  }
  munmap(map, (size_t)size);
  *inflated_bytes = out;
  return 0;
}

bool bgzf_inflate_host(int fd, const BgzfMember& m, std::vector<uint8_t>* text) {
  std::vector<uint8_t> comp(m.payload_len);
  size_t got = 0;
  while (got < comp.size()) {
    const ssize_t n = pread(fd, comp.data() + got, comp.size() - got, (off_t)(m.file_off + m.payload_off + got));
    if (n <= 0) return false;
    got += (size_t)n;
  }
  text->assign((size_t)m.isize + 1, 0);  // (one byte over: a stream that makes more than ISIZE shows as "not at its end")
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (inflateInit2(&zs, -15) != Z_OK) return false;
  zs.next_in = comp.data();
  zs.avail_in = (uInt)comp.size();
  zs.next_out = text->data();
  zs.avail_out = (uInt)text->size();
  const int rc = inflate(&zs, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && zs.total_out == m.isize;
  inflateEnd(&zs);
  text->resize(m.isize);
  return ok && (uint32_t)crc32(crc32(0L, Z_NULL, 0), text->data(), (uInt)text->size()) == m.crc32;
}

long BgzfHostReader::read_at(char* dst, size_t n, unsigned long long off) {
  size_t done = 0;
  while (done < n && off + done < inflated) {
    const unsigned long long at = off + done;
    // the last member that starts at or before `at` and is not empty there
    size_t k = (size_t)(std::upper_bound(members->begin(), members->end(), at,
                                         [](unsigned long long v, const BgzfMember& m) { return v < m.out_off; }) -
                        members->begin()) - 1;
    const BgzfMember& m = (*members)[k];
    if (cached != k) {
      cached = (size_t)-1;
      if (!bgzf_inflate_host(fd, m, &text)) return -1;
      cached = k;
    }
    const size_t in_m = (size_t)(at - m.out_off);
    const size_t take = std::min(n - done, text.size() - in_m);
    memcpy(dst + done, text.data() + in_m, take);
    done += take;
  }
  return (long)done;
}

}  // namespace bc

using namespace bc;

extern "C" int bc_bgzf_scan(const char* path, uint64_t* n_blocks, uint64_t* inflated_bytes) {
  if (n_blocks) *n_blocks = 0;
  if (inflated_bytes) *inflated_bytes = 0;
  const std::string p = path ? path : "";
  std::vector<BgzfMember> members;
  uint64_t inflated = 0;
  std::string why;
  const int rc = bgzf_index(p, &members, &inflated, &why);
  if (rc < 0) {
    set_error("Failed to open file: " + p);
    return BC_ERR_INVALID;
  }
  if (rc > 0) {
    set_error("not BGZF: " + why);
    return BC_ERR_UNSUPPORTED;
  }
  if (n_blocks) *n_blocks = members.size();
  if (inflated_bytes) *inflated_bytes = inflated;
  return BC_OK;
}

#define HIP_TRY(expr)                                               \
  do {                                                              \
    hipError_t _e = (expr);                                         \
    if (_e != hipSuccess) {                                         \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e)); \
      rc = BC_ERR_HIP;                                              \
      goto done;                                                    \
    }                                                               \
  } while (0)

extern "C" int bc_bgzf_inflate_device(int device_id, void* hip_stream, const void* d_src, uint64_t src_bytes,
                                      const bc_bgzf_block* blocks, uint64_t n_blocks, void* d_dst, uint64_t dst_bytes,
                                      uint32_t* status) {
  for (uint64_t i = 0; i < n_blocks; ++i) {
    const bc_bgzf_block& b = blocks[i];
    if (b.src_len > 65536u || b.isize > 65536u || b.src_off > src_bytes || b.src_len > src_bytes - b.src_off || b.dst_off > dst_bytes ||
        b.isize > dst_bytes - b.dst_off) {
      set_error("bc_bgzf_inflate_device: block " + std::to_string((unsigned long long)i) +
                " of the table lies outside the buffers (or is longer than a BGZF block can be)");
      return BC_ERR_INVALID;
    }
  }
  if (n_blocks == 0) return BC_OK;
  if (!d_src || !d_dst || !status) {
    set_error("bc_bgzf_inflate_device: null buffer");
    return BC_ERR_INVALID;
  }
  int rc = BC_OK;
  bc_bgzf_block* d_blocks = nullptr;
  uint32_t* d_status = nullptr;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(hipSetDevice(device_id));
  HIP_TRY(hipMalloc((void**)&d_blocks, n_blocks * sizeof(bc_bgzf_block)));
  HIP_TRY(hipMalloc((void**)&d_status, n_blocks * sizeof(uint32_t)));
  HIP_TRY(hipMemcpyAsync(d_blocks, blocks, n_blocks * sizeof(bc_bgzf_block), hipMemcpyHostToDevice, st));
  HIP_TRY((hipError_t)bgzf_inflate_launch(st, d_src, d_blocks, n_blocks, d_dst, d_status));
  HIP_TRY(hipMemcpyAsync(status, d_status, n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
done:
  if (rc != BC_OK) (void)hipStreamSynchronize(st);
  if (d_blocks) (void)hipFree(d_blocks);
  if (d_status) (void)hipFree(d_status);
  return rc;
}
