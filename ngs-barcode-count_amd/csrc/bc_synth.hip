// bc_synth.hip -- the synthetic read generator behind bc_synth_* (include/barcode_count_hip.h): the same reads on the
// host and on the device (bc_synth.h).  It needs nothing of the engine.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/barcode_count_hip.h"
#include "bc_engine_impl.h"
#include "bc_synth.h"

namespace bc {

__global__ void synth_kernel(SynthDev S, uint64_t first, uint64_t n, uint8_t* __restrict__ seq,
                             uint8_t* __restrict__ qual, uint32_t stride) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint64_t i = first + t;
  SynthRead R;
  synth_begin(S, i, R);
  uint8_t* so = seq + t * stride;
  uint8_t* qo = qual ? qual + t * stride : nullptr;
  for (uint32_t p = 0; p < S.read_len; ++p) {
    uint8_t b, q;
    synth_byte(S, i, R, p, b, q);
    so[p] = b;
    if (qo) qo[p] = q;
  }
  for (uint32_t p = S.read_len; p < stride; ++p) {
    so[p] = '\n';
    if (qo) qo[p] = '\n';
  }
}

}  // namespace bc

using namespace bc;

struct bc_synth {
  SynthDev S;                       // host view (refs -> host memory)
  std::vector<std::string> flat;    // per group: concatenated reference bases
  int dev_device = -1;
  SynthDev D;                       // device view (refs -> device memory)
  std::vector<void*> dev_allocs;
};

extern "C" {

bc_synth* bc_synth_create(const bc_plan* p, const bc_synth_params* prm) {
  if (!p || !prm) {
    set_error("bc_synth_create: null argument");
    return nullptr;
  }
  if (!p->unsupported.empty() || p->length > (uint32_t)kSynthMaxL || p->groups.size() > (size_t)kMaxGroups) {
    set_error("bc_synth_create: scheme not supported by the generator");
    return nullptr;
  }
  if (prm->read_len <= p->length || prm->phred_hi < prm->phred_lo || prm->lowq_hi < prm->lowq_lo) {
    set_error("bc_synth_create: read_len must exceed the format length; Phred ranges must be ordered");
    return nullptr;
  }
  bc_synth* s = new bc_synth();
  SynthDev& S = s->S;
  memset(&S, 0, sizeof S);
  S.seed = prm->seed;
  S.read_len = prm->read_len;
  S.L = p->length;
  S.p_sub = prm->p_sub;
  S.p_n = prm->p_n;
  S.p_lowq = prm->p_lowq;
  S.phred_lo = prm->phred_lo;
  S.phred_hi = prm->phred_hi;
  S.lowq_lo = prm->lowq_lo;
  S.lowq_hi = prm->lowq_hi;
  S.n_molecules = prm->n_molecules;
  S.zipf = prm->zipf;
  S.geo_total = prm->geo_total;
  S.n_groups = (uint32_t)p->groups.size();
  s->flat.resize(S.n_groups);
  for (uint32_t g = 0; g < S.n_groups; ++g) {
    const auto& fg = p->groups[g];
    SynthGroup& G = S.groups[g];
    G.type = fg.type;
    G.off = fg.off;
    G.len = fg.len;
    const KnownSet* set = nullptr;
    if (fg.type == kGroupSample && p->samples.size()) set = &p->samples;
    if (fg.type == kGroupBarcode && p->counted_loaded) set = &p->counted[fg.number - 1];
    if (fg.type != kGroupRandom) S.n_sb++;
    if (set) {
      for (const auto& q : set->seqs) {
        if (q.size() != fg.len) {
          set_error("bc_synth_create: every known barcode must have the length of its group");
          delete s;
          return nullptr;
        }
        s->flat[g] += q;
      }
      G.n_refs = (uint32_t)set->size();
      // a multiplier coprime to the set size: rank -> reference index is then a bijection
      uint32_t mul = G.n_refs > 2 ? 2654435761u % G.n_refs : 1u;
      auto gcd = [](uint32_t a, uint32_t b) {
        while (b) {
          const uint32_t t = a % b;
          a = b;
          b = t;
        }
        return a;
      };
      if (G.n_refs > 2) {
        while (mul < 2u || gcd(mul, G.n_refs) != 1u) mul = mul + 1u >= G.n_refs ? 2u : mul + 1u;  // n - 1 is coprime to n
      } else {
        mul = 1u;
      }
      G.zmul = mul;
    }
  }
  for (uint32_t g = 0; g < S.n_groups; ++g) S.groups[g].refs = s->flat[g].data();
  for (uint32_t i = 0; i < p->pos.size(); ++i) {
    const auto& fp = p->pos[i];
    S.fmt[i] = fp.kind == kPosConst ? (uint8_t)fp.letter : (fp.kind == kPosFmtN ? (uint8_t)'n' : (uint8_t)(0x80 | fp.group));
  }
  return s;
}

void bc_synth_destroy(bc_synth* s) {
  if (!s) return;
  if (s->dev_device >= 0) {
    (void)hipSetDevice(s->dev_device);
    for (void* p : s->dev_allocs) (void)hipFree(p);
  }
  delete s;
}

int bc_synth_generate_host(bc_synth* s, uint64_t first, uint64_t n, void* seq, void* qual, uint32_t stride) {
  if (stride < s->S.read_len) {
    set_error("bc_synth_generate: stride below read_len");
    return BC_ERR_INVALID;
  }
  uint8_t* so = (uint8_t*)seq;
  uint8_t* qo = (uint8_t*)qual;
  for (uint64_t t = 0; t < n; ++t) {
    SynthRead R;
    synth_begin(s->S, first + t, R);
    for (uint32_t p = 0; p < s->S.read_len; ++p) {
      uint8_t b, q;
      synth_byte(s->S, first + t, R, p, b, q);
      so[t * stride + p] = b;
      if (qo) qo[t * stride + p] = q;
    }
    for (uint32_t p = s->S.read_len; p < stride; ++p) {
      so[t * stride + p] = '\n';
      if (qo) qo[t * stride + p] = '\n';
    }
  }
  return BC_OK;
}

int bc_synth_generate_device(bc_synth* s, int device_id, void* hip_stream, uint64_t first, uint64_t n, void* d_seq,
                             void* d_qual, uint32_t stride) {
  if (stride < s->S.read_len) {
    set_error("bc_synth_generate: stride below read_len");
    return BC_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device_id));
  if (s->dev_device != device_id) {
    for (void* p : s->dev_allocs) (void)hipFree(p);
    s->dev_allocs.clear();
    s->D = s->S;
    for (uint32_t g = 0; g < s->S.n_groups; ++g) {
      void* d = nullptr;
      HIP_TRY(hipMalloc(&d, s->flat[g].size() + 16));
      s->dev_allocs.push_back(d);
      if (!s->flat[g].empty()) HIP_TRY(hipMemcpy(d, s->flat[g].data(), s->flat[g].size(), hipMemcpyHostToDevice));
      s->D.groups[g].refs = (const char*)d;
    }
    s->dev_device = device_id;
  }
  if (n == 0) return BC_OK;
  const uint64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(synth_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)hip_stream, s->D, first, n,
                     (uint8_t*)d_seq, (uint8_t*)d_qual, stride);
  HIP_TRY(hipGetLastError());
  return BC_OK;
}

int bc_synth_make_set(uint64_t seed, uint32_t n, uint32_t k, uint32_t min_dist, char* out) {
  if (k == 0 || k > 32 || (k < 16 && (uint64_t)n > (1ull << (2 * k)))) {
    set_error("bc_synth_make_set: cannot draw that many distinct k-mers");
    return BC_ERR_INVALID;
  }
  std::vector<uint64_t> acc;  // 2 bits per base
  acc.reserve(n);
  const uint64_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
  uint64_t ctr = 0;
  while (acc.size() < n) {
    if (ctr > 400ull * n + 100000) {
      set_error("bc_synth_make_set: could not place the requested k-mers at that minimum distance");
      return BC_ERR_INVALID;
    }
    const uint64_t c = synth_mix(seed ^ 0xB0C0DEull, ctr++, k) & mask;
    bool ok = true;
    for (uint64_t a : acc) {
      const uint64_t x = a ^ c;
      const uint64_t diff = (x | (x >> 1)) & 0x5555555555555555ull;
      if ((uint32_t)__builtin_popcountll(diff) < std::max(min_dist, 1u)) {
        ok = false;
        break;
      }
    }
    if (ok) acc.push_back(c);
  }
  const char* acgt = "ACGT";
  for (uint32_t i = 0; i < n; ++i) {
    for (uint32_t b = 0; b < k; ++b) out[(size_t)i * (k + 1) + b] = acgt[(acc[i] >> (2 * b)) & 3];
    out[(size_t)i * (k + 1) + k] = 0;
  }
  return BC_OK;
}

}  // extern "C"
