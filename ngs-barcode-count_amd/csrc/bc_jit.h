// bc_jit.h -- the scheme-specialised match kernel (bc_jit.hip): which kernel shape a batch needs, the plan edits both
// the engine and the ahead-of-time build apply, and the compiled, cached and loaded kernels of one engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "bc_plan.hpp"

namespace bc {

// The env-driven edits of a freshly lowered plan (BC_ABLATE, BC_LHASH in experiment builds) and the bit-map layout:
// tables too large for the memory-side cache get the first-occurrence bit map (bc_kernel.h: two-level counting), and,
// when the engine owns the table, the dirty-block map behind it (the plan the kernels read holds its offset, dirty_off).
struct PlanSetup {
  int lhash_mode = 1;        // LDS exact-match tables: 0 never, 1 in the specialised kernel, 2 in both (BC_LHASH=0|1|2)
  uint64_t n_bit_words = 0;  // words of the bit map (0: none)
  uint64_t dirty_bytes = 0;  // bytes of the dirty-block map: one flag per 64 entries (0: none)
};
PlanSetup plan_setup(HostDevPlan& h, bool long_only, bool own_table);

// the generic kernel instantiation a read length falls into: 32-base words per read (4 / 8 / 10)
inline int generic_nw(uint32_t maxlen) { return maxlen <= 128 ? 4 : (maxlen <= 256 ? 8 : 10); }

// The specialised kernel's compile-time shape
struct JitShape {
  int NW, NWW;  // exact words per read / words of candidate offsets of the batch shape
  bool lens, tables, trace;
  bool qshare = false;        // quality filter with the pipelined fetch: sequence and quality lines share one LDS region
  uint32_t stride, read_len, region;
  bool conservative = false;  // last try after builds that needed scratch memory: the loop-based counting form
  int min_waves = 3;          // waves per SIMD the register allocation must leave room for (__launch_bounds__)
};

// What a launch fixes beneath the shape key: how its reads are counted and whether the workgroups keep a hot-counter
// cache.  A log-mode launch gets a kernel compiled for its variant (JIT_COUNT=1, JIT_HOT: bc_kernel.h), which carries
// no counting atomic, bit-map probe or, with the cache off, cache.  A launch of the atomic path gets the source as it
// always was, count and cache as launch arguments: one object for both its variants (jit_defines).  The variant is
// part of the code object's cache name, not of MatchShape::key.
struct JitVariant {
  int count;  // 1: through the count log; 2: counting atomics
  bool hot;   // hot-counter cache
  uint32_t id() const { return count == 1 ? (hot ? 3u : 2u) : 0u;  }  // (the engine's map: one entry per code object)
};
// the variant of a launch: use_log / hot_on as launch_match decides them
inline JitVariant jit_variant(const struct MatchShape& s, bool use_log, bool hot_on);

// What a match launch derives from the plan and the batch shape, for the generic kernel and the specialised one
struct MatchShape {
  int generic_nw;                   // the generic instantiation's NW
  uint32_t region;                  // per-wave LDS region: 64 reads + the few bytes past them the lane code may touch
  uint32_t lds, lds_jit;            // dynamic LDS of the generic / specialised kernel
  uint32_t lds_cold, lds_jit_cold;  // ... of a launch with the hot-counter cache off (the same where a plan has none)
  bool tables_generic, tables_jit;  // LDS exact-match tables
  bool hot_generic, hot_jit;        // hot-counter cache (log mode may still switch it off per launch: lds_cold)
  bool pipe;                        // the tile fetch the LDS figures are for: software-pipelined, or on demand
  JitShape jit;
  int first_min_waves;              // waves per SIMD the specialised build tries first
  uint64_t key;                     // the engine's key for the specialised kernel of this shape
};
// table_entries: 0 for sparse plans; read_len: ignored with per-read lengths (lens); trace: per-read outcomes recorded;
// qshare: the specialised kernel of a plan with the quality filter and the pipelined fetch gets one tile region per
// wave, not two
MatchShape match_shape(const DevPlan& P, uint64_t table_entries, uint32_t stride, uint32_t read_len, bool lens, bool trace,
                       uint32_t lds_limit, bool pipe, bool qshare, int lhash_mode);
// BC_QUAL_REGION=own|shared (default shared): what engines and the ahead-of-time build pass as qshare
bool qual_region_shared();
inline JitVariant jit_variant(const MatchShape& s, bool use_log, bool hot_on) {
  return JitVariant{use_log ? 1 : 2, s.hot_jit && hot_on};
}

// scheme-specialised kernels of one engine, one per MatchShape::key and variant; destruction joins the workers and unloads the
// modules
struct JitKernels {
  struct Jit {
    enum { kIdle = 0, kCompiling = 1, kCodeReady = 2, kLoaded = 3, kFailed = -1 };
    std::atomic<int> state{kIdle};
    std::thread worker;      // compiles in the background while the generic kernel keeps counting
    std::vector<char> code;  // written by the worker before it publishes kCodeReady
    std::string log;
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    int per_cu = 0, per_cu_cold = 0;  // workgroups per CU at lds_jit / lds_jit_cold
  };
  std::map<std::pair<uint64_t, uint32_t>, std::unique_ptr<Jit>> slots;  // (shape key, JitVariant::id)

  JitKernels() = default;
  JitKernels(const JitKernels&) = delete;
  JitKernels& operator=(const JitKernels&) = delete;
  ~JitKernels();
  // The specialised kernel of one shape, if it can be had now (mode: BC_JIT as bc_engine::jit_mode reads it;
  // reads_seen: reads submitted so far; v: the launch's variant, *per_cu: the workgroups a CU holds of such a launch).
  // Returns nullptr while the generic kernel must do.
  hipFunction_t function(const DevPlan& plan, int device, int mode, uint64_t reads_seen, const MatchShape& s, const JitVariant& v,
                         int* per_cu);
};

}  // namespace bc
