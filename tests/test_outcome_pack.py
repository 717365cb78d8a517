"""The packed outcome counters of the specialised match kernels (bc_device_plan.h outcome_pack / outcome_split /
outcome_fold), compiled for the host: a lane adds one per tile to one 8-bit field and the wave adds its 64 lanes up
every kPackTiles tiles over 16-bit halves.  The run is as long as a field allows -- kPackTiles = 2^8 - 1 tiles with
every lane on ONE outcome, which fills that field to its last value and the wave's half to 64 x 255 -- and checks that
nothing carries into a neighbouring field; one tile more must be seen to overflow, which is what bounds kPackTiles."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include "bc_device_plan.h"
using namespace bc;
// the wave's counters after `tiles` tiles in which lane l has outcome pick(l, t); 64 lanes, inactive ones count nothing
template <class F>
static void run(uint32_t tiles, F pick, uint32_t (&acc)[kNCounters]) {
  uint64_t pk[64] = {};
  for (uint32_t t = 0; t < tiles; ++t)
    for (uint32_t l = 0; l < 64; ++l) {
      const int o = pick(l, t);
      pk[l] += outcome_pack(o >= 0, o >= 0 ? (uint32_t)o : 0u);
    }
  uint32_t sums[4] = {};
  for (uint32_t l = 0; l < 64; ++l) {
    uint32_t w[4];
    outcome_split(pk[l], w);
    for (int j = 0; j < 4; ++j) sums[j] += w[j];
  }
  for (int k = 0; k < kNCounters; ++k) acc[k] = 0;
  outcome_fold(sums, acc);
}
int main() {
  static_assert(kPackTiles == 255u, "one less than an 8-bit field holds");
  int bad = 0;
  for (int k = 0; k < kNCounters; ++k) {  // every lane on outcome k for as long as a field allows
    uint32_t acc[kNCounters];
    run(kPackTiles, [k](uint32_t, uint32_t) { return k; }, acc);
    for (int j = 0; j < kNCounters; ++j) {
      const uint32_t want = (j == k && k != kTotalReads) ? 64u * kPackTiles : 0u;  // (field 6: kPending, never counted)
      if (acc[j] != want) { printf("outcome %d field %d: %u, not %u\n", k, j, acc[j], want); ++bad; }
    }
  }
  {  // a mix, inactive lanes among it: each lane's outcome changes from tile to tile
    uint32_t acc[kNCounters], want[kNCounters] = {};
    auto pick = [](uint32_t l, uint32_t t) { return (l * 7u + t * 3u) % 9u == 8u ? -1 : (int)((l * 7u + t * 3u) % 9u); };
    for (uint32_t t = 0; t < kPackTiles; ++t)
      for (uint32_t l = 0; l < 64; ++l)
        if (pick(l, t) >= 0 && pick(l, t) != kTotalReads) ++want[pick(l, t)];
    run(kPackTiles, pick, acc);
    for (int j = 0; j < kNCounters; ++j)
      if (acc[j] != want[j]) { printf("mix field %d: %u, not %u\n", j, acc[j], want[j]); ++bad; }
  }
  {  // one tile past the bound carries into the next field: the bound is tight
    uint32_t acc[kNCounters];
    run(kPackTiles + 1u, [](uint32_t, uint32_t) { return 0; }, acc);
    if (acc[0] == 64u * (kPackTiles + 1u)) { printf("256 tiles did not overflow an 8-bit field?\n"); ++bad; }
  }
  printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
"""


def test_fields_hold_the_longest_run_between_two_sums(tmp_path):
    src = tmp_path / "pack.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "pack")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", exe, str(src)])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout
