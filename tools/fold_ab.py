"""The count-log fold alone, variants of csrc/bc_fold.h interleaved on ONE box: a config-3-like log (100 M entries over
954 buckets, 11 % kLogNone) folded in fresh mode, as bench.py's step folds it, through builds of
tests/fold/fold_fresh_harness.hip against different headers:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I<dir with the variant's bc_fold.h> -Ings-barcode-count_amd/csrc \
          -o variant.so tests/fold/fold_fresh_harness.hip
    python tools/fold_ab.py parent.so new.so ...
Every variant must leave the same bit map, table and dirty map; the figure is the wall time of a fold (its five or six
launches and the harness's synchronise), twelve rounds of five folds per variant."""
import ctypes as C, os, sys, time
import torch
libs = {}
for path in sys.argv[1:]:
    nme = os.path.basename(path).replace(".so", "")
    L = C.CDLL(os.path.abspath(path))
    L.fold_fresh_harness_run.restype = C.c_int
    L.fold_fresh_harness_run.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    libs[nme] = L
dev = "cuda"
entries = 954 * (1 << 22) - 12345
n = 100_000_000
g = torch.Generator(device=dev); g.manual_seed(1)
log = torch.randint(0, entries, (n,), generator=g, device=dev, dtype=torch.int64)
none = torch.rand(n, generator=g, device=dev) < 0.11
log[none] = 0xFFFFFFFF
log = log.to(torch.int32)
del none
n_words = (entries + 31) // 32
nb = (entries + (1 << 22) - 1) >> 22
bits = torch.zeros(n_words + 64, dtype=torch.int32, device=dev)
table = torch.zeros(entries + 64, dtype=torch.int32, device=dev)
dirty = torch.zeros(entries // 64 + 256, dtype=torch.uint8, device=dev)
grouped = torch.zeros(n + 64, dtype=torch.int32, device=dev)
meta = torch.zeros(4 * 1025 + 64, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
def run(L):
    rc = L.fold_fresh_harness_run(log.data_ptr(), n, grouped.data_ptr(), meta.data_ptr(), nb, bits.data_ptr(), n_words,
                                  table.data_ptr(), dirty.data_ptr(), 0, 0, 1)
    assert rc == 0, rc
ref = None
for nme, L in libs.items():
    table.zero_(); torch.cuda.synchronize()
    run(L)
    sig = (int(bits.to(torch.int64).sum()), int(table[:entries:1].to(torch.int64).sum()), int(dirty.to(torch.int64).sum()))
    print(nme, "signature", sig, flush=True)
    ref = ref or sig
    assert sig == ref
rows = {k: [] for k in libs}
for r in range(12):
    order = list(libs.items()) if r % 2 == 0 else list(libs.items())[::-1]
    for nme, L in order:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            run(L)
        rows[nme].append((time.perf_counter() - t0) * 1e3 / 5)
for nme, v in rows.items():
    s = sorted(v)
    print("%-8s min %.3f med %.3f max %.3f ms per fold" % (nme, s[0], s[len(s) // 2], s[-1]))
