"""The count-log fold (csrc/bc_fold.h) on its own: tests/fold/fold_harness.hip runs the four fold kernels through the
engine's launch sequence (bc::fold_launch) on logs built here, and every case is checked against a numpy reference of
the fold's contract.  For each tuple with c > 0 log entries: bit clear before -> bit set, table + c - 1; bit set before
-> table + c; the dirty byte of its 64-entry block set exactly where the table changed.  Nothing else may change: not
the other words of bit map, table or dirty map, not the bits past the table's end, not the canary words after each
buffer; the grouped log holds the valid entries grouped by bucket, and the fold leaves the bucket counts (the `cnt`
section of the meta buffer) zero for the next one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "fold", "fold_harness.hip")
SO = os.path.join(ROOT, "tests", "fold", "libfold_harness.so")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("bc_fold.h", "bc_kernel.h", "bc_lane.h", "bc_intrin.h", "bc_device_plan.h")]
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")

CANARY_WORDS = 64
CANARY = 0x5A5A5A5A
CANARY_BYTE = 0xA5


def build(so=SO):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", so, SRC])
    return so


def load(so=SO):
    import torch  # noqa: F401  (first: one HIP runtime in the process, as _lib.load() arranges)
    L = C.CDLL(build(so) if so == SO else so)
    L.fold_harness_constants.restype = None
    L.fold_harness_constants.argtypes = [C.POINTER(C.c_uint64)]
    L.fold_harness_run.restype = C.c_int
    L.fold_harness_run.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    return L


def constants(L):
    out = (C.c_uint64 * 8)()
    L.fold_harness_constants(out)
    return dict(zip(("none", "bucket_shift", "quarter_shift", "max_buckets", "tile", "chunk"), list(out)[:6]))


def test_fold_harness_cross_compiles(tmp_path):
    """no GPU needed: the harness builds against the shipped headers and reports the constants the cases below rely on"""
    so = str(tmp_path / "libfold_harness.so")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", so, SRC])
    k = constants(load(so))
    assert k["none"] == 0xFFFFFFFF
    assert k["max_buckets"] << k["bucket_shift"] == 1 << 32
    assert k["quarter_shift"] < k["bucket_shift"] and k["chunk"] >= k["tile"]


# ---------------------------------------------------------------------------------------------------------------------
# GPU cases

_K = {}


def K():
    if not _K:
        _K["lib"] = load()
        _K.update(constants(_K["lib"]))
    return _K


class Fold:
    """bit map, table, dirty map, grouped log and meta buffer of one table of `entries` tuples, each followed by canary
    words; folds logs into them and checks every fold against the reference"""

    def __init__(self, entries, log_cap, seed, dirty=True, table_max=1 << 20):
        import torch
        k = K()
        self.entries = entries
        self.n_words = (entries + 31) // 32
        self.nb = (entries + (1 << k["bucket_shift"]) - 1) >> k["bucket_shift"]
        assert 1 <= self.nb <= k["max_buckets"]
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        dev = "cuda"
        canary = torch.full((CANARY_WORDS,), CANARY, dtype=torch.int32, device=dev)
        # random bits (the ones past the table's end in the last word included) and random counts
        self.bits = torch.cat([torch.randint(-2**31, 2**31, (self.n_words,), generator=g, dtype=torch.int32, device=dev), canary])
        self.table = torch.cat([torch.randint(0, table_max, (entries,), generator=g, dtype=torch.int32, device=dev), canary])
        n_dirty = (entries + 63) // 64
        self.dirty = None
        if dirty:
            self.dirty = torch.cat([torch.zeros(n_dirty, dtype=torch.uint8, device=dev),
                                    torch.full((256,), CANARY_BYTE, dtype=torch.uint8, device=dev)])
        self.grouped = torch.full((log_cap + CANARY_WORDS,), CANARY, dtype=torch.int32, device=dev)
        self.meta = torch.cat([torch.zeros(4 * (k["max_buckets"] + 1), dtype=torch.int32, device=dev), canary])

    def set_bits(self, idx, value):
        """bit of each tuple in idx (numpy) set (value True) or cleared"""
        import torch
        for i in np.unique(np.asarray(idx, dtype=np.int64)):
            w = int(i) >> 5
            m = np.int32(np.uint32(1 << (int(i) & 31)).view(np.int32))
            cur = np.int32(self.bits[w].item())
            self.bits[w] = int(cur | m) if value else int(cur & ~m)
        torch.cuda.synchronize()

    def fold(self, log, scatter_grid=0, apply_grid=0):
        """one fold of `log` (numpy uint32), then every check"""
        import torch
        k = K()
        none = k["none"]
        log = np.ascontiguousarray(log, dtype=np.uint32)
        n = log.size
        assert n + CANARY_WORDS <= self.grouped.numel()
        valid = log[log != none]
        assert valid.size == 0 or int(valid.max()) < self.entries
        # ---- reference: counts per tuple, from the state before
        idx, c = np.unique(valid.astype(np.int64), return_counts=True)
        idx_t = torch.from_numpy(idx).cuda()
        w_t = idx_t >> 5
        bits_at = self.bits[w_t].cpu().numpy().view(np.uint32)
        was_set = (bits_at >> (idx & 31).astype(np.uint32)) & 1
        add = c.astype(np.int64) - 1 + was_set.astype(np.int64)
        table_new = (self.table[idx_t].cpu().numpy().view(np.uint32).astype(np.int64) + add).astype(np.uint32)
        words = idx >> 5
        first = np.flatnonzero(np.r_[True, words[1:] != words[:-1]]) if idx.size else np.zeros(0, np.int64)
        mask = (np.uint32(1) << (idx & 31).astype(np.uint32)).astype(np.uint32)
        words_new = bits_at[first] | np.bitwise_or.reduceat(mask, first) if idx.size else np.zeros(0, np.uint32)
        exp_bits = self.bits.clone()
        exp_table = self.table.clone()
        if idx.size:
            exp_bits[torch.from_numpy(words[first]).cuda()] = torch.from_numpy(words_new.view(np.int32)).cuda()
            exp_table[idx_t] = torch.from_numpy(table_new.view(np.int32)).cuda()
        exp_dirty = None
        if self.dirty is not None:
            exp_dirty = self.dirty.clone()
            changed = np.unique(idx[add > 0] >> 6)
            if changed.size:
                exp_dirty[torch.from_numpy(changed).cuda()] = 1
        # ---- the fold (what an earlier fold left in `grouped` is canaries again: nothing past this fold's entries may
        # be written)
        self.grouped.fill_(CANARY)
        d_log = torch.from_numpy(log.view(np.int32)).cuda()
        torch.cuda.synchronize()
        rc = k["lib"].fold_harness_run(d_log.data_ptr(), n, self.grouped.data_ptr(), self.meta.data_ptr(), self.nb,
                                       self.bits.data_ptr(), self.n_words, self.table.data_ptr(),
                                       self.dirty.data_ptr() if self.dirty is not None else None, scatter_grid, apply_grid)
        assert rc == 0, "hipError %d" % rc
        # ---- checks
        assert torch.equal(self.bits, exp_bits), self._diff("bits", self.bits, exp_bits)
        assert torch.equal(self.table, exp_table), self._diff("table", self.table, exp_table)
        if exp_dirty is not None:
            assert torch.equal(self.dirty, exp_dirty), self._diff("dirty", self.dirty, exp_dirty)
        mb = k["max_buckets"] + 1
        meta = self.meta.cpu().numpy().view(np.uint32)
        assert not meta[:mb].any(), "cnt not zeroed for the next fold"
        assert (meta[4 * mb:] == CANARY).all()
        start, item_off = meta[mb:2 * mb], meta[3 * mb:4 * mb]
        per_bucket = np.bincount((valid >> np.uint32(k["bucket_shift"])).astype(np.int64), minlength=self.nb)
        assert start[self.nb] == valid.size
        assert np.array_equal(start[:self.nb + 1], np.r_[0, np.cumsum(per_bucket)])
        assert item_off[self.nb] == int(((per_bucket + k["chunk"] - 1) // k["chunk"]).sum())
        # the grouped log: the valid entries, bucket by bucket; nothing written past them
        gv = self.grouped[:valid.size].to(torch.int64) & 0xFFFFFFFF
        if valid.size:
            gb = gv >> k["bucket_shift"]
            assert bool((gb[1:] >= gb[:-1]).all())
            assert torch.equal(torch.sort(gv).values, torch.sort(torch.from_numpy(valid.astype(np.int64)).cuda()).values)
        assert bool((self.grouped[valid.size:] == CANARY).all())

    @staticmethod
    def _diff(name, got, exp):
        import torch
        bad = torch.nonzero(got != exp).flatten()[:8].tolist()
        return "%s differs at %d places, first %s: got %s, expected %s" % (
            name, int((got != exp).sum()), bad, [int(got[i]) for i in bad], [int(exp[i]) for i in bad])


GRIDS_SMALL = [(0, 0), (1, 1)]  # the engine's grids; one workgroup each for scatter and apply
SMALL_LOG = 1 << 22


def _grids(n):
    return GRIDS_SMALL if n <= SMALL_LOG else GRIDS_SMALL[:1]


def _run(entries, log, seed, prep=None, dirty=True):
    for sg, ag in _grids(log.size):
        f = Fold(entries, log.size, seed, dirty=dirty)
        if prep:
            prep(f)
        f.fold(log, sg, ag)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_tiny_logs(n):
    k = K()
    rng = np.random.default_rng(100 + n)
    entries = 3 * (1 << k["bucket_shift"]) + 1000
    log = rng.integers(0, entries, n).astype(np.uint32)
    if n >= 3:
        log[1] = log[0]  # a repeat
        log[-1] = k["none"]
    _run(entries, log, seed=n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 16384, 50_001])
def test_log_of_none_only(n):
    k = K()
    _run(2 * (1 << k["bucket_shift"]) + 77, np.full(n, k["none"], dtype=np.uint32), seed=7)


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(32))
def test_every_index_on_a_boundary(r):
    """indexes at k*2^20 - 1, k*2^20 (quarters; buckets among them) and entries - 1, once to three times each, with
    entries % 32 = r and n_words % 4 = every residue: the last uint4 of the bit map holds 1-4 words"""
    k = K()
    q = r % 4 + 4 * (r // 4) * 37
    entries = 2 * (1 << k["bucket_shift"]) + 3 * (1 << k["quarter_shift"]) + 32 * q + r
    n_words = (entries + 31) // 32
    assert entries % 32 == r
    rng = np.random.default_rng(1000 + r)
    qs = 1 << k["quarter_shift"]
    tuples = [0, entries - 1] + [j * qs + d for j in range(1, entries // qs + 1) for d in (-1, 0) if j * qs + d < entries]
    tuples = np.unique(np.array(tuples, dtype=np.int64))
    reps = rng.integers(1, 4, tuples.size)
    log = np.repeat(tuples, reps).astype(np.uint32)
    log = np.concatenate([log, np.full(17, k["none"], dtype=np.uint32)])
    rng.shuffle(log)
    preset = tuples[rng.random(tuples.size) < 0.5]

    def prep(f):
        f.set_bits(tuples, False)
        f.set_bits(preset[preset != entries - 1], True)  # the last tuple's bit stays clear: its word must be written back

    assert n_words % 4 == (r % 4 + (r > 0)) % 4  # over r = 0..31: every residue, each with several values of r
    _run(entries, log, seed=r, prep=prep)


@pytest.mark.gpu
@pytest.mark.parametrize("reps", ["chunk-1", "chunk", "chunk+1", "20*chunk+7"])
@pytest.mark.parametrize("preset", [False, True])
def test_one_tuple_repeated_around_the_chunk(reps, preset):
    """a bucket of exactly kFoldChunk entries has one (owner) item; one more entry splits it"""
    k = K()
    ch = k["chunk"]
    n = {"chunk-1": ch - 1, "chunk": ch, "chunk+1": ch + 1, "20*chunk+7": 20 * ch + 7}[reps]
    entries = 4 * (1 << k["bucket_shift"]) + 5
    t = 2 * (1 << k["bucket_shift"]) + 3 * (1 << k["quarter_shift"]) + 12345
    log = np.full(n, t, dtype=np.uint32)

    def prep(f):
        f.set_bits([t], preset)
        if preset:
            f.table[t] = 1000

    _run(entries, log, seed=11, prep=prep)


@pytest.mark.gpu
def test_hot_split_bucket_next_to_cold_buckets():
    """~40 apply items on one bucket (a few hundred tuples, random preset bits) among buckets of one item each"""
    k = K()
    bs, ch = 1 << k["bucket_shift"], k["chunk"]
    entries = 6 * bs - 3
    rng = np.random.default_rng(5)
    hot_tuples = 3 * bs + rng.choice(bs, 300, replace=False)
    hot = rng.choice(hot_tuples, 40 * ch - 1000)
    cold = np.concatenate([b * bs + rng.integers(0, bs if b < 5 else bs - 3, 3000 + 17 * b) for b in (0, 1, 2, 4, 5)])
    log = np.concatenate([hot, cold, np.full(999, k["none"])]).astype(np.uint32)
    rng.shuffle(log)
    for sg, ag in [(0, 0), (0, 7)]:
        f = Fold(entries, log.size, seed=5)
        f.set_bits(hot_tuples, False)
        f.set_bits(hot_tuples[::3], True)
        f.fold(log, sg, ag)


@pytest.mark.gpu
def test_every_tile_touches_every_bucket():
    k = K()
    bs, tile = 1 << k["bucket_shift"], k["tile"]
    nb = 160
    entries = nb * bs - 5
    rng = np.random.default_rng(6)
    n = 4 * tile + 100
    b = np.arange(n) % nb
    off = rng.integers(0, bs - 5, n)
    log = (b * bs + off).astype(np.uint32)
    log[::97] = k["none"]
    _run(entries, log, seed=6)


@pytest.mark.gpu
def test_most_buckets():
    """nb = kFoldMaxBuckets: the largest table the fold takes (a 17 GB table of counts)"""
    import torch
    k = K()
    bs, qs = 1 << k["bucket_shift"], 1 << k["quarter_shift"]
    entries = (k["max_buckets"] - 1) * bs + 33
    need = entries * 4 * 3 + entries // 4 + (2 << 30)  # table, its expected copy, a transient copy; bit maps
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %.1f GB of free device memory, has %.1f" % (need / 1e9, free / 1e9))
    rng = np.random.default_rng(8)
    edges = np.concatenate([np.arange(1, entries // qs + 1) * qs + d for d in (-1, 0)])
    edges = edges[edges < entries]
    log = np.concatenate([edges, [0, entries - 1, entries - 1], rng.integers(0, entries, 1 << 20),
                          np.full(5, k["none"])]).astype(np.uint32)
    rng.shuffle(log)
    f = Fold(entries, log.size, seed=8)
    assert f.nb == k["max_buckets"]
    f.set_bits([entries - 1], False)
    f.fold(log)
    del f
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_largest_chunk_zipf():
    """a 2^27-entry log (BC_COUNT_LOG_CHUNK's default) with Zipf-distributed tuples: hot buckets split many ways"""
    k = K()
    entries = 600_000_001
    rng = np.random.default_rng(9)
    rank = rng.zipf(1.2, 1 << 27)
    log = ((rank.astype(np.uint64) * np.uint64(2_654_435_761)) % np.uint64(entries)).astype(np.uint32)
    log[rng.integers(0, log.size, 1000)] = k["none"]
    f = Fold(entries, log.size, seed=9)
    f.fold(log)


@pytest.mark.gpu
@pytest.mark.parametrize("grids", [(0, 0), (1, 1)])
def test_three_folds_on_the_same_buffers(grids):
    """meta and grouped reused as the engine reuses them; each fold is checked against the state the last one left"""
    k = K()
    bs = 1 << k["bucket_shift"]
    entries = 3 * bs + 999
    rng = np.random.default_rng(10)
    f = Fold(entries, 600_000, seed=10)
    for n, hot in ((600_000, 50), (12_345, 5), (400_000, 2000)):
        tup = rng.integers(0, entries, hot)
        log = np.concatenate([rng.choice(tup, n // 2), rng.integers(0, entries, n - n // 2)]).astype(np.uint32)
        f.fold(log, *grids)


@pytest.mark.gpu
def test_without_a_dirty_map():
    k = K()
    bs = 1 << k["bucket_shift"]
    entries = 2 * bs + 64
    rng = np.random.default_rng(12)
    log = np.concatenate([rng.integers(0, entries, 300_000), np.full(300_000, bs + 7)]).astype(np.uint32)
    _run(entries, log, seed=12, dirty=False)
