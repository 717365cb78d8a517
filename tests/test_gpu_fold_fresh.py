"""The count-log fold's fresh mode (csrc/bc_fold.h): the first fold after a reset takes the bit map as all zero without
anyone having written the zeros, and leaves every word of it defined.  tests/fold/fold_fresh_harness.hip runs
bc::fold_launch(..., fresh) on a bit map filled with 0xFF words; map, table, dirty map, grouped log and meta buffer are
then checked word by word by the reference of test_gpu_fold.py, computed from an all-zero map: for each tuple with
c > 0 entries the bit set and table + c - 1, every other word of the map zero, nothing else changed (canaries included).
The harness with fresh = 0 is the ordinary fold."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_fold as tg

SRC = os.path.join(tg.ROOT, "tests", "fold", "fold_fresh_harness.hip")
SO = os.path.join(tg.ROOT, "tests", "fold", "libfold_fresh_harness.so")
DEPS = [SRC] + tg.DEPS[1:]


def _compile(so):
    subprocess.check_call([tg.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I" + tg.CSRC, "-o", so, SRC])


def _bind(so):
    import torch  # noqa: F401  (first: one HIP runtime in the process)
    L = C.CDLL(so)
    L.fold_fresh_harness_run.restype = C.c_int
    L.fold_fresh_harness_run.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int]
    return L


def test_fresh_harness_cross_compiles(tmp_path):
    """no GPU needed: the harness builds against the shipped headers"""
    so = str(tmp_path / "libfold_fresh_harness.so")
    _compile(so)
    assert hasattr(_bind(so), "fold_fresh_harness_run")


_L = {}


def _lib():
    if not _L:
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in DEPS):
            _compile(SO)
        _L["lib"] = _bind(SO)
    return _L["lib"]


class _Through:
    """stands in for the ordinary harness inside Fold.fold: the same call, through the fresh harness"""

    def __init__(self, fold, fresh):
        self.fold, self.fresh = fold, fresh

    def fold_harness_run(self, *args):
        import torch
        if self.fresh:
            self.fold.bits[:self.fold.n_words] = -1  # garbage where the reference saw zeros: the fold may not read it
            torch.cuda.synchronize()
        return _lib().fold_fresh_harness_run(*args, 1 if self.fresh else 0)


class FreshFold(tg.Fold):
    def fold(self, log, scatter_grid=0, apply_grid=0, fresh=True):
        import torch
        k = tg.K()
        if fresh:
            self.bits[:self.n_words] = 0  # the state the reference starts from
            torch.cuda.synchronize()
        real = k["lib"]
        k["lib"] = _Through(self, fresh)
        try:
            super().fold(log, scatter_grid, apply_grid)
        finally:
            k["lib"] = real


def _run(entries, log, seed, dirty=True, grids=None):
    for sg, ag in grids or tg._grids(log.size):
        FreshFold(entries, log.size, seed, dirty=dirty).fold(log, sg, ag)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 16384, 50_001])
def test_no_entries(n):
    """every bucket is empty: the whole map is zeroed by bc_fold_zero_unowned"""
    k = tg.K()
    _run(2 * (1 << k["bucket_shift"]) + 77, np.full(n, k["none"], dtype=np.uint32), seed=7)


@pytest.mark.gpu
@pytest.mark.parametrize("entries_off", [0, -5, 1000])
def test_one_bucket(entries_off):
    """a table of one bucket (whole, ragged, and a second bucket that stays empty), repeats among the entries"""
    k = tg.K()
    bs = 1 << k["bucket_shift"]
    entries = bs + entries_off
    rng = np.random.default_rng(21)
    log = rng.integers(0, min(entries, bs), 200_000).astype(np.uint32)
    log[::5] = log[1::5][:log[::5].size]  # repeats
    log[::101] = k["none"]
    _run(entries, log, seed=21)


@pytest.mark.gpu
def test_empty_buckets_between_full_ones():
    k = tg.K()
    bs = 1 << k["bucket_shift"]
    entries = 9 * bs - 3
    rng = np.random.default_rng(22)
    full = (0, 3, 4, 8)  # 1, 2, 5, 6, 7 stay empty; the last bucket is ragged
    log = np.concatenate([b * bs + rng.integers(0, bs - 3, 40_000 + 11 * b) for b in full]).astype(np.uint32)
    log = np.concatenate([log, log[:5000], np.full(77, k["none"], dtype=np.uint32)])
    rng.shuffle(log)
    _run(entries, log, seed=22)
    _run(entries, log, seed=23, dirty=False, grids=[(0, 3)])


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_a_bucket_of_exactly_one_chunk_and_one_more(extra):
    """kFoldChunk entries: one item, which owns the bucket and never reads it; one more entry: two items, which meet on
    zeros that bc_fold_zero_unowned wrote"""
    k = tg.K()
    bs, ch = 1 << k["bucket_shift"], k["chunk"]
    entries = 4 * bs + 5
    rng = np.random.default_rng(24 + extra)
    hot = 2 * bs + rng.integers(0, bs, ch + extra)
    hot[:1000] = hot[1000:2000]  # repeats inside the bucket
    cold = np.concatenate([b * bs + rng.integers(0, bs if b < 4 else 5, 3000) for b in (0, 4)])  # bucket 1, 3: empty
    log = np.concatenate([hot, cold]).astype(np.uint32)
    rng.shuffle(log)
    for sg, ag in [(0, 0), (1, 1), (0, 2)]:
        FreshFold(entries, log.size, seed=24).fold(log, sg, ag)


@pytest.mark.gpu
def test_one_tuple_many_chunks():
    """a bucket split twenty ways over one tuple: exactly one item finds the bit clear"""
    k = tg.K()
    bs, ch = 1 << k["bucket_shift"], k["chunk"]
    t = bs + 3 * (1 << k["quarter_shift"]) + 12345
    _run(3 * bs + 9, np.full(20 * ch + 7, t, dtype=np.uint32), seed=26)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [0, 1, 31, 32 + 5, 64 + 17, 96 + 9, 4 * 37 * 32 + 3])
@pytest.mark.parametrize("last", ["owned", "empty", "split"])
def test_ragged_last_quarter(r, last):
    """the table ends r tuples into a quarter (n_words % 4 = every residue): the last bucket with one item, with none,
    and split; nothing past n_words may be written and the last word's bits past the table's end are zero"""
    k = tg.K()
    bs, qs, ch = 1 << k["bucket_shift"], 1 << k["quarter_shift"], k["chunk"]
    entries = 2 * bs + qs + r + (1 if r == 0 else 0)
    tail = entries - 2 * bs
    rng = np.random.default_rng(300 + r)
    parts = [rng.integers(0, bs, 5000), np.array([0, bs - 1, entries - 1 if last != "empty" else 0])]
    if last != "empty":
        parts.append(2 * bs + rng.integers(0, tail, 4000 if last == "owned" else ch + 4000))
    log = np.concatenate(parts).astype(np.uint32)
    rng.shuffle(log)
    _run(entries, log, seed=r)


@pytest.mark.gpu
def test_three_folds_first_one_fresh():
    """as the engine folds a submit of several chunks after a reset: the first fresh, the others onto what it left"""
    k = tg.K()
    bs = 1 << k["bucket_shift"]
    entries = 3 * bs + 999
    rng = np.random.default_rng(30)
    f = FreshFold(entries, 600_000, seed=30)
    for j, (n, hot) in enumerate(((600_000, 50), (12_345, 5), (400_000, 2000))):
        tup = rng.integers(0, entries, hot)
        log = np.concatenate([rng.choice(tup, n // 2), rng.integers(0, entries, n - n // 2)]).astype(np.uint32)
        f.fold(log, fresh=j == 0)


@pytest.mark.gpu
def test_the_ordinary_fold_through_this_harness():
    """fresh = 0: random bits already set, as in test_gpu_fold.py"""
    k = tg.K()
    bs = 1 << k["bucket_shift"]
    entries = 2 * bs + 64
    rng = np.random.default_rng(31)
    log = np.concatenate([rng.integers(0, entries, 300_000), np.full(300_000, bs + 7)]).astype(np.uint32)
    FreshFold(entries, log.size, seed=31).fold(log, fresh=False)
