"""The order of keys several u64 wide (csrc/bc_sort.h, bc::sort_words_launch) on its own: tests/sort/sort_words_harness.hip
calls it on buffers built here, and the permutation is compared with numpy.lexsort over the words as unsigned 64-bit
numbers (word K-1 the most significant), which is stable as the sort must be: keys equal in every word keep their input
order.  Canary words after every buffer must stay, and the keys themselves are only read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "sort", "sort_words_harness.hip")
SO = os.path.join(ROOT, "tests", "sort", "libsort_words_harness.so")
DEPS = [SRC, os.path.join(CSRC, "bc_sort.h")]
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
CANARY = 0x5A5A5A5A5A5A5A5A
CANARY_WORDS = 64
TILE = 2048
SIZES = [0, 1, 63, TILE, TILE + 1, 5 * TILE + 17]


def compile_to(so):
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", so, SRC])


def load(so=SO):
    import torch  # noqa: F401  (first: one HIP runtime in the process, as _lib.load() arranges)
    if so == SO and (not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS)):
        compile_to(so)
    L = C.CDLL(so)
    L.sort_words_harness_tile.restype = C.c_uint64
    L.sort_words_harness_scratch_words.restype = C.c_uint64
    L.sort_words_harness_scratch_words.argtypes = [C.c_uint64]
    L.sort_words_harness_run.restype = C.c_int
    L.sort_words_harness_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 5 + [C.POINTER(C.c_uint32)]
    return L


def test_sort_words_harness_cross_compiles(tmp_path):
    """no GPU needed: the harness builds against the shipped header, and the sizes below are cut at its tile"""
    so = str(tmp_path / "libsort_words_harness.so")
    compile_to(so)
    L = load(so)
    assert L.sort_words_harness_tile() == TILE
    assert L.sort_words_harness_scratch_words(TILE + 1) == 2 * 256 + 8 * 256


_L = []


def lib():
    if not _L:
        _L.append(load())
    return _L[0]


def run_sort(words):
    """words: (K, n) u64 -> (perm, live passes); checks the canaries and that the keys were left alone"""
    import torch
    L = lib()
    K, n = words.shape
    canary64 = np.full(CANARY_WORDS, CANARY, dtype=np.uint64)
    canary32 = canary64.view(np.uint32)[:CANARY_WORDS]

    def dev(a, canary):
        return torch.from_numpy(np.concatenate([a, canary]).view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()

    dw = dev(np.ascontiguousarray(words, dtype=np.uint64).reshape(-1), canary64)
    perm = dev(np.full(n, 0xEEEEEEEE, dtype=np.uint32), canary32)
    col, col2 = (dev(np.full(n, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64), canary64) for _ in range(2))
    perm2 = dev(np.full(n, 0xEEEEEEEE, dtype=np.uint32), canary32)
    sc = dev(np.zeros(int(L.sort_words_harness_scratch_words(n)), dtype=np.uint32), canary32)
    live = C.c_uint32(99)
    rc = L.sort_words_harness_run(dw.data_ptr(), K, n, perm.data_ptr(), col.data_ptr(), col2.data_ptr(), perm2.data_ptr(),
                                  sc.data_ptr(), C.byref(live))
    assert rc == 0, "hipError_t %d" % rc
    back = dw.cpu().numpy().view(np.uint64)
    assert np.array_equal(back[:K * n].reshape(K, n), words), "the keys were written"
    for name, t, cn in (("words", back, canary64), ("perm", perm.cpu().numpy().view(np.uint32), canary32),
                        ("col", col.cpu().numpy().view(np.uint64), canary64), ("col_tmp", col2.cpu().numpy().view(np.uint64), canary64),
                        ("perm_tmp", perm2.cpu().numpy().view(np.uint32), canary32),
                        ("scratch", sc.cpu().numpy().view(np.uint32), canary32)):
        assert np.array_equal(t[-CANARY_WORDS:], cn), name + ": canary overwritten"
    return perm.cpu().numpy().view(np.uint32)[:n], live.value


def check(words):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    K, n = words.shape
    want = np.lexsort(tuple(words[w] for w in range(K))) if n else np.zeros(0, dtype=np.int64)  # (the last key is primary)
    got, live = run_sort(words)
    assert np.array_equal(got.astype(np.int64), want), "order differs at %s" % np.flatnonzero(got != want)[:8]
    return live


def random_words(K, n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 63, size=(K, n), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(K, n), dtype=np.uint64)
    if n > 2:  # few distinct values in the upper words, so that the lower ones decide often; bit 63 set in some
        for k in range(1, K):
            w[k] = w[k, rng.integers(0, 3, size=n)]
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 3, 7])
def test_every_size(K):
    for i, n in enumerate(SIZES):
        w = random_words(K, n, 100 * K + i)
        if n > 2:
            top = w[K - 1] >> np.uint64(63)
            assert K == 1 or len(np.unique(w[K - 1])) <= 3
            assert top.any() or K > 1  # sorted as unsigned numbers
        live = check(w)
        if n < 2:
            assert live == 0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 3, 7])
def test_keys_that_differ_in_one_word_only(K):
    n = TILE + 1
    rng = np.random.default_rng(K)
    base = rng.integers(0, 1 << 62, size=(K, 1), dtype=np.uint64)
    for only in (0, K - 1):  # the least significant word alone decides; then the most significant alone
        w = np.repeat(base, n, axis=1)
        w[only] = rng.integers(0, 1 << 62, size=n, dtype=np.uint64) * np.uint64(4) + np.uint64(1)
        live = check(w)
        assert 1 <= live <= 8  # every other word is one skipped sweep


@pytest.mark.gpu
def test_constant_middle_word():
    n = 5 * TILE + 17
    w = random_words(3, n, 9)
    w[1] = np.uint64(0x0123456789ABCDEF)
    check(w)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
def test_all_keys_equal_is_the_identity(K):
    n = 2 * TILE + 3
    w = np.full((K, n), 0xFEDCBA9876543210, dtype=np.uint64)
    got, live = run_sort(w)
    assert live == 0 and np.array_equal(got, np.arange(n, dtype=np.uint32))
