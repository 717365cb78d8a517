"""The run reduction (csrc/bc_reduce.h) on its own: tests/reduce/reduce_harness.hip calls bc::reduce_runs_launch on
buffers built here, and run keys, run sums and the number of runs are compared with numpy.unique + numpy.add.reduceat
over the values as unsigned 64-bit numbers.  Canary words after every buffer must stay, and so must whatever lies in
out_keys beyond the last run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ngs-barcode-count_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "reduce", "reduce_harness.hip")
SO = os.path.join(ROOT, "tests", "reduce", "libreduce_harness.so")
DEPS = [SRC, os.path.join(CSRC, "bc_reduce.h")]
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
CANARY = 0x5A5A5A5A5A5A5A5A
CANARY_WORDS = 64
POISON = 0xEEEEEEEEEEEEEEEE
HIP_INVALID_VALUE = 1


def compile_harness(so):
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", so, SRC])


def build(so=SO):
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        compile_harness(so)
    return so


def load(so=SO):
    import torch  # noqa: F401  (first: one HIP runtime in the process, as _lib.load() arranges)
    L = C.CDLL(build(so) if so == SO else so)
    L.reduce_harness_constants.restype = None
    L.reduce_harness_constants.argtypes = [C.POINTER(C.c_uint64)]
    L.reduce_harness_scratch_words.restype = C.c_uint64
    L.reduce_harness_scratch_words.argtypes = [C.c_uint64]
    L.reduce_harness_run.restype = C.c_int
    L.reduce_harness_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def constants(L):
    out = (C.c_uint64 * 4)()
    L.reduce_harness_constants(out)
    return dict(zip(("tile", "waves", "chunks"), list(out)[:3]))


def test_reduce_harness_cross_compiles(tmp_path):
    """no GPU needed: the harness builds against the shipped header, reports the tile the shapes below come from, and a
    size the counters cannot hold is refused before anything is touched"""
    so = str(tmp_path / "libreduce_harness.so")
    compile_harness(so)
    L = load(so)
    k = constants(L)
    assert k["tile"] == 2048 == k["waves"] * k["chunks"] * 64
    assert L.reduce_harness_scratch_words(k["tile"] + 1) == 2 and L.reduce_harness_scratch_words(0) == 1
    for n in (2 ** 32 - k["tile"] - 1, 2 ** 32, 2 ** 40):
        assert L.reduce_harness_run(None, None, n, None, None, None, None) == HIP_INVALID_VALUE


# ---------------------------------------------------------------------------------------------------------------------
# GPU cases

_K = {}


def K():
    if not _K:
        _K["lib"] = load()
        _K.update(constants(_K["lib"]))
    return _K


def run_reduce(keys, vals):
    """reduces the sorted (keys u64, vals u32) on the device, checks the canaries -> (run keys, run sums)"""
    import torch
    k = K()
    n = len(keys)
    canary64 = np.full(CANARY_WORDS, CANARY, dtype=np.uint64)
    canary32 = canary64.view(np.uint32)[:CANARY_WORDS]

    def dev(a, canary):
        return torch.from_numpy(np.concatenate([a, canary]).view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()

    dk, dv = dev(keys.astype(np.uint64), canary64), dev(vals.astype(np.uint32), canary32)
    ok = dev(np.full(n, POISON, dtype=np.uint64), canary64)
    os_ = dev(np.full(n, POISON, dtype=np.uint64), canary64)  # (the launch zeroes it: out_sums need not come zeroed)
    nr = dev(np.full(1, 0xEEEEEEEE, dtype=np.uint32), canary32)
    sc = dev(np.full(int(k["lib"].reduce_harness_scratch_words(n)), 0xEEEEEEEE, dtype=np.uint32), canary32)
    rc = k["lib"].reduce_harness_run(dk.data_ptr(), dv.data_ptr(), n, ok.data_ptr(), os_.data_ptr(), nr.data_ptr(), sc.data_ptr())
    assert rc == 0, "hipError_t %d" % rc
    gk, gs = ok.cpu().numpy().view(np.uint64), os_.cpu().numpy().view(np.uint64)
    gn = nr.cpu().numpy().view(np.uint32)
    for name, t, cn in (("keys", dk.cpu().numpy().view(np.uint64), canary64), ("vals", dv.cpu().numpy().view(np.uint32), canary32),
                        ("out_keys", gk, canary64), ("out_sums", gs, canary64), ("n_runs", gn, canary32),
                        ("scratch", sc.cpu().numpy().view(np.uint32), canary32)):
        assert np.array_equal(t[-CANARY_WORDS:], cn), name + ": canary overwritten"
    assert np.array_equal(dk.cpu().numpy().view(np.uint64)[:n], keys) and np.array_equal(dv.cpu().numpy().view(np.uint32)[:n], vals)
    runs = int(gn[0])
    assert runs <= n
    assert (gk[runs:n] == np.uint64(POISON)).all(), "out_keys written beyond the last run"
    if n:
        assert not gs[runs:n].any(), "out_sums not zero beyond the last run"
    return gk[:runs], gs[:runs]


def check(keys, vals=None, seed=0):
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    assert n < 2 or (keys[1:] >= keys[:-1]).all()  # sorted as unsigned numbers
    vals = np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) if vals is None \
        else np.asarray(vals, dtype=np.uint32)
    uk, first = np.unique(keys, return_index=True)
    sums = np.add.reduceat(vals.astype(np.uint64), first) if n else np.zeros(0, dtype=np.uint64)
    gk, gs = run_reduce(keys, vals)
    assert len(gk) == len(uk), (len(gk), len(uk))
    assert np.array_equal(gk, uk), "keys differ at %s" % np.flatnonzero(gk != uk)[:8]
    assert np.array_equal(gs, sums), "sums differ at %s" % np.flatnonzero(gs != sums)[:8]
    return len(uk)


def keys_of_runs(lengths, start=5, step=3):
    """sorted keys whose runs have the given lengths"""
    lengths = np.asarray(lengths, dtype=np.int64)
    return np.repeat(np.uint64(start) + np.arange(len(lengths), dtype=np.uint64) * np.uint64(step), lengths)


SIZES = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049]


@pytest.mark.gpu
def test_every_size():
    assert K()["tile"] == 2048
    rng = np.random.default_rng(1)
    for n in SIZES:
        keys = np.sort(rng.integers(0, max(1, n // 3) + 1, size=n, dtype=np.uint64))  # runs of about 3
        check(keys, seed=n)
        check(np.full(n, 7, dtype=np.uint64), seed=n + 1)  # one run
        assert check(np.arange(n, dtype=np.uint64) * np.uint64(11), seed=n + 2) == n  # all distinct


@pytest.mark.gpu
def test_small_inputs():
    """n = 0 and n = 1 run no kernel: the result is there all the same"""
    gk, gs = run_reduce(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    assert len(gk) == 0 and len(gs) == 0
    gk, gs = run_reduce(np.array([2 ** 64 - 1], dtype=np.uint64), np.array([2 ** 32 - 1], dtype=np.uint32))
    assert list(gk) == [2 ** 64 - 1] and list(gs) == [2 ** 32 - 1]


@pytest.mark.gpu
def test_all_keys_distinct():
    n = 3 * 2048 + 100
    keys = np.cumsum(np.random.default_rng(2).integers(1, 1 << 40, size=n, dtype=np.uint64), dtype=np.uint64)
    assert check(keys) == n


@pytest.mark.gpu
def test_one_run_across_wavefronts_tiles_and_workgroups():
    n = 5 * 2048 + 17
    assert check(np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)) == 1
    assert check(np.full(n, 3, dtype=np.uint64), vals=np.ones(n, dtype=np.uint32)) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("edge", [64, 512, 2048], ids=["chunk", "wavefront", "tile"])
def test_runs_at_the_edges(edge):
    """runs that end exactly on an edge, runs that begin one before it, and runs that begin on it"""
    for first in (edge, edge - 1, edge + 1):
        lengths = [first, 1, edge - 1, edge, 1, 2 * edge - 1, 3, edge + 1, edge - 2, 5]
        check(keys_of_runs(lengths), seed=first)
    # every run ends on the edge; every run begins one before it
    check(keys_of_runs([edge] * 6), seed=3)
    check(keys_of_runs([edge - 1] + [edge] * 5 + [1]), seed=4)


@pytest.mark.gpu
def test_alternating_run_lengths():
    lengths = [1, 300] * 40
    assert check(keys_of_runs(lengths)) == 80
    assert check(keys_of_runs(lengths[::-1])) == 80


@pytest.mark.gpu
def test_bit_63_is_a_key_bit():
    lengths = [70, 1, 2048, 3, 500]
    low = keys_of_runs(lengths, start=2 ** 63 - 8, step=3)  # crosses 2^63 between two runs
    assert (low >> np.uint64(63)).any() and not (low >> np.uint64(63)).all()
    assert check(low) == len(lengths)
    # keys that differ in bit 63 alone are different runs
    keys = np.array([5] * 100 + [5 + 2 ** 63] * 100, dtype=np.uint64)
    assert check(keys) == 2
    assert check(np.full(4097, 2 ** 64 - 1, dtype=np.uint64)) == 1


@pytest.mark.gpu
def test_sums_pass_two_to_the_32():
    n = 70_000
    keys = np.concatenate([np.full(10, 1, dtype=np.uint64), np.full(n, 2, dtype=np.uint64), np.full(10, 9, dtype=np.uint64)])
    vals = np.full(len(keys), 2 ** 32 - 1, dtype=np.uint32)
    gk, gs = run_reduce(keys, vals)
    assert list(gk) == [1, 2, 9] and list(gs) == [10 * (2 ** 32 - 1), n * (2 ** 32 - 1), 10 * (2 ** 32 - 1)]
    assert int(gs[1]) > 2 ** 48
    check(keys, vals)


@pytest.mark.gpu
def test_zipf_like_run_lengths():
    rng = np.random.default_rng(7)
    lengths = np.minimum(rng.zipf(1.7, size=60_000), 60_000)
    lengths = lengths[np.cumsum(lengths) <= 200_000]
    assert lengths.sum() > 190_000 and lengths.max() > 4 * 2048 and (lengths == 1).sum() > 1000
    keys = keys_of_runs(lengths, start=2 ** 62, step=2 ** 40 + 1)
    assert check(keys, seed=8) == len(lengths)
