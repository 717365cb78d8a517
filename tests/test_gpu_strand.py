"""The strand setting on the engine (bc_plan_set_strand: forward | reverse | both) against the oracle composition of
strand_cases.expected(): every read's traced outcome and index, the counters, the rows and strand_reads()."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import parity
import readgen
import strand_cases as sc
import wide_lane_cases as wlc

pytestmark = pytest.mark.gpu

MODES = ["forward", "reverse", "both"]
MATRIX = ["del_mismatch_quality", "crispr", "fmtn", "refs_with_n_and_ragged", "long_gaps"]


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


@pytest.fixture(autouse=True)
def _own_jit_cache(monkeypatch, tmp_path_factory):
    monkeypatch.setenv("BC_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit_cache"))


@pytest.fixture
def kernel(request, monkeypatch):
    monkeypatch.setenv("BC_JIT", "force" if request.param == "specialised" else "0")
    return request.param


@pytest.fixture
def generic(monkeypatch):
    monkeypatch.setenv("BC_JIT", "0")


def make_plan(case, mode=None):
    """mode None: a plan nobody has given a strand"""
    p = _pkg().Plan(case["scheme"])
    for s, i in (case.get("samples") or {}).items():
        p.add_sample(s, i)
    for bi, refs in enumerate(case.get("counted") or []):
        for r in refs:
            p.add_counted(bi, r, r)
    kw = case.get("kwargs", {})
    p.set_max_errors(kw.get("max_sample"), kw.get("max_barcode"), kw.get("max_constant"))
    p.set_min_quality(kw.get("min_quality", 0.0))
    if mode is not None:
        p.set_strand(mode)
    return p


def last_key(eng):
    key, lds, grid, resident = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    f = eng._lib.bc_internal_last_launch
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    f.restype = C.c_int
    assert f(eng._e, C.byref(key), C.byref(lds), C.byref(grid), C.byref(resident)) == 0
    return key.value


def submit(eng, reads, use_lens=True, how="device", trace=True, stride=None, qlens=None):
    """one submit of (seq, qual) strings; -> (outcomes, indexes) of the trace, or (None, None)"""
    import torch
    seq, qual, lens = readgen.to_arrays(reads, stride)
    n, stride = seq.shape
    if not use_lens:
        assert (lens == stride).all()
    outc = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    eng.trace(*((outc.data_ptr(), idx.data_ptr()) if trace else (None, None)))
    if how == "host":
        eng.submit_host(seq, qual, stride, stride, lens if use_lens else None)
    else:
        dseq, dqual = torch.from_numpy(seq.reshape(-1)).cuda(), torch.from_numpy(qual.reshape(-1)).cuda()
        dlens = torch.from_numpy(lens.view(np.int16)).cuda()
        if qlens is not None:
            dq = torch.from_numpy(np.asarray(qlens, dtype=np.uint16).view(np.int16)).cuda()
            eng.submit_device_q(dseq.data_ptr(), dqual.data_ptr(), n, stride, dlens.data_ptr(), dq.data_ptr())
        else:
            eng.submit_device(dseq.data_ptr(), dqual.data_ptr(), n, stride, stride, dlens.data_ptr() if use_lens else None)
    eng.sync()
    eng.trace(None, None)
    return (outc.cpu().numpy(), idx.cpu().numpy().view(np.uint64)) if trace else (None, None)


@functools.lru_cache(maxsize=None)
def mixed_case(name, use_lens, n=3000):
    c = cases.build_case(name, seed=11 + use_lens, n=n)
    if not use_lens:
        c = sc.fixed_length(c)
    return sc.mix(c, 11 + use_lens)


@functools.lru_cache(maxsize=None)
def expected(name, use_lens, mode):
    return sc.expected(mixed_case(name, use_lens), mode)


@functools.lru_cache(maxsize=None)
def census(name, use_lens):
    return sc.orientation_census(mixed_case(name, use_lens))


def assert_not_vacuous(name, use_lens):
    """From the oracle's own verdicts on every read as it stands and reversed.  A read "matches" an orientation here when
    it gets past the constant region in it -- the event `both` decides on: at least a quarter of the reads do as they
    stand, a quarter only reversed, one in neither.  (Counted by final outcome BC_MATCHED instead, no input whose scheme
    matches well under half of its reads -- refs_with_n_and_ragged: 41 % -- could hold a quarter in each orientation; an
    eighth each way ending BC_MATCHED is asserted on top, so that the rows depend on both passes.)"""
    k, n = census(name, use_lens), len(mixed_case(name, use_lens)["reads"])
    assert k["forward"] * 4 >= n and k["reverse_only"] * 4 >= n and k["neither"] >= 1, k
    assert k["matched_forward"] * 8 >= n and k["matched_reverse_only"] * 8 >= n, k
    if name == "long_gaps":
        assert k["either_way"] >= 100, k  # forward wins: the order is observable here


@pytest.mark.parametrize("name", MATRIX)
@pytest.mark.parametrize("use_lens", [False, True], ids=["fixed", "ragged"])
def test_inputs_are_not_vacuous(name, use_lens):
    assert_not_vacuous(name, use_lens)


def check_kernel(eng, kernel):
    name = eng.kernel_name()
    nw, nww = (int(v) for v in name[name.index("<") + 1:-1].split(","))
    if kernel == "specialised" and nw <= 8 and nww <= 4:
        assert name.startswith("bc_jit_match_count"), name
    else:
        assert name.startswith("match_count_kernel"), name


@pytest.mark.parametrize("name", MATRIX)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("use_lens", [False, True], ids=["fixed", "ragged"])
@pytest.mark.parametrize("kernel", ["generic", "specialised"], indirect=True)
def test_engine_vs_composition(name, mode, use_lens, kernel):
    c, exp = mixed_case(name, use_lens), expected(name, use_lens, mode)
    plan = make_plan(c, mode)
    eng = _pkg().Engine(plan, device=0)
    outc, idx = submit(eng, c["reads"], use_lens)
    sc.check_engine(c, plan, eng, exp, outc, idx)
    check_kernel(eng, kernel)
    eng.close()


# ---- chunk and wave edges: BC_STRAND_CHUNK=256 ----

def _sub(case, reads):
    c = dict(case)
    c["reads"] = list(reads)
    return c


@pytest.mark.parametrize("how", ["device", "host"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3000])
def test_chunks_of_256(n, how, generic, monkeypatch):
    monkeypatch.setenv("BC_STRAND_CHUNK", "256")
    c = _sub(mixed_case("del_mismatch_quality", True), mixed_case("del_mismatch_quality", True)["reads"][:n])
    for mode in ("both", "reverse"):
        plan = make_plan(c, mode)
        eng = _pkg().Engine(plan, device=0)
        outc, idx = submit(eng, c["reads"], how=how)
        sc.check_engine(c, plan, eng, sc.expected(c, mode), outc, idx)
        eng.close()


@pytest.mark.parametrize("how", ["device", "host"])
@pytest.mark.parametrize("which", ["none_retried", "all_retried"])
@pytest.mark.parametrize("chunk", ["256", None])
def test_batches_of_one_kind(which, how, chunk, generic, monkeypatch):
    """a batch in which no read is retried (m = 0 in every chunk), and one in which every read is"""
    if chunk:
        monkeypatch.setenv("BC_STRAND_CHUNK", chunk)
    full = mixed_case("crispr", True)
    probe = parity.oracle_for(full)
    const = [probe.process(s, q) == "constant_region" for s, q in full["reads"]]
    c = _sub(full, [r for r, k in zip(full["reads"], const) if k == (which == "all_retried")][:700])
    assert len(c["reads"]) == 700
    plan = make_plan(c, "both")
    eng = _pkg().Engine(plan, device=0)
    outc, idx = submit(eng, c["reads"], how=how)
    exp = sc.expected(c, "both")
    assert exp["retried"] == (700 if which == "all_retried" else 0)
    sc.check_engine(c, plan, eng, exp, outc, idx)
    eng.close()


def test_untraced_submits_count_the_same(generic, monkeypatch):
    """no caller's trace: pass 1 records into the engine's scratch, pass 2 runs untraced"""
    monkeypatch.setenv("BC_STRAND_CHUNK", "512")
    c = mixed_case("fmtn", True)
    for mode in ("both", "reverse"):
        plan = make_plan(c, mode)
        eng = _pkg().Engine(plan, device=0)
        submit(eng, c["reads"], trace=False)
        sc.check_engine(c, plan, eng, expected("fmtn", True, mode))
        eng.close()


# ---- counting modes ----

@pytest.mark.parametrize("count_log", ["1", "0"])
@pytest.mark.parametrize("kernel", ["generic", "specialised"], indirect=True)
def test_counting_modes(count_log, kernel, monkeypatch):
    monkeypatch.setenv("BC_BITMAP_MIN_ENTRIES", "1")
    monkeypatch.setenv("BC_COUNT_LOG", count_log)
    c, exp = mixed_case("del_mismatch_quality", False), expected("del_mismatch_quality", False, "both")
    plan = make_plan(c, "both")
    eng = _pkg().Engine(plan, device=0)
    outc, idx = submit(eng, c["reads"], use_lens=False)
    sc.check_engine(c, plan, eng, exp, outc, idx)
    # one chunk, both passes: a fold each when the log is on
    assert eng.count_log_folds() == (2 if count_log == "1" else 0)
    check_kernel(eng, kernel)
    eng.close()


# ---- one case per plan kind, in `both` ----

def test_random_barcode_molecules_seen_both_ways(generic):
    """del_random mixed, then every molecule once as it stands and once reversed: one Results, so the second sighting is a
    duplicate.  Which of two equal keys is the duplicate depends on scheduling: per read matched / duplicate are one class"""
    base = cases.build_case("del_random", seed=11, n=1500)
    c = _sub(base, sc.mix(base, 3)["reads"] + [sc.rc(s, q) for s, q in base["reads"]])
    exp = sc.expected(c, "both")
    assert exp["counters"]["duplicates"] >= exp["counters"]["matched"] > 100
    plan = make_plan(c, "both")
    eng = _pkg().Engine(plan, device=0)
    outc, idx = submit(eng, c["reads"])
    sc.check_engine(c, plan, eng, exp, outc, idx, fold_duplicates=True)
    assert eng.key_count() == exp["counters"]["matched"]
    eng.close()


def test_raw_key_plan(generic):
    c = sc.mix(cases.build_case("raw_counted", seed=11, n=3000), 5)
    plan = make_plan(c, "both")
    assert plan.mode == "sparse"
    eng = _pkg().Engine(plan, device=0)
    outc, idx = submit(eng, c["reads"])
    exp = sc.expected(c, "both")
    assert exp["matched_reverse"] > 300
    sc.check_engine(c, plan, eng, exp, outc, idx)
    eng.close()


@pytest.mark.parametrize("wide_lane", ["0", "1"])
def test_wide_key_plan(wide_lane, generic, monkeypatch):
    monkeypatch.setenv("BC_WIDE_LANE", wide_lane)
    w, pools, reads = wlc.pools_and_reads("raw_22_21", 2000, 7)
    samples, counted = wlc.sets_of(w, pools)
    c = sc.mix(dict(scheme=w["scheme"], samples=samples, counted=counted, kwargs={}, reads=[(r, "I" * len(r)) for r in reads]), 9)
    plan = make_plan(c, "both")
    eng = _pkg().Engine(plan, device=0)
    outc, _ = submit(eng, c["reads"])
    exp = sc.expected(c, "both")
    assert exp["matched_reverse"] > 300
    sc.check_engine(c, plan, eng, exp)
    assert [int(v) for v in outc] == [parity.CODE[e] for e in exp["outcomes"]]
    assert eng.wide_lane_reads() == (len(reads) + exp["retried"] if wide_lane == "1" else 0)
    eng.close()


def test_batch_of_321_bases_on_the_wave_per_read_kernel(generic):
    base = mixed_case("del_mismatch_quality", True, 1000)
    filler = ("TGCA" * 81)[:221]
    c = _sub(base, [(s + filler, q + "I" * 221) if len(s) == 100 else (s, q) for s, q in base["reads"]])
    for mode in ("both", "reverse"):
        plan = make_plan(c, mode)
        eng = _pkg().Engine(plan, device=0)
        outc, idx = submit(eng, c["reads"], stride=321)
        assert eng.kernel_name() == "long_match_kernel"
        sc.check_engine(c, plan, eng, sc.expected(c, mode), outc, idx)
        eng.close()


def test_short_quality_lines(generic, monkeypatch):
    """bc_engine_submit_device_q: quality lines cut short (and some longer than the sequence line's bases in use); each line
    is reversed over its own length"""
    monkeypatch.setenv("BC_STRAND_CHUNK", "256")
    base = mixed_case("del_mismatch_quality", True, 1500)
    rng = np.random.default_rng(77)
    reads = []
    for s, q in base["reads"]:
        r = rng.random()
        reads.append((s, q[:int(rng.integers(0, len(q) + 1))]) if r < 0.4 else ((s[:int(rng.integers(60, len(s) + 1))], q) if r < 0.6 else (s, q)))
    c = _sub(base, reads)
    qlens = [len(q) for _, q in reads]
    assert any(a < len(s) for a, (s, _) in zip(qlens, reads)) and any(a > len(s) for a, (s, _) in zip(qlens, reads))
    for mode in ("both", "reverse"):
        plan = make_plan(c, mode)
        eng = _pkg().Engine(plan, device=0)
        outc, idx = submit(eng, reads, qlens=qlens)
        exp = sc.expected(c, mode)
        assert exp["counters"]["low_quality"] > 0
        sc.check_engine(c, plan, eng, exp, outc, idx)
        eng.close()


# ---- job sequences ----

def test_two_jobs_on_one_engine(generic, monkeypatch):
    """reset_results keeps the counters and strand_reads going, reset zeroes the counters; strand_reads counts since
    creation either way"""
    monkeypatch.setenv("BC_STRAND_CHUNK", "1024")
    c = mixed_case("crispr", True)
    a, b = _sub(c, c["reads"][:1700]), _sub(c, c["reads"][1700:])
    ea, eb = sc.expected(a, "both"), sc.expected(b, "both")
    plan = make_plan(c, "both")
    eng = _pkg().Engine(plan, device=0)
    submit(eng, a["reads"])
    sc.check_engine(a, plan, eng, ea)
    eng.reset_results()
    submit(eng, b["reads"], trace=False)
    got = eng.counters()
    assert {k: got[k] for k in ea["counters"]} == {k: ea["counters"][k] + eb["counters"][k] for k in ea["counters"]}
    assert got["total_reads"] == 3000 and eng.result_rows() == eb["rows"]
    assert eng.strand_reads() == (ea["retried"] + eb["retried"], ea["matched_reverse"] + eb["matched_reverse"])
    eng.reset()
    outc, idx = submit(eng, a["reads"])
    ea2 = dict(ea, retried=2 * ea["retried"] + eb["retried"], matched_reverse=2 * ea["matched_reverse"] + eb["matched_reverse"])
    sc.check_engine(a, plan, eng, ea2, outc, idx)
    eng.close()


@pytest.mark.parametrize("kernel", ["generic", "specialised"], indirect=True)
def test_forward_engine_is_untouched(kernel):
    """a forward plan's engine reports (0, 0) and launches the kernel key of an engine whose plan was never given a
    strand; the key of a `both` engine under the same trace is that key too (pass 2 launches pass 1's shape)"""
    c = mixed_case("del_mismatch_quality", False)
    keys = {}
    for mode in (None, "forward", "both"):
        plan = make_plan(c, mode)
        if mode is None:
            assert plan.strand == "forward"
        eng = _pkg().Engine(plan, device=0)
        submit(eng, c["reads"], use_lens=False, trace=False)
        keys[mode] = (last_key(eng), eng.kernel_name())
        if mode != "both":
            assert eng.strand_reads() == (0, 0)
            sc.check_engine(c, plan, eng, expected("del_mismatch_quality", False, "forward"))
        eng.close()
    assert keys[None] == keys["forward"] == keys["both"]
    assert (keys[None][0] != 0) == (kernel == "specialised")
