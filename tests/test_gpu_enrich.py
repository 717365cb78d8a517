"""Single and double barcode enrichment on the device (bc_engine_enrich, Engine.enrichment, ResultsEnrichment.fill):
the device's marginal sums against numpy's over the engine's own rows, and, where an oracle exists, the maps against
the reference's string path (pyref_output.Writer.add_single / add_double) over the oracle's rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import parity
import pyref_output
import readgen
from test_gpu_parity import _long_cases, kernel, make_plan, run_device  # noqa: F401  (kernel: the fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def sizes_of(plan):
    return [len(plan.counted(g)) for g in range(plan.barcode_num)]


def marginals(s, b, c, n_samples, sizes):
    """numpy marginal sums of index rows (Engine.rows() form), in Engine.enrichment's form"""
    G = len(sizes)
    singles = [np.zeros((n_samples, n), dtype=np.uint64) for n in sizes]
    for g in range(G):
        np.add.at(singles[g], (s.astype(np.int64), b[:, g].astype(np.int64)), c.astype(np.uint64))
    doubles = {}
    if G >= 3:
        for g in range(G):
            for h in range(g + 1, G):
                a = np.zeros((n_samples, sizes[g], sizes[h]), dtype=np.uint64)
                np.add.at(a, (s.astype(np.int64), b[:, g].astype(np.int64), b[:, h].astype(np.int64)), c.astype(np.uint64))
                doubles[(g, h)] = a
    return singles, doubles


def assert_same(got, exp):
    gs, gd = got
    es, ed = exp
    assert len(gs) == len(es)
    for a, e in zip(gs, es):
        assert a.shape == e.shape and np.array_equal(a, e)
    assert sorted(gd) == sorted(ed)
    for k in ed:
        assert gd[k].shape == ed[k].shape and np.array_equal(gd[k], ed[k]), k


def check_against_rows(eng):
    plan = eng.plan
    got = eng.enrichment()
    s, b, c = eng.rows()
    n_samples = len(plan.samples()) if plan.sample_barcode else 1
    assert_same(got, marginals(s, b, c, n_samples, sizes_of(plan)))
    return got


def string_maps(oracle_rows, plan):
    """the maps the reference builds from the oracle's rows (IDs: make_plan names every sequence by itself)"""
    # the Results keys the reference's writers see (info.rs:698-719): the sample file's, else "barcode" without a sample
    # barcode, and every key a row landed on
    samples = [x for x, _ in plan.samples()]
    keys = samples if samples else ([] if plan.sample_barcode else ["barcode"])
    keys = keys + sorted({r[0] for r in oracle_rows} - set(keys))
    w = pyref_output.Writer({k: {} for k in keys}, {}, [], plan.barcode_num, "p", False, True)
    for k in keys:
        w.single[k], w.double[k] = {}, {}
    for sample, tup, n in oracle_rows:
        w.add_single(sample, tup, n)
        if plan.barcode_num > 2:
            w.add_double(sample, tup, n)
    return w.single, w.double


def check_maps(eng, oracle_rows):
    e = _pkg().ResultsEnrichment().fill(eng)
    single, double = string_maps(oracle_rows, eng.plan)
    assert e.single_hashmap == single
    assert e.double_hashmap == double


def oracle_rows(c):
    o = parity.oracle_for(c)
    for s, q in c["reads"]:
        o.process(s, q)
    return o.rows()


def _random_case_seeds():
    return [seed for seed in range(24) if 2 <= len(cases.random_case(seed, n=10)["counted"] or []) <= 4][:8]


@pytest.mark.parametrize("name", cases.ALL_CASES)
@pytest.mark.parametrize("kernel", ["generic", "specialised"], indirect=True)
def test_enrichment_of_every_case(name, kernel):
    c = cases.build_case(name, seed=13, n=3000)
    plan = make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    if plan.mode != "dense":  # raw captures: keys are sequences, not indices
        with pytest.raises(_pkg().BarcodeCountError) as ex:
            eng.enrichment()
        assert ex.value.code == -2
        eng.close()
        return
    got = check_against_rows(eng)
    discard = (not plan.sample_barcode) and len(plan.samples()) > 0 and not plan.random_barcode
    if plan.barcode_num >= 1 and not discard:
        assert any(a.any() for a in got[0])
    if plan.barcode_num >= 2:  # (the reference enriches only then, main.rs:22-25)
        check_maps(eng, oracle_rows(c))
    assert len(got[1]) == (plan.barcode_num * (plan.barcode_num - 1) // 2 if plan.barcode_num >= 3 else 0)
    eng.close()


@pytest.mark.parametrize("seed", _random_case_seeds())
@pytest.mark.parametrize("kernel", ["generic", "specialised"], indirect=True)
def test_enrichment_of_random_schemes(seed, kernel):
    c = cases.random_case(seed, n=2000)
    plan = make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    if plan.mode != "dense":
        with pytest.raises(_pkg().BarcodeCountError):
            eng.enrichment()
    else:
        check_against_rows(eng)
        check_maps(eng, oracle_rows(c))
    eng.close()


@pytest.mark.parametrize("name", ["del_random", "example_files_samples", "example_files_random_nosample", "rnd_rb_2"])
def test_random_barcode_enrich_before_and_after_finish(name):
    c = cases.build_case(name, seed=17, n=4000)
    plan = make_plan(c)
    if plan.mode != "dense":
        pytest.fail("expected a dense random-barcode case: %s" % name)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    before = eng.enrichment()
    again = eng.enrichment()
    assert_same(again, before)
    counters = eng.counters()
    n = eng.finish()
    assert n > 0
    assert_same(eng.enrichment(), before)
    assert eng.counters() == counters and eng.finish() == n  # the call changes nothing the engine holds
    check_against_rows(eng)
    check_maps(eng, oracle_rows(c))
    eng.close()


@pytest.mark.parametrize("name", ["del_mismatch_quality", "del_dense_ties"])
def test_two_level_counting_enriched_straight_after_submit(name, monkeypatch):
    """bit map + count log (forced on for any table size); enrich with no sync between the submit and the call"""
    import torch
    monkeypatch.setenv("BC_BITMAP_MIN_ENTRIES", "1")
    monkeypatch.setenv("BC_COUNT_LOG", "1")
    c = cases.build_case(name, seed=19, n=5000)
    plan = make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    stride = seq.shape[1]
    dseq = torch.from_numpy(seq.reshape(-1)).cuda()
    dqual = torch.from_numpy(qual.reshape(-1)).cuda()
    dlens = torch.from_numpy(lens.view(np.int16)).cuda()
    torch.cuda.synchronize()
    eng = _pkg().Engine(plan, device=0)
    eng.submit_device(dseq.data_ptr(), dqual.data_ptr(), seq.shape[0], stride, stride, dlens.data_ptr())
    got = eng.enrichment()
    assert eng.count_log_folds() == 1
    s, b, c_ = eng.rows()
    assert_same(got, marginals(s, b, c_, len(plan.samples()), sizes_of(plan)))
    assert_same(eng.enrichment(), got)
    check_maps(eng, oracle_rows(c))
    eng.close()


@pytest.mark.parametrize("name", ["reads_of_520_bases", "groups_of_40_and_36_bases", "random_barcode_reads_of_400_bases"])
def test_wave_per_read_kernel(name):
    c = _long_cases()[name]
    plan = make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    assert eng.kernel_name() == "long_match_kernel"
    check_against_rows(eng)
    check_maps(eng, oracle_rows(c))
    eng.close()


def test_u64_sums_and_indices_above_2_32():
    """a caller-owned table of 5 x 1000^3 u32 (20 GB): entries near 2^32-1, many of them above index 2^32, runs of 64
    full entries in one wavefront chunk (sums above 2^32 on one atomic) and across an innermost wrap"""
    import torch
    pkg = _pkg()
    plan = pkg.Plan("[6]ACGTAC{5}TTGG{5}CCAA{5}GGTT")
    rng = np.random.default_rng(5)
    for i, s in enumerate(readgen.make_set(rng, 5, 6, 2)):
        plan.add_sample(s, "S%d" % i)
    for g in range(3):
        for i, s in enumerate(readgen.make_set(rng, 1000, 5, 1)):
            plan.add_counted(g, s, "b%d_%d" % (g, i))
    sizes = sizes_of(plan)
    assert sizes == [1000, 1000, 1000]
    entries = plan.table_entries
    assert entries == 5 * 10 ** 9
    idx = rng.integers(0, entries, 3000, dtype=np.int64)
    base = 4_300_000_064  # a multiple of 64, innermost digit 64: no wrap inside its chunk
    assert base % 64 == 0 and base % 1000 + 63 < 1000
    wrap = next(b for b in range(2 ** 32 // 64 * 64 + 64, 2 ** 32 + 64_000, 64) if b % 1000 > 936)  # an innermost wrap
    assert (wrap % 1000) + 63 >= 1000
    idx = np.unique(np.concatenate([idx, np.arange(base, base + 64), np.arange(wrap, wrap + 64), [entries - 1, 2 ** 32,
                                                                                                   2 ** 32 - 1]]))
    vals = rng.integers(2 ** 32 - 4096, 2 ** 32, idx.size, dtype=np.uint64)
    table = torch.zeros(entries, dtype=torch.int32, device="cuda")
    table[torch.from_numpy(idx).cuda()] = torch.from_numpy(vals.astype(np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    eng = pkg.Engine(plan, device=0, table_ptr=table.data_ptr())
    got = eng.enrichment()
    s = idx // 10 ** 9
    b = np.stack([(idx // 10 ** 6) % 1000, (idx // 1000) % 1000, idx % 1000], axis=1)
    exp = marginals(s, b, vals, 5, sizes)
    assert_same(got, exp)
    assert int(got[0][0][4].max()) >= 2 ** 32  # (u64 sums really happened)
    assert int(exp[0][0][4, (base // 10 ** 6) % 1000]) > 2 ** 36
    eng.close()
    del table
    torch.cuda.empty_cache()


def test_eighteen_counted_barcodes():
    """as many counted barcodes as a plan may have groups (no sample barcode): all 153 pairs, on a caller-owned table"""
    import torch
    pkg = _pkg()
    consts = ["AC", "GT", "CA", "TG", "AG", "CT", "GA", "TC", "AA", "CC", "GG", "TT", "ACG", "CGT", "GTA", "TAC", "AGC",
              "GCA", "TTG"]
    plan = pkg.Plan("".join(consts[g] + "{2}" for g in range(18)) + consts[18])
    for g in range(18):
        for i, seq in enumerate(["AC", "GT", "CA"][:2 + g % 2]):
            plan.add_counted(g, seq, "b%d_%d" % (g, i))
    sizes = sizes_of(plan)
    entries = plan.table_entries
    assert plan.barcode_num == 18 and plan.mode == "dense" and entries == int(np.prod(sizes))
    rng = np.random.default_rng(18)
    vals = rng.integers(0, 5, entries).astype(np.uint32) * (rng.random(entries) < 0.3)
    table = torch.from_numpy(vals.view(np.int32)).cuda()
    torch.cuda.synchronize()
    eng = pkg.Engine(plan, device=0, table_ptr=table.data_ptr())
    got = eng.enrichment()
    idx = np.flatnonzero(vals)
    digits, r = [], idx.copy()
    for n in reversed(sizes):
        digits.append(r % n)
        r //= n
    b = np.stack(digits[::-1], axis=1)
    assert_same(got, marginals(np.zeros(idx.size, dtype=np.int64), b, vals[idx].astype(np.uint64), 1, sizes))
    assert len(got[1]) == 153
    eng.close()


def test_reset_null_doubles_and_sparse_plans():
    pkg = _pkg()
    c = cases.build_case("del_mismatch_quality", seed=23, n=3000)
    plan = make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    full = check_against_rows(eng)
    singles, doubles = eng.enrichment(doubles=False)  # double_counts = NULL
    assert doubles == {}
    assert_same((singles, {}), (full[0], {}))
    eng.reset_results()
    singles, doubles = eng.enrichment()
    assert all(not a.any() for a in singles) and all(not a.any() for a in doubles.values())
    assert len(doubles) == 3
    e = pkg.ResultsEnrichment().fill(eng)
    assert all(m == {} for m in e.single_hashmap.values()) and all(m == {} for m in e.double_hashmap.values())
    eng.close()
    c = cases.build_case("raw_counted", seed=23, n=500)
    plan = make_plan(c)
    assert plan.mode == "sparse"
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    with pytest.raises(pkg.BarcodeCountError) as ex:
        eng.enrichment()
    assert ex.value.code == -2 and "raw captures" in str(ex.value)
    lib = plan._lib
    import ctypes as C
    ns = C.c_uint64()
    assert lib.bc_engine_enrich_entries(eng._e, C.byref(ns), None) == -2
    eng.close()


def _oracle_rows_mp(case, n):
    import mp_rank
    import workloads
    w = mp_rank.make_case(case)
    seq, qual = w.synth.generate_host(0, n)
    o = workloads.oracle_for(w)
    o.process_batch(seq, qual if w.min_quality > 0 else None, w.read_len, w.read_len)
    return w, o.rows()


@pytest.mark.parametrize("case,world,n,root", [("dense", 2, 40_001, 0), ("dense", 3, 30_000, 2),
                                               ("dense+bits", 2, 40_001, 1), ("dense+bits", 3, 30_000, 0),
                                               ("random", 2, 40_000, 0), ("random", 3, 30_000, 1)])
def test_ranks_on_one_gpu_enrich_the_job(tmp_path, case, world, n, root):
    cdir = tmp_path / "comm"
    cdir.mkdir()
    out = tmp_path / "job.json"
    env = dict(os.environ, BC_COMM_TIMEOUT_S="120")
    if case.endswith("+bits"):
        case = case[:-5]
        env["BC_BITMAP_MIN_ENTRIES"] = "1"
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_rank_enrich.py"), case, str(r), str(world),
                               str(cdir), str(n), str(root), str(out)], env=env, stderr=subprocess.PIPE)
             for r in range(world)]
    for r, p in enumerate(procs):
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (r, err.decode()[-1500:])
    job = json.load(open(out))
    w, rows = _oracle_rows_mp(case, n)
    assert [tuple(r) for r in job["rows"]] == rows
    samples = {x: i for i, (x, _) in enumerate(w.plan.samples())}
    sets = [{x: i for i, (x, _) in enumerate(w.plan.counted(g))} for g in range(w.plan.barcode_num)]
    s = np.array([samples[r[0]] for r in rows])
    b = np.array([[sets[g][x] for g, x in enumerate(r[1].split(","))] for r in rows])
    cnt = np.array([r[2] for r in rows], dtype=np.uint64)
    sizes = [len(x) for x in sets]
    es, ed = marginals(s, b, cnt, len(samples), sizes)
    got = ([np.array(a, dtype=np.uint64) for a in job["singles"]],
           {tuple(map(int, k.split(","))): np.array(v, dtype=np.uint64) for k, v in job["doubles"].items()})
    assert_same(got, (es, ed))
