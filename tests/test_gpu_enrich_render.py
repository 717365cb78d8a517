"""The Single / Double enrichment files of a dense plan as text from the device (bc_engine_render_enriched /
bc_engine_render_enriched_merged, Engine.render_enriched / render_enriched_merged).  Expected text is built in Python
(tests/enrich_render_lib.py) from Engine.enrichment()'s raw sums -- an independent path: bc_engine_enrich's own scratch,
no fold, no text -- and, where an oracle exists, from the maps the reference's string path builds over the oracle's
rows; the comparison is bytes equal."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import enrich_render_lib as erl
import readgen
from test_gpu_enrich import oracle_rows, string_maps
from test_gpu_parity import make_plan, run_device
from test_gpu_render import _engine_on, _table_plan, ids_of, n_samples_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE, DOUBLE = erl.SINGLE, erl.DOUBLE


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def raw_sums(eng, kind):
    """Engine.enrichment() as sums[s][k] in the key order of bc_engine_enrich's layout"""
    singles, doubles = eng.enrichment()
    S = n_samples_of(eng.plan)
    G = eng.plan.barcode_num
    if kind == SINGLE:
        parts = [singles[g].reshape(S, -1) for g in range(G)]
    else:
        parts = [doubles[(g, h)].reshape(S, -1) for g in range(G) for h in range(g + 1, G)] if G >= 3 else []
    if not parts:
        return [[] for _ in range(S)]
    return np.concatenate(parts, axis=1).tolist()


def check_engine(eng, merged_orders=None):
    """every sample's Single and Double text and the merged texts against Engine.enrichment(); -> {(kind, sample): text}"""
    ids = ids_of(eng.plan)
    S = n_samples_of(eng.plan)
    texts = {}
    for kind in (SINGLE, DOUBLE):
        sums = raw_sums(eng, kind)
        for s in range(S):
            exp, lines = erl.render_py(ids, sums, kind, [s])
            texts[(kind, s)] = eng.render_enriched(kind, s)
            assert texts[(kind, s)] == exp, (kind, s)
            assert eng.render_enriched(kind, s, on_text=lambda ch: None) == lines
        for cols in (merged_orders or [list(range(S))]):
            assert eng.render_enriched_merged(kind, cols) == erl.render_py(ids, sums, kind, cols)[0], (kind, cols)
        if eng.plan.barcode_num < 3 and kind == DOUBLE:
            assert all(texts[(kind, s)] == b"" for s in range(S))
    return texts


def run_case(name, seed=29, n=4000):
    c = cases.build_case(name, seed=seed, n=n)
    plan = make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    return eng, c


@pytest.mark.parametrize("name", ["del_mismatch_quality", "del_dense_ties", "example_files_samples", "crispr", "del_random",
                                  "nosample"])
def test_cases_render_the_enrichment_of_what_finish_hands_out(name):
    eng, c = run_case(name)
    assert eng.plan.mode == "dense"
    S = n_samples_of(eng.plan)
    texts = check_engine(eng, [list(range(S)), list(reversed(range(S))), [0], [S - 1, 0, S - 1]])
    assert any(texts[(SINGLE, s)] for s in range(S))
    # the reference's string path over the oracle's rows: the same set of lines (IDs are the sequences, make_plan)
    single, double = string_maps(oracle_rows(c), eng.plan)
    keys = [x for x, _ in eng.plan.samples()] if eng.plan.sample_barcode else ["barcode"]
    for kind, maps in ((SINGLE, single), (DOUBLE, double)):
        for s, key in enumerate(keys):
            exp = sorted("%s,%d" % kv for kv in maps.get(key, {}).items())
            if kind == DOUBLE and eng.plan.barcode_num < 3:
                exp = []
            assert sorted(texts[(kind, s)].decode().split("\n")[:-1]) == exp, (kind, key)
    eng.close()


def _four_barcode_plan():
    pkg = _pkg()
    plan = pkg.Plan("[4]AC{3}GT{3}CA{3}TG{3}AA")
    for i, s in enumerate(["ACGT", "TTTT", "GGCC"]):
        plan.add_sample(s, "S%d" % i)
    for g in range(4):
        for i, s in enumerate(["ACG", "TTT", "GCA", "CAT", "GGG"][:3 + g % 3]):
            plan.add_counted(g, s, "g%d_%d" % (g, i))
    return plan, 3 * 4 * 5 * 3


def test_sample_without_reads_and_four_counted_barcodes():
    plan, T = _four_barcode_plan()
    assert plan.table_entries == 3 * T
    rng = np.random.default_rng(4)
    vals = (rng.integers(1, 5000, 3 * T) * (rng.random(3 * T) < 0.4)).astype(np.uint32)
    vals[T:2 * T] = 0  # sample 1 receives nothing
    eng = _engine_on(plan, vals)
    texts = check_engine(eng, [[0, 1, 2], [1], [2, 1], [1, 1, 0]])
    assert texts[(SINGLE, 1)] == b"" and texts[(DOUBLE, 1)] == b"" and eng.render_enriched_merged(DOUBLE, [1]) == b""
    assert texts[(SINGLE, 0)].count(b",") == 4 * texts[(SINGLE, 0)].count(b"\n")
    assert texts[(SINGLE, 0)].startswith(b"g0_0,,,,") and b"\n,,,g3_2," in texts[(SINGLE, 0)]
    assert texts[(DOUBLE, 0)].startswith(b"g0_0,g1_0,,,") and b"\n,,g2_4,g3_2," in texts[(DOUBLE, 0)]
    eng.close()


def test_caller_owned_table_whose_marginals_pass_2_32():
    S = 2
    plan = _table_plan([["a%d" % i for i in range(3)], ["b%d" % i for i in range(700)], ["c%d" % i for i in range(5)]], S)
    T = 3 * 700 * 5
    vals = np.zeros(S * T, dtype=np.uint32)
    vals[:T] = 4294967295          # every single of sample 0 is far above 2^32
    vals[T + 7] = 4294967295
    vals[T + 12] = 4294967295      # (0, 1, 2) and (0, 2, 2): single a0 and pair (a0, c2) = 2^33 - 2
    vals[T + 3499] = 1
    eng = _engine_on(plan, vals)
    texts = check_engine(eng, [[0, 1], [1, 0, 1]])
    assert b"a0,,,%d\n" % (4294967295 * 3500) in texts[(SINGLE, 0)]
    assert b"a0,,,8589934591\n" in texts[(SINGLE, 1)] and b"a0,,c2,8589934590\n" in texts[(DOUBLE, 1)]
    # a table the caller owns may change unseen: no sums are kept for it
    import torch
    eng._keep[T + 3499] = 5
    torch.cuda.synchronize()
    passes = eng.enrich_render_passes()
    assert b",b699,,5\n" in eng.render_enriched(SINGLE, 1)
    eng.render_enriched(DOUBLE, 1)
    assert eng.enrich_render_passes() == passes + 2
    eng.close()


@pytest.mark.parametrize("name", ["del_mismatch_quality", "del_dense_ties"])
def test_two_level_counting_and_log_mode_rendered_straight_after_submit(name, monkeypatch):
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
    S = n_samples_of(plan)
    before = {(k, s): eng.render_enriched(k, s) for k in (SINGLE, DOUBLE) for s in range(S)}  # no sync, no finish
    assert eng.count_log_folds() == 1
    rows1 = [a.copy() for a in eng.rows()]
    texts = check_engine(eng)
    assert texts == before and any(before.values())
    rows2 = eng.rows()
    key = lambda r: sorted(zip(r[0].tolist(), map(tuple, r[1].tolist()), r[2].tolist()))
    assert key(rows1) == key(rows2)  # the render leaves finish()'s rows as they were
    eng.close()


def test_shared_ids_inside_a_set_are_one_key():
    ids = [["A", "B", "A", "C", "B"], ["x", "x", "y"], ["p", "q", "p"]]
    plan = _table_plan(ids, 2)
    T = 5 * 3 * 3
    rng = np.random.default_rng(11)
    vals = (rng.integers(1, 2 ** 32, 2 * T, dtype=np.uint64) * (rng.random(2 * T) < 0.5)).astype(np.uint32)
    vals[:T] = 0
    vals[(2 * 3 + 1) * 3 + 2] = 9  # sample 0 counts only (A#2, x#1, p#2): every key exists through folded entries alone
    eng = _engine_on(plan, vals)
    texts = check_engine(eng, [[0, 1], [1, 0]])
    assert texts[(SINGLE, 0)] == b"A,,,9\n,x,,9\n,,p,9\n"
    assert texts[(DOUBLE, 0)] == b"A,x,,9\nA,,p,9\n,x,p,9\n"
    assert texts[(SINGLE, 1)].count(b"\n") <= 3 + 2 + 2
    eng.close()


def test_chunk_sizes_callback_row_counts_and_errors(monkeypatch):
    pkg = _pkg()
    S = 3
    plan = _table_plan([["a%d" % i for i in range(40)], ["Z" * 300] + ["b%d" % i for i in range(699)], ["c0", "c1"]], S)
    T = 40 * 700 * 2
    rng = np.random.default_rng(3)
    vals = (rng.integers(1, 2 ** 32, S * T, dtype=np.uint64) * (rng.random(S * T) < 0.3)).astype(np.uint32)
    eng = _engine_on(plan, vals)
    monkeypatch.delenv("BC_RENDER_CHUNK_BYTES", raising=False)
    whole = {(k, s): eng.render_enriched(k, s) for k in (SINGLE, DOUBLE) for s in (0, 2)}
    whole[(SINGLE, "m")] = eng.render_enriched_merged(SINGLE, [2, 0, 1])
    whole[(DOUBLE, "m")] = eng.render_enriched_merged(DOUBLE, [2, 0, 1])
    ids = ids_of(plan)
    assert whole[(DOUBLE, 2)] == erl.render_py(ids, raw_sums(eng, DOUBLE), DOUBLE, [2])[0]
    for size in ("1", "331", "1009"):  # 1: clamps to the longest possible line, the minimum
        monkeypatch.setenv("BC_RENDER_CHUNK_BYTES", size)
        for (kind, s), exp in whole.items():
            chunks = []
            n = (eng.render_enriched_merged(kind, [2, 0, 1], on_text=chunks.append) if s == "m"
                 else eng.render_enriched(kind, s, on_text=chunks.append))
            assert all(ch.endswith(b"\n") and len(ch) > 0 for ch in chunks)
            assert b"".join(chunks) == exp, (size, kind, s)
            assert n == exp.count(b"\n")
            assert len(chunks) > 1 and max(map(len, chunks)) <= max(int(size), 700)
    monkeypatch.setenv("BC_RENDER_CHUNK_BYTES", "331")
    # a callback that stops: BC_ERR_STATE, and the engine renders correctly afterwards
    seen = []

    def stop(chunk):
        seen.append(chunk)
        raise RuntimeError("enough")

    with pytest.raises(RuntimeError):
        eng.render_enriched(SINGLE, 0, on_text=stop)
    assert len(seen) == 1
    fn = pkg._lib.TEXT_FN(lambda tp, n, user: 1)
    n = C.c_uint64(5)
    assert eng._lib.bc_engine_render_enriched(eng._e, DOUBLE, 0, fn, None, C.byref(n)) == -5
    assert eng._lib.bc_engine_render_enriched(eng._e, DOUBLE, 0, fn, None, None) == -5  # n_rows may be NULL
    cols = (C.c_uint32 * 2)(0, 1)
    assert eng._lib.bc_engine_render_enriched_merged(eng._e, SINGLE, cols, 2, fn, None, C.byref(n)) == -5
    assert eng.render_enriched(SINGLE, 0) == whole[(SINGLE, 0)]
    monkeypatch.delenv("BC_RENDER_CHUNK_BYTES")
    for call in (lambda: eng.render_enriched(SINGLE, S), lambda: eng.render_enriched(0, 0), lambda: eng.render_enriched(3, 0),
                 lambda: eng.render_enriched_merged(DOUBLE, [0, S]), lambda: eng.render_enriched_merged(7, [0])):
        with pytest.raises(pkg.BarcodeCountError) as ex:
            call()
        assert ex.value.code == -1
    assert eng.render_enriched_merged(DOUBLE, [2, 0, 1]) == whole[(DOUBLE, "m")]
    assert eng.render_enriched_merged(SINGLE, []) == b""
    eng.close()


def test_raw_key_plan_is_unsupported():
    pkg = _pkg()
    eng, _ = run_case("raw_counted", seed=23, n=500)
    assert eng.plan.mode == "sparse"
    for call in (lambda: eng.render_enriched(SINGLE, 0), lambda: eng.render_enriched_merged(DOUBLE, [0])):
        with pytest.raises(pkg.BarcodeCountError) as ex:
            call()
        assert ex.value.code == -2 and "raw captures" in str(ex.value)
    eng.close()


def _submit(eng, seq, qual, lens):
    import torch
    stride = seq.shape[1]
    d = [torch.from_numpy(seq.reshape(-1)).cuda(), torch.from_numpy(qual.reshape(-1)).cuda(),
         torch.from_numpy(lens.view(np.int16)).cuda()]
    torch.cuda.synchronize()
    eng.submit_device(d[0].data_ptr(), d[1].data_ptr(), seq.shape[0], stride, stride, d[2].data_ptr())
    eng.sync()
    return d


def _all_texts(eng):
    S = n_samples_of(eng.plan)
    out = {(k, s): eng.render_enriched(k, s) for k in (SINGLE, DOUBLE) for s in range(S)}
    out["m"] = [eng.render_enriched_merged(k, list(range(S))) for k in (SINGLE, DOUBLE)]
    return out


@pytest.mark.parametrize("name", ["del_mismatch_quality", "del_random"])
def test_kept_sums_are_never_stale(name):
    """render, submit more reads, render again: the text of a fresh engine given all the reads; the same across
    reset_results; and two renders in a row are the same bytes"""
    pkg = _pkg()
    c = cases.build_case(name, seed=41, n=4000)
    plan = make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    half = seq.shape[0] // 2
    eng = pkg.Engine(plan, device=0)
    _submit(eng, seq[:half], qual[:half], lens[:half])
    assert eng.enrich_render_passes() == 0
    first = _all_texts(eng)
    assert eng.enrich_render_passes() == 1  # the 2 (S + 1) renders of one state of the counts: one pass over the table
    assert _all_texts(eng) == first and eng.enrich_render_passes() == 1  # served from the kept sums
    eng.enrichment()
    eng.result_rows()
    assert _all_texts(eng) == first and eng.enrich_render_passes() == 1  # (enrich and finish change no count)
    _submit(eng, seq[half:], qual[half:], lens[half:])
    second = _all_texts(eng)
    assert eng.enrich_render_passes() == 2
    fresh = pkg.Engine(plan, device=0)
    _submit(fresh, seq, qual, lens)
    whole = _all_texts(fresh)
    assert second == whole and second != first
    check_engine(eng)
    passes = eng.enrich_render_passes()
    eng.reset_results()
    assert not any(_all_texts(eng)[(SINGLE, s)] for s in range(n_samples_of(plan)))
    assert eng.enrich_render_passes() == passes + 1
    _submit(eng, seq[:half], qual[:half], lens[:half])
    assert _all_texts(eng) == first
    eng.reset()
    _submit(eng, seq, qual, lens)
    assert _all_texts(eng) == whole
    fresh.close()
    eng.close()


@pytest.mark.parametrize("case,n", [("dense", 40_001), ("random", 40_000)])
def test_root_renders_the_job_after_finish_all(tmp_path, case, n):
    """2 ranks on one GPU over the message-file transport: the root's text against the job's rows"""
    cdir = tmp_path / "comm"
    cdir.mkdir()
    out = tmp_path / "job.json"
    env = dict(os.environ, BC_COMM_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_rank_enrich_render.py"), case, str(r), "2",
                               str(cdir), str(n), "0", str(out)], env=env, stderr=subprocess.PIPE) for r in range(2)]
    for r, p in enumerate(procs):
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (r, err.decode()[-1500:])
    job = json.load(open(out))
    import mp_rank
    plan = mp_rank.make_case(case).plan
    ids = ids_of(plan)
    G = plan.barcode_num
    S = n_samples_of(plan)
    samples = {x: i for i, (x, _) in enumerate(plan.samples())}
    sets = [{x: i for i, (x, _) in enumerate(plan.counted(g))} for g in range(G)]
    assert job["rows"]
    for kind, name in ((SINGLE, "single"), (DOUBLE, "double")):
        ks = erl.keys(ids, kind)
        at = {fields: k for k, (fields, _) in enumerate(ks)}
        sums = [[0] * len(ks) for _ in range(S)]
        for sample, tup, cnt in job["rows"]:
            d = [sets[g][x] for g, x in enumerate(tup.split(","))]
            s = samples.get(sample, 0)
            if kind == SINGLE:
                for g in range(G):
                    sums[s][at[((g, d[g]),)]] += cnt
            elif G >= 3:
                for g in range(G):
                    for h in range(g + 1, G):
                        sums[s][at[((g, d[g]), (h, d[h]))]] += cnt
        for s in range(S):
            assert job[name][s].encode("latin-1") == erl.render_py(ids, sums, kind, [s])[0], (name, s)
        cols = list(reversed(range(S)))
        assert job[name + "_merged"].encode("latin-1") == erl.render_py(ids, sums, kind, cols)[0], name
    assert any(job["single"])
