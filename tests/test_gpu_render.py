"""The counts files of a dense plan as text from the device (bc_engine_render_counts / bc_engine_render_merged,
Engine.render_counts / render_merged).  Expected text is built in Python from Engine.finish() rows sorted by dense index
and the plan's IDs (or from the values a caller-owned table was filled with); the comparison is bytes equal."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import readgen
from test_gpu_parity import make_plan, run_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def ids_of(plan):
    return [[i.encode() for _, i in plan.counted(g)] for g in range(plan.barcode_num)]


def n_samples_of(plan):
    return len(plan.samples()) if plan.sample_barcode else 1


def lines_of(ids, sizes, t_sorted, columns):
    """the text of tuples t_sorted (ascending) whose counts per column are columns[k][j]"""
    out = []
    for j, t in enumerate(t_sorted):
        digits, r = [], int(t)
        for n in reversed(sizes):
            digits.append(r % n)
            r //= n
        digits.reverse()
        out.append(b",".join([ids[g][d] for g, d in enumerate(digits)] + [b"%d" % int(col[j]) for col in columns]) + b"\n")
    return b"".join(out)


def sample_maps(eng):
    """{sample index: {tuple index: count}} from Engine.rows() (bc_engine_finish + bc_engine_rows)"""
    plan = eng.plan
    sizes = [len(plan.counted(g)) for g in range(plan.barcode_num)]
    s, b, c = eng.rows()
    t = np.zeros(s.size, dtype=np.int64)
    for g, n in enumerate(sizes):
        t = t * n + b[:, g].astype(np.int64)
    maps = {i: {} for i in range(n_samples_of(plan))}
    for si, ti, ci in zip(s.tolist(), t.tolist(), c.tolist()):
        maps[si][ti] = ci
    return maps, sizes


def expected_counts(maps, sizes, ids, sample):
    ts = sorted(maps[sample])
    return lines_of(ids, sizes, ts, [[maps[sample][t] for t in ts]])


def expected_merged(maps, sizes, ids, cols):
    ts = sorted(set().union(*[set(maps[s]) for s in cols])) if cols else []
    return lines_of(ids, sizes, ts, [[maps[s].get(t, 0) for t in ts] for s in cols])


def check_engine(eng, merged_orders=None):
    """every sample's text and the merged text of all samples against the rows; -> {sample: text}"""
    ids = ids_of(eng.plan)
    maps, sizes = sample_maps(eng)
    S = n_samples_of(eng.plan)
    texts = {}
    for s in range(S):
        texts[s] = eng.render_counts(s)
        assert texts[s] == expected_counts(maps, sizes, ids, s), s
    for cols in (merged_orders or [list(range(S))]):
        assert eng.render_merged(cols) == expected_merged(maps, sizes, ids, cols), cols
    return texts


def run_case(name, seed=29, n=4000):
    c = cases.build_case(name, seed=seed, n=n)
    plan = make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    return eng


@pytest.mark.parametrize("name", ["del_mismatch_quality", "del_dense_ties", "example_files_samples", "crispr", "del_random",
                                  "nosample"])
def test_cases_render_what_finish_hands_out(name):
    eng = run_case(name)
    assert eng.plan.mode == "dense"
    S = n_samples_of(eng.plan)
    before = [eng.render_counts(s) for s in range(S)]  # before any finish
    texts = check_engine(eng, [list(range(S)), list(reversed(range(S))), [0], [S - 1, 0, S - 1]])
    assert [texts[s] for s in range(S)] == before
    assert any(texts.values())
    eng.close()


def test_sample_without_reads_and_four_counted_barcodes():
    pkg = _pkg()
    import torch
    plan = pkg.Plan("[4]AC{3}GT{3}CA{3}TG{3}AA")
    for i, s in enumerate(["ACGT", "TTTT", "GGCC"]):
        plan.add_sample(s, "S%d" % i)
    for g in range(4):
        for i, s in enumerate(["ACG", "TTT", "GCA", "CAT", "GGG"][:3 + g % 3]):
            plan.add_counted(g, s, "g%d_%d" % (g, i))
    T = 3 * 4 * 5 * 3
    assert plan.table_entries == 3 * T
    rng = np.random.default_rng(4)
    vals = (rng.integers(1, 5000, 3 * T) * (rng.random(3 * T) < 0.4)).astype(np.uint32)
    vals[T:2 * T] = 0  # sample 1 receives nothing
    table = torch.from_numpy(vals.view(np.int32)).cuda()
    torch.cuda.synchronize()
    eng = pkg.Engine(plan, device=0, table_ptr=table.data_ptr())
    texts = check_engine(eng, [[0, 1, 2], [1], [2, 1]])
    assert texts[1] == b"" and eng.render_merged([1]) == b""
    assert texts[0].count(b",") == 4 * texts[0].count(b"\n")
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
    before = [eng.render_counts(s) for s in range(S)]  # no sync, no finish: bit map read as it stands
    merged_before = eng.render_merged(list(range(S)))
    assert eng.count_log_folds() == 1
    rows1 = [a.copy() for a in eng.rows()]
    texts = check_engine(eng)
    assert [texts[s] for s in range(S)] == before and eng.render_merged(list(range(S))) == merged_before
    rows2 = eng.rows()
    key = lambda r: sorted(zip(r[0].tolist(), map(tuple, r[1].tolist()), r[2].tolist()))
    assert key(rows1) == key(rows2)  # the render leaves finish()'s rows as they were
    eng.close()


def _table_plan(ids_per_group, n_samples):
    """a dense plan whose known sets have the given IDs (sequences are made up; nothing is counted through it)"""
    pkg = _pkg()
    G = len(ids_per_group)
    L = max(2, int(np.ceil(np.log(max(len(g) for g in ids_per_group)) / np.log(4))) + 1)
    consts = ["AC", "GT", "CA", "TG", "AG"]
    scheme = ("[4]" if n_samples else "") + "".join(consts[g] + "{%d}" % L for g in range(G)) + consts[G]
    plan = pkg.Plan(scheme)
    for i in range(n_samples):
        plan.add_sample("".join("ACGT"[(i >> (2 * k)) & 3] for k in range(4)), "S%d" % i)
    for g, ids in enumerate(ids_per_group):
        for i, ident in enumerate(ids):
            plan.add_counted(g, "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(L)), ident)
    return plan


def _engine_on(plan, vals):
    import torch
    table = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    eng = _pkg().Engine(plan, device=0, table_ptr=table.data_ptr())
    eng._keep = table
    return eng


def _expect_from_values(plan, vals, S):
    ids = ids_of(plan)
    sizes = [len(g) for g in ids]
    T = vals.size // S
    maps = {s: {int(t): int(vals[s * T + t]) for t in np.flatnonzero(vals[s * T:(s + 1) * T])} for s in range(S)}
    return maps, sizes, ids


BOUNDARY_COUNTS = [1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999,
                   100000000, 999999999, 1000000000, 4294967295]


def _chosen_table():
    """3 samples x (40 x 700 = 28,000 tuples): every digit length, index 0 and T-1, both sides of every slice and chunk
    boundary, a run of 10,000 empty entries, a fully dense stretch"""
    S, T = 3, 28000
    vals = np.zeros(S * T, dtype=np.uint32)
    k = 0
    for i in range(0, S * T, 64):  # both sides of every 64-entry chunk boundary
        for j in (i - 1, i):
            if j >= 0:
                vals[j] = BOUNDARY_COUNTS[k % len(BOUNDARY_COUNTS)]
                k += 1
    for s in range(S):  # index 0 / T-1 of every slice = both sides of every slice boundary
        vals[s * T] = 4294967295
        vals[s * T + T - 1] = 1000000000 + s
    vals[T + 5000:T + 15000] = 0  # 10,000 empty entries inside sample 1
    vals[2 * T + 3000:2 * T + 5000] = np.arange(1, 2001, dtype=np.uint32) * 2147483  # a fully dense stretch
    return S, T, vals


def test_caller_owned_table_with_chosen_values():
    S, T, vals = _chosen_table()
    plan = _table_plan([["a%d" % i for i in range(40)], ["b%d" % i for i in range(700)]], S)
    assert plan.table_entries == S * T
    eng = _engine_on(plan, vals)
    maps, sizes, ids = _expect_from_values(plan, vals, S)
    for s in range(S):
        assert eng.render_counts(s) == expected_counts(maps, sizes, ids, s)
    for cols in ([0, 1, 2], [2, 0, 1], [1, 1], [2]):
        assert eng.render_merged(cols) == expected_merged(maps, sizes, ids, cols)
    # the union is over the listed samples only
    only2 = next(t for t in maps[2] if t not in maps[0] and t not in maps[1])
    digits = ids[0][only2 // 700] + b"," + ids[1][only2 % 700] + b","
    assert digits not in eng.render_merged([0, 1]) and digits in eng.render_merged([0, 2])
    eng.close()


def test_ids_empty_long_and_odd_and_a_pool_beyond_lds():
    odd = ["", "Z" * 300, "a,b", 'say "hi"', "é中🙂", "C1=CC=C(C=C1)C(=O)O"]
    big = ["id%d_%s" % (i, "x" * (i % 7)) for i in range(100_000)]
    plan = _table_plan([odd, big], 0)
    T = len(odd) * len(big)
    assert plan.table_entries == T
    rng = np.random.default_rng(8)
    vals = (rng.integers(1, 2 ** 32, T, dtype=np.uint64) * (rng.random(T) < 0.05)).astype(np.uint32)
    vals[0], vals[T - 1] = 1, 2
    vals[len(big):len(big) + 300] = 7  # a dense stretch of 300-byte lines: chunks wider than one staging window
    eng = _engine_on(plan, vals)
    maps, sizes, ids = _expect_from_values(plan, vals, 1)
    exp = expected_counts(maps, sizes, ids, 0)
    got = eng.render_counts(0)
    assert got == exp
    assert eng.render_merged([0, 0]) == expected_merged(maps, sizes, ids, [0, 0])
    eng.close()


def test_chunk_sizes_callback_and_row_counts(monkeypatch):
    S, T, vals = _chosen_table()
    plan = _table_plan([["a%d" % i for i in range(40)], ["", "Z" * 300] + ["b%d" % i for i in range(698)]], S)
    eng = _engine_on(plan, vals)
    pkg = _pkg()
    monkeypatch.delenv("BC_RENDER_CHUNK_BYTES", raising=False)
    whole = {("c", s): eng.render_counts(s) for s in range(S)}
    whole[("m",)] = eng.render_merged([2, 0, 1])
    maps, sizes, ids = _expect_from_values(plan, vals, S)
    assert whole[("c", 1)] == expected_counts(maps, sizes, ids, 1)
    for size in ("1", "331", "1009", "4099", "65537"):  # 1: clamps to the longest possible line, the minimum
        monkeypatch.setenv("BC_RENDER_CHUNK_BYTES", size)
        for key, exp in whole.items():
            chunks = []
            n = (eng.render_counts(key[1], on_text=chunks.append) if key[0] == "c"
                 else eng.render_merged([2, 0, 1], on_text=chunks.append))
            assert all(ch.endswith(b"\n") and len(ch) > 0 for ch in chunks)
            assert b"".join(chunks) == exp, (size, key)
            assert n == exp.count(b"\n")
            if int(size) < len(exp):
                assert len(chunks) > 1 and max(map(len, chunks)) <= max(int(size), 400)
    # a callback that stops: BC_ERR_STATE, and the engine renders correctly afterwards
    seen = []

    def stop(chunk):
        seen.append(chunk)
        raise RuntimeError("enough")

    with pytest.raises(RuntimeError):
        eng.render_counts(0, on_text=stop)
    assert len(seen) == 1
    fn = pkg._lib.TEXT_FN(lambda tp, n, user: 1)
    n = C.c_uint64(5)
    assert eng._lib.bc_engine_render_counts(eng._e, 0, fn, None, C.byref(n)) == -5
    assert eng._lib.bc_engine_render_counts(eng._e, 0, fn, None, None) == -5  # n_rows may be NULL
    with pytest.raises(pkg.BarcodeCountError) as ex:
        eng.render_counts(S)
    assert ex.value.code == -1
    assert eng.render_counts(0) == whole[("c", 0)]
    monkeypatch.delenv("BC_RENDER_CHUNK_BYTES")
    assert eng.render_merged([2, 0, 1]) == whole[("m",)]
    eng.close()


def test_table_above_2_32_entries():
    """the 5 x 1000^3 shape of the enrichment test: a handful of entries, some beyond index 2^32"""
    import torch
    pkg = _pkg()
    plan = pkg.Plan("[6]ACGTAC{5}TTGG{5}CCAA{5}GGTT")
    rng = np.random.default_rng(5)
    for i, s in enumerate(readgen.make_set(rng, 5, 6, 2)):
        plan.add_sample(s, "S%d" % i)
    for g in range(3):
        for i, s in enumerate(readgen.make_set(rng, 1000, 5, 1)):
            plan.add_counted(g, s, "b%d_%d" % (g, i))
    entries, T = plan.table_entries, 10 ** 9
    assert entries == 5 * T
    idx = np.unique(np.concatenate([rng.integers(0, entries, 200, dtype=np.int64),
                                    [0, T - 1, T, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 4 * T, 4 * T + 123456789, entries - 1]]))
    vals = rng.integers(1, 2 ** 32, idx.size, dtype=np.uint64).astype(np.uint32)
    table = torch.zeros(entries, dtype=torch.int32, device="cuda")
    table[torch.from_numpy(idx).cuda()] = torch.from_numpy(vals.view(np.int32)).cuda()
    torch.cuda.synchronize()
    eng = pkg.Engine(plan, device=0, table_ptr=table.data_ptr())
    ids = ids_of(plan)
    sizes = [1000, 1000, 1000]
    maps = {s: {} for s in range(5)}
    for i, v in zip(idx.tolist(), vals.tolist()):
        maps[i // T][i % T] = v
    for s in (0, 4):
        assert eng.render_counts(s) == expected_counts(maps, sizes, ids, s)
    assert len(maps[4]) >= 3
    assert eng.render_merged([4, 3, 0, 1, 2]) == expected_merged(maps, sizes, ids, [4, 3, 0, 1, 2])
    eng.close()
    del table
    torch.cuda.empty_cache()


def test_raw_key_plan_is_unsupported():
    pkg = _pkg()
    eng = run_case("raw_counted", seed=23, n=500)
    assert eng.plan.mode == "sparse"
    for call in (lambda: eng.render_counts(0), lambda: eng.render_merged([0])):
        with pytest.raises(pkg.BarcodeCountError) as ex:
            call()
        assert ex.value.code == -2 and "raw captures" in str(ex.value)
    eng.close()


@pytest.mark.parametrize("case,n", [("dense", 40_001), ("random", 40_000)])
def test_root_renders_the_job_after_finish_all(tmp_path, case, n):
    """2 ranks on one GPU over the message-file transport: the root's text against its own rows"""
    cdir = tmp_path / "comm"
    cdir.mkdir()
    out = tmp_path / "job.json"
    env = dict(os.environ, BC_COMM_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_rank_render.py"), case, str(r), "2", str(cdir),
                               str(n), "0", str(out)], env=env, stderr=subprocess.PIPE) for r in range(2)]
    for r, p in enumerate(procs):
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (r, err.decode()[-1500:])
    job = json.load(open(out))
    import mp_rank
    plan = mp_rank.make_case(case).plan
    ids = ids_of(plan)
    sizes = [len(g) for g in ids]
    samples = {x: i for i, (x, _) in enumerate(plan.samples())}
    sets = [{x: i for i, (x, _) in enumerate(plan.counted(g))} for g in range(plan.barcode_num)]
    maps = {i: {} for i in range(n_samples_of(plan))}
    for sample, tup, cnt in job["rows"]:
        t = 0
        for g, x in enumerate(tup.split(",")):
            t = t * sizes[g] + sets[g][x]
        maps[samples.get(sample, 0)][t] = cnt
    assert job["rows"]
    for s in maps:
        assert job["counts"][s].encode("latin-1") == expected_counts(maps, sizes, ids, s)
    cols = list(reversed(sorted(maps)))
    assert job["merged"].encode("latin-1") == expected_merged(maps, sizes, ids, cols)
