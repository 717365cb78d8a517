"""The Single and Double enrichment files of raw-key plans as text from the device (bc_engine_render_raw_enriched /
bc_engine_render_raw_enriched_merged: csrc/bc_raw_enrich_render.h, the sums made by csrc/bc_sort.h + csrc/bc_reduce.h).
The expected text never comes from the renderer: it is built in Python from the engine's rows (bc_engine_finish +
bc_engine_row_text) by the formatter of tests/raw_enrich_render_lib.py, which fills the Single / Double maps row by row
as add_single / add_double do, and compared byte for byte."""
import os

import numpy as np
import pytest

import cases
import readgen
import raw_enrich_render_lib as rel
import raw_render_cases as rrc
import raw_render_lib as rrl
from test_gpu_parity import make_plan, run_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (rel.SINGLE, rel.DOUBLE)


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def run(c, plan=None):
    plan = plan or make_plan(c)
    seq, qual, lens = readgen.to_arrays(c["reads"])
    eng, _, _ = run_device(plan, seq, qual, lens, seq.shape[1], seq.shape[1])
    return eng


def n_samples_of(plan):
    return len(plan.samples()) if plan.sample_barcode else 1


def expected(plan, scheme, result_rows, cols, merged, kind):
    groups, rows = rrc.rows_of(plan, scheme, result_rows)
    return rel.render_py(groups, rows, list(cols), merged, kind)[0]


def check_engine(eng, scheme, merged_orders):
    """every per-sample and the given merged files of both kinds against the formatter -> (rows, {(kind, s): text})"""
    plan = eng.plan
    rows = eng.result_rows()
    texts = {}
    for kind in KINDS:
        for s in range(n_samples_of(plan)):
            texts[kind, s] = eng.render_raw_enriched(kind, s)
            assert texts[kind, s] == expected(plan, scheme, rows, [s], False, kind), (kind, s)
        for cols in merged_orders:
            assert eng.render_raw_enriched_merged(kind, cols) == expected(plan, scheme, rows, cols, True, kind), (kind, cols)
    return rows, texts


_DEL = {}


def del_engine():
    """the DEL raw-key engine and its rows: made once, shared, never changed"""
    if not _DEL:
        c = rrc.del_raw_case()
        eng = run(c)
        _DEL.update(case=c, eng=eng, rows=eng.result_rows())
    return _DEL


def test_del_three_raw_groups_four_samples():
    d = del_engine()
    eng, scheme = d["eng"], d["case"]["scheme"]
    assert eng.plan.mode == "sparse" and n_samples_of(eng.plan) == 4
    assert len(d["rows"]) > 4 * 2048  # several tiles of the sort and of the reduction
    rows, texts = check_engine(eng, scheme, [[0, 1, 2, 3], [3, 1], [2, 2, 0]])
    assert rows == d["rows"]
    for kind in KINDS:
        chunks = []
        n = eng.render_raw_enriched(kind, 1, on_text=chunks.append)
        assert b"".join(chunks) == texts[kind, 1] and n == texts[kind, 1].count(b"\n") > 2048
        chunks = []
        n = eng.render_raw_enriched_merged(kind, [3, 1], on_text=chunks.append)
        whole = eng.render_raw_enriched_merged(kind, [3, 1])
        assert b"".join(chunks) == whole and n == whole.count(b"\n")
    # the order, said without the renderer: lines ascend by (group or pair, digits) computed from their own text
    pairs = [(0, 1), (0, 2), (1, 2)]
    for (kind, s), t in texts.items():
        keys = []
        for line in t.split(b"\n")[:-1]:
            f = line.split(b",")
            assert len(f) == 4
            held = tuple(g for g in range(3) if f[g])
            assert len(held) == kind and all(len(f[g]) == 8 for g in held)
            keys.append(((held[0],) if kind == rel.SINGLE else (pairs.index(held),)) + tuple(rrl.code_of(f[g].decode()) for g in held))
        assert keys == sorted(keys) and len(set(keys)) == len(keys) and keys
    # every row adds its count to one Single line per group and one Double line per pair
    total = sum(r[2] for r in rows)
    for kind in KINDS:
        assert sum(int(line.rsplit(b",", 1)[1]) for s in range(4) for line in texts[kind, s].split(b"\n")[:-1]) == 3 * total


def test_raw_counted_case():
    """cases.build_case("raw_counted"): two counted barcodes, so there is no Double file (no line, BC_OK)"""
    c = cases.build_case("raw_counted", seed=29, n=4000)
    eng = run(c)
    assert eng.plan.mode == "sparse" and eng.plan.barcode_num == 2
    S = n_samples_of(eng.plan)
    rows, texts = check_engine(eng, c["scheme"], [list(range(S))])
    assert len(rows) > 20 and all(texts[rel.SINGLE, s] for s in range(S))
    for s in range(S):
        assert texts[rel.DOUBLE, s] == b""
    chunks = []
    assert eng.render_raw_enriched_merged(rel.DOUBLE, range(S), on_text=chunks.append) == 0 and not chunks
    assert eng.raw_enrich_reduces() == 1  # (the Single set alone was built)
    eng.close()


def test_one_counted_group():
    """a CRISPR run without a counted-barcodes file: Single is the counts file, line for line; there is no Double file"""
    rng = np.random.default_rng(53)
    c = {"scheme": cases.CRISPR_SCHEME, "samples": None, "counted": None, "kwargs": {}}
    c["reads"] = readgen.gen_reads(rng, cases.CRISPR_SCHEME, 3000, 100, None, [readgen.make_set(rng, 40, 20, 3)], p_sub=0.01,
                                   p_n=0.004)
    eng = run(c)
    assert eng.plan.mode == "sparse" and eng.plan.barcode_num == 1 and n_samples_of(eng.plan) == 1
    rows, texts = check_engine(eng, c["scheme"], [[0], [0, 0]])
    assert len(rows) > 40
    assert texts[rel.SINGLE, 0] == eng.render_raw_counts(0) and texts[rel.SINGLE, 0].count(b"\n") == len(rows)
    assert eng.render_raw_enriched_merged(rel.SINGLE, [0]) == eng.render_raw_merged([0])
    assert texts[rel.DOUBLE, 0] == b"" and eng.render_raw_enriched_merged(rel.DOUBLE, [0]) == b""
    eng.close()


def test_random_barcode_known_sample_raw_counted():
    """the sums are over the counts of distinct random barcodes"""
    c = rrc.random_raw_case()
    eng = run(c)
    plan = eng.plan
    assert plan.mode == "sparse" and plan.random_barcode and n_samples_of(plan) == 3 and plan.barcode_num == 2
    rows, texts = check_engine(eng, c["scheme"], [[0, 1, 2], [2, 0]])
    total = sum(r[2] for r in rows)
    k = eng.counters()
    assert k["duplicates"] > 0 and len(rows) < total == k["matched"]
    lines = [line for s in range(3) for line in texts[rel.SINGLE, s].split(b"\n")[:-1]]
    assert sum(int(x.rsplit(b",", 1)[1]) for x in lines) == 2 * total and len(lines) < 2 * len(rows)  # keys are shared
    assert all(texts[rel.DOUBLE, s] == b"" for s in range(3))
    eng.close()


def mixed_case(n=6000, seed=47):
    """DEL scheme: barcode 1 a known set in which two sequences carry one ID, barcodes 2 and 3 raw"""
    rng = np.random.default_rng(seed)
    known = readgen.make_set(rng, 6, 8, 3)
    ids = ["bb_%d" % i for i in range(6)]
    ids[4] = ids[1]  # sequences 1 and 4: one ID
    pools = [known, readgen.make_set(rng, 7, 8, 2), readgen.make_set(rng, 5, 8, 2)]
    c = {"scheme": cases.DEL_SCHEME, "samples": {s: "Sample_%d" % i for i, s in enumerate(rrc.DEL_SAMPLES)}, "kwargs": {}}
    c["reads"] = readgen.gen_reads(rng, cases.DEL_SCHEME, n, 100, rrc.DEL_SAMPLES, pools, p_sub=0.004, p_n=0.002)
    plan = _pkg().Plan(c["scheme"])
    for s, i in c["samples"].items():
        plan.add_sample(s, i)
    for seq, i in zip(known, ids):
        plan.add_counted(0, seq, i)
    plan.set_max_errors(None, None, None)
    plan.set_min_quality(0.0)
    return c, plan, known, ids


def test_mixed_plan_with_a_shared_id():
    c, plan, known, ids = mixed_case()
    eng = run(c, plan)
    assert plan.mode == "sparse" and eng._lib.bc_engine_key_words(eng._e) == 1
    assert [i for _, i in plan.counted(0)] == ids and not plan.counted(1) and not plan.counted(2)
    rows, texts = check_engine(eng, c["scheme"], [[0, 1, 2, 3], [1, 1, 3, 0]])
    # the shared ID: one line, holding the sums of both sequences
    for s, sample in enumerate(rrc.DEL_SAMPLES):
        both = [sum(n for smp, t, n in rows if smp == sample and t.split(",")[0] == known[i]) for i in (1, 4)]
        assert min(both) > 0
        lines = [x for x in texts[rel.SINGLE, s].split(b"\n") if x.startswith(ids[1].encode() + b",")]
        assert lines == [("%s,,,%d" % (ids[1], sum(both))).encode()]
    assert any(x.startswith(ids[1].encode() + b",") and x.count(b",") == 3 and len(x.split(b",")[1]) == 8
               for x in texts[rel.DOUBLE, 0].split(b"\n"))
    eng.close()


def test_small_chunks_give_the_same_text(monkeypatch):
    """BC_RENDER_CHUNK_BYTES of a few hundred bytes, set the way the raw-key renderer's test sets it (the library reads
    it at every render)"""
    d = del_engine()
    eng = d["eng"]
    for kind in KINDS:
        monkeypatch.delenv("BC_RENDER_CHUNK_BYTES", raising=False)
        whole = [eng.render_raw_enriched(kind, 2), eng.render_raw_enriched_merged(kind, [1, 3])]
        monkeypatch.setenv("BC_RENDER_CHUNK_BYTES", "300")
        for text, call in zip(whole, (lambda f: eng.render_raw_enriched(kind, 2, on_text=f),
                                      lambda f: eng.render_raw_enriched_merged(kind, [1, 3], on_text=f))):
            chunks = []
            n = call(chunks.append)
            assert b"".join(chunks) == text and n == text.count(b"\n")
            assert len(chunks) > 100 and all(0 < len(x) <= 300 and x.endswith(b"\n") for x in chunks)


def test_builds_are_shared_until_the_counts_change():
    import torch
    c = del_engine()["case"]
    plan = make_plan(c)
    S = 4
    seq, _, lens = readgen.to_arrays(c["reads"][:3000], stride=100)
    dseq = torch.from_numpy(seq.reshape(-1)).cuda()
    dlens = torch.from_numpy(lens.view(np.int16)).cuda()
    e2 = _pkg().Engine(plan, device=0)
    e2.submit_device(dseq.data_ptr(), None, 3000, 100, 100, dlens.data_ptr())
    assert e2.raw_enrich_reduces() == 0 and e2.raw_render_sorts() == 0
    first = [e2.render_raw_enriched(rel.SINGLE, s) for s in range(S)] + [e2.render_raw_enriched_merged(rel.SINGLE, range(S))]
    assert e2.raw_enrich_reduces() == 1 and e2.raw_render_sorts() == 1 and all(first)
    double = [e2.render_raw_enriched(rel.DOUBLE, s) for s in range(S)] + [e2.render_raw_enriched_merged(rel.DOUBLE, range(S))]
    assert e2.raw_enrich_reduces() == 2 and e2.raw_render_sorts() == 1 and all(double)
    assert e2.render_raw_counts(0) and e2.render_raw_enriched(rel.SINGLE, 0) == first[0]
    assert e2.raw_enrich_reduces() == 2 and e2.raw_render_sorts() == 1
    assert e2.raw_enrich_reduce_ms() > 0
    e2.submit_device(dseq.data_ptr(), None, 3000, 100, 100, dlens.data_ptr())
    second = e2.render_raw_enriched(rel.SINGLE, 0)
    assert e2.raw_enrich_reduces() == 3 and e2.raw_render_sorts() == 2
    rows = e2.result_rows()
    assert second == expected(plan, c["scheme"], rows, [0], False, rel.SINGLE) and second != first[0]
    assert e2.render_raw_enriched_merged(rel.DOUBLE, [2, 0]) == expected(plan, c["scheme"], rows, [2, 0], True, rel.DOUBLE)
    assert e2.raw_enrich_reduces() == 4 and e2.raw_render_sorts() == 2
    e2.reset()
    assert e2.render_raw_enriched(rel.SINGLE, 0) == b"" and e2.render_raw_enriched_merged(rel.DOUBLE, [0, 1]) == b""
    e2.close()


def test_empty_engine():
    c = rrc.del_raw_case(n=10)
    eng = _pkg().Engine(make_plan(c), device=0)
    for kind in KINDS:
        chunks = []
        assert eng.render_raw_enriched(kind, 0, on_text=chunks.append) == 0 and not chunks
        assert eng.render_raw_enriched_merged(kind, [0, 1, 2, 3]) == b"" and eng.render_raw_enriched_merged(kind, []) == b""
    assert eng.raw_enrich_reduces() == 0
    eng.close()


def test_refusals():
    pkg = _pkg()
    import test_gpu_wide_keys as wk
    dense = run(cases.build_case("del_exact", seed=3, n=300))
    raw_sample = run(cases.build_case("raw_sample", seed=3, n=300))
    plan, _, reads = wk._build("barcode_seq_40", 300, 7)
    wide, _ = wk._run_engine(plan, reads, trace=False)
    assert dense.plan.mode == "dense" and raw_sample.plan.mode == "sparse" and wide._lib.bc_engine_key_words(wide._e) > 1
    for eng, word in ((dense, "bc_engine_render_enriched"), (raw_sample, "bc_engine_row_text"), (wide, "bc_engine_row_text")):
        for kind in KINDS:
            for call in (lambda: eng.render_raw_enriched(kind, 0), lambda: eng.render_raw_enriched_merged(kind, [0])):
                with pytest.raises(pkg.BarcodeCountError) as ex:
                    call()
                assert ex.value.code == -2 and word in str(ex.value)
        assert eng.raw_enrich_reduces() == 0
        eng.close()
    eng = del_engine()["eng"]
    before = eng.raw_enrich_reduces()
    for call in (lambda: eng.render_raw_enriched(3, 0), lambda: eng.render_raw_enriched_merged(0, [0]),
                 lambda: eng.render_raw_enriched(rel.SINGLE, 4), lambda: eng.render_raw_enriched_merged(rel.DOUBLE, [0, 4])):
        with pytest.raises(pkg.BarcodeCountError) as ex:
            call()
        assert ex.value.code == -1
    assert eng.raw_enrich_reduces() == before
