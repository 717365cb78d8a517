"""The counts files of wide-key plans as text from the device (bc_engine_render_wide_counts / bc_engine_render_wide_merged,
csrc/bc_wide_render.h, the order made by bc::sort_words_launch of csrc/bc_sort.h).  The expected text never comes from
the renderer: it is built in Python from the engine's rows (bc_engine_finish + bc_engine_row_text), grouped by sample and
ordered by the digit tuple computed from each row's own text with integers of any size (raw_render_cases.expected), and
compared byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import raw_render_cases as rrc
import raw_render_lib as rrl
import test_gpu_wide_keys as wk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ40 = wk.CASES["barcode_seq_40"]


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def key_words(eng):
    return eng._lib.bc_engine_key_words(eng._e)


def n_samples_of(plan):
    return len(plan.samples()) if plan.sample_barcode else 1


def submit(eng, reads):
    """one more batch into an engine that exists"""
    import torch
    stride = (max(len(r) for r in reads) + 3) & ~3
    seq = np.full((len(reads), stride), ord("\n"), dtype=np.uint8)
    lens = np.zeros(len(reads), dtype=np.uint16)
    for i, r in enumerate(reads):
        seq[i, :len(r)] = np.frombuffer(r.encode(), dtype=np.uint8)
        lens[i] = len(r)
    dseq = torch.from_numpy(seq.reshape(-1)).cuda()
    dlens = torch.from_numpy(lens.view(np.int16)).cuda()
    eng.submit_device(dseq.data_ptr(), None, len(reads), stride, stride, d_lens=dlens.data_ptr())
    eng.sync()


def check_engine(eng, scheme, merged_orders):
    plan = eng.plan
    rows = eng.result_rows()
    texts = {}
    for s in range(n_samples_of(plan)):
        texts[s] = eng.render_wide_counts(s)
        assert texts[s] == rrc.expected(plan, scheme, rows, [s], False), s
    for cols in merged_orders:
        assert eng.render_wide_merged(cols) == rrc.expected(plan, scheme, rows, cols, True), cols
    return rows, texts


def test_every_single_base_variant_of_a_40_mer():
    """the planes of a 40-base capture cross a payload word and a base lies astride the order key's two words: a wrong
    boundary in either shows as a wrong base or a line out of place"""
    rng = np.random.default_rng(5)
    master = "".join(rng.choice(list("ACGT"), 40))
    seqs = [master] + [master[:k] + c + master[k + 1:] for k in range(40) for c in "ACGTN" if c != master[k]]
    assert len(seqs) == 161
    reads = []
    for i, s in enumerate(seqs):
        for j in range(2 + i % 3):
            reads.append("ACGTTGCA"[:(i + j) % 8] + "GTACCAGTC" + s + "TGCATGGAC" + "TTGACA"[:1 + (i + j) % 5])
    order = np.random.default_rng(6).permutation(len(reads))
    plan = _pkg().Plan(SEQ40["scheme"])
    eng, _ = wk._run_engine(plan, [reads[i] for i in order], trace=False)
    assert plan.mode == "sparse" and key_words(eng) == 3
    before = eng.render_wide_counts(0)  # before any finish
    rows, texts = check_engine(eng, SEQ40["scheme"], [[0]])
    assert before == texts[0]
    assert sorted((t, n) for _, t, n in rows) == sorted((s, 2 + i % 3) for i, s in enumerate(seqs))
    lines = texts[0].split(b"\n")[:-1]
    codes = [rrl.code_of(x.split(b",")[0].decode()) for x in lines]
    assert codes == sorted(codes) and len(set(codes)) == 161
    eng.close()


_RANDOM40 = {}


def random40():
    """barcode_seq_40 with captures drawn at random: about one row per matched read, more than two sort tiles of them.
    Made once, shared, never changed."""
    if not _RANDOM40:
        parts = [("const", "GTACCAGTC"), ("cap", 40, None), ("const", "TGCATGGAC")]
        reads = wk._reads(parts, 6000, 21, [])
        plan = _pkg().Plan(SEQ40["scheme"])
        eng, _ = wk._run_engine(plan, reads, trace=False)
        rows = eng.result_rows()
        _RANDOM40.update(eng=eng, rows=rows, text=rrc.expected(plan, SEQ40["scheme"], rows, [0], False))
    return _RANDOM40


def test_several_sort_tiles():
    d = random40()
    assert len(d["rows"]) > 2 * 2048
    chunks = []
    n = d["eng"].render_wide_counts(0, on_text=chunks.append)
    assert b"".join(chunks) == d["text"] and n == len(d["rows"]) == d["text"].count(b"\n")
    assert any(b"N" in line for line in d["text"].split(b"\n"))


def test_small_chunks_give_the_same_text(monkeypatch):
    d = random40()
    monkeypatch.setenv("BC_RENDER_CHUNK_BYTES", "300")
    chunks = []
    n = d["eng"].render_wide_counts(0, on_text=chunks.append)
    assert b"".join(chunks) == d["text"] and n == len(d["rows"])
    assert len(chunks) > 500 and all(0 < len(x) <= 300 and x.endswith(b"\n") for x in chunks)


def test_samples_and_merged_views():
    c = wk.CASES["samples_plus_raw_35"]
    plan, _, reads = wk._build("samples_plus_raw_35", 4000, 7)
    eng, _ = wk._run_engine(plan, reads, trace=False)
    assert n_samples_of(plan) == 5 and key_words(eng) > 1
    rows, texts = check_engine(eng, c["scheme"], [[0, 1, 2, 3, 4], [3, 1], [2, 2, 0]])
    assert len(rows) > 500 and sum(t.count(b"\n") for t in texts.values()) == len(rows)
    merged = eng.render_wide_merged(range(5)).split(b"\n")[:-1]
    assert len(merged) == len({t for _, t, _ in rows}) < len(rows)  # tuples shared between samples: runs longer than 1
    assert any(b",0" in x for x in merged)
    eng.close()


@pytest.mark.parametrize("name", ["known_plus_random_30", "raw_plus_random_28"])
def test_random_barcodes_count_distinct(name):
    c = wk.CASES[name]
    plan, _, reads = wk._build(name, 4000, 7)
    eng, _ = wk._run_engine(plan, reads, trace=False)
    assert plan.random_barcode and key_words(eng) > 1
    S = n_samples_of(plan)
    before = [eng.render_wide_counts(s) for s in range(S)]
    rows, texts = check_engine(eng, c["scheme"], [list(range(S))])
    assert [texts[s] for s in range(S)] == before  # the same bytes before and after bc_engine_finish
    k = eng.counters()
    assert k["duplicates"] > 0 and sum(r[2] for r in rows) == k["matched"] and max(r[2] for r in rows) > 1
    assert eng.wide_render_sorts() == 1
    eng.close()


def test_sort_is_shared_until_the_counts_change():
    c = wk.CASES["samples_plus_raw_35"]
    plan, _, reads = wk._build("samples_plus_raw_35", 3000, 9)
    S = 5
    eng = _pkg().Engine(plan, device=0)
    submit(eng, reads[:1500])
    assert eng.wide_render_sorts() == 0 and eng.wide_render_sort_ms() == 0
    first = [eng.render_wide_counts(s) for s in range(S)] + [eng.render_wide_merged(range(S))]
    assert eng.wide_render_sorts() == 1 and all(first) and eng.wide_render_sort_ms() > 0
    rows = eng.result_rows()  # a finish in between costs no sort
    assert [eng.render_wide_counts(s) for s in range(S)] + [eng.render_wide_merged(range(S))] == first
    assert eng.wide_render_sorts() == 1
    assert first[0] == rrc.expected(plan, c["scheme"], rows, [0], False)
    submit(eng, reads[1500:])
    second = [eng.render_wide_counts(s) for s in range(S)] + [eng.render_wide_merged(range(S))]
    assert eng.wide_render_sorts() == 2
    rows = eng.result_rows()
    assert second[0] == rrc.expected(plan, c["scheme"], rows, [0], False) and second[0] != first[0]
    assert second[5] == rrc.expected(plan, c["scheme"], rows, range(S), True)
    eng.reset()
    assert eng.render_wide_counts(0) == b"" and eng.wide_render_sorts() == 3
    assert eng.raw_render_sorts() == 0
    eng.close()


def test_empty_engine_and_one_read():
    plan = _pkg().Plan(SEQ40["scheme"])
    eng = _pkg().Engine(plan, device=0)
    chunks = []
    assert eng.render_wide_counts(0, on_text=chunks.append) == 0 and not chunks
    assert eng.render_wide_merged([0]) == b"" and eng.render_wide_merged([]) == b""
    cap = "ACGTN" * 8
    submit(eng, ["TT" + "GTACCAGTC" + cap + "TGCATGGAC" + "A"])
    assert eng.render_wide_counts(0) == cap.encode() + b",1\n"
    assert eng.render_wide_merged([0, 0]) == cap.encode() + b",1,1\n"
    eng.close()


def test_failing_callback_leaves_the_engine_usable(monkeypatch):
    pkg = _pkg()
    d = random40()
    eng = d["eng"]
    monkeypatch.setenv("BC_RENDER_CHUNK_BYTES", "4096")
    import ctypes as C
    lib = pkg._lib.load()
    fail, go_on = pkg._lib.TEXT_FN(lambda t, k, u: 1), pkg._lib.TEXT_FN(lambda t, k, u: 0)
    n = C.c_uint64(7)
    rc = lib.bc_engine_render_wide_counts(eng._e, 0, fail, None, C.byref(n))
    assert rc == -5 and "callback" in pkg._lib.last_error(lib) and n.value == 0   # BC_ERR_STATE
    assert eng.render_wide_counts(0) == d["text"]                                 # the next render is whole
    assert lib.bc_engine_render_wide_counts(eng._e, 0, None, None, C.byref(n)) == -1      # null callback
    assert lib.bc_engine_render_wide_counts(eng._e, 1, go_on, None, C.byref(n)) == -1     # sample 1 of 1
    assert lib.bc_engine_render_wide_merged(eng._e, None, 2, go_on, None, C.byref(n)) == -1  # null list, two columns
    assert eng.render_wide_counts(0) == d["text"]


def test_refusals():
    pkg = _pkg()
    from test_gpu_raw_render import run
    dense = run(cases.build_case("del_exact", seed=3, n=300))
    narrow = run(cases.build_case("raw_counted", seed=29, n=300))
    raw_sample = run(cases.build_case("raw_sample", seed=3, n=300))
    wide_raw_sample = pkg.Engine(pkg.Plan(wk.CASES["samples_plus_raw_35"]["scheme"]), device=0)  # (no sample file)
    assert dense.plan.mode == "dense" and key_words(narrow) == 1 and key_words(wide_raw_sample) > 1
    for eng, word in ((dense, "bc_engine_render_counts"), (narrow, "bc_engine_render_raw_counts"),
                      (raw_sample, "bc_engine_row_text"), (wide_raw_sample, "bc_engine_row_text")):
        for call in (lambda: eng.render_wide_counts(0), lambda: eng.render_wide_merged([0])):
            with pytest.raises(pkg.BarcodeCountError) as ex:
                call()
            assert ex.value.code == -2 and word in str(ex.value)
        assert eng.wide_render_sorts() == 0
        eng.close()


def test_root_renders_the_job_after_finish_all(tmp_path):
    """2 ranks on one GPU over the message-file transport: the root's text equals the one-engine text of all reads"""
    name, n = "samples_plus_raw_35", 3000
    cdir = tmp_path / "comm"
    cdir.mkdir()
    out = tmp_path / "job.json"
    env = dict(os.environ, BC_COMM_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_rank_wide_render.py"), str(r), "2", str(cdir), str(n),
                               "0", str(out), name], env=env, stderr=subprocess.PIPE) for r in range(2)]
    for r, p in enumerate(procs):
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (r, err.decode()[-1500:])
    job = json.load(open(out))
    plan, _, reads = wk._build(name, n, 7)
    eng, _ = wk._run_engine(plan, reads, trace=False)
    for s in range(5):
        assert job["counts"][s].encode("latin-1") == eng.render_wide_counts(s), s
    assert job["merged"].encode("latin-1") == eng.render_wide_merged([4, 3, 2, 1, 0])
    assert job["sorts"] == 1 and len(job["merged"]) > 1000
    eng.close()
