"""Log-mode counting (bc_fold.h): the match kernel writes one slot per read and the fold kernels apply the log to the
first-occurrence bit map + table.  Forced on (BC_COUNT_LOG=1) for small tables with the bit map forced too
(BC_BITMAP_MIN_ENTRIES=1), every counter and row must equal the oracle's, and at config 3's full size the table must
equal the atomic path's bit for bit.  Every test also asserts how many folds the engine ran (Engine.count_log_folds):
the atomic path gives the same answers, so only the count shows that the log path ran at all.  The fold kernels on their
own: tests/test_gpu_fold.py."""
import os
import subprocess
import sys

import pytest

import workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _submit(w, eng, first, n, chunk=1 << 20):
    import torch
    rl = w.read_len
    done = 0
    while done < n:
        m = min(chunk, n - done)
        dseq = torch.empty(m * rl, dtype=torch.uint8, device="cuda")
        dqual = torch.empty(m * rl, dtype=torch.uint8, device="cuda")
        w.synth.generate_device(0, None, first + done, m, dseq.data_ptr(), dqual.data_ptr())
        torch.cuda.synchronize()
        eng.submit_device(dseq.data_ptr(), dqual.data_ptr(), m, rl, rl)
        eng.sync()
        done += m


def _oracle(w, spans):
    o = workloads.oracle_for(w)
    for first, n in spans:
        seq, qual = w.synth.generate_host(first, n)
        o.process_batch(seq, qual if getattr(w, "min_quality", 1) > 0 else None, w.read_len, w.read_len)
    return o


def _check(eng, o):
    got = eng.counters()
    assert {k: got[k] for k in o.counters} == o.counters
    assert eng.result_rows() == o.rows()


@pytest.fixture
def log_on(monkeypatch):
    monkeypatch.setenv("BC_BITMAP_MIN_ENTRIES", "1")
    monkeypatch.setenv("BC_COUNT_LOG", "1")
    return monkeypatch


@pytest.mark.parametrize("n_sets", [(4, 30, 30, 30), (4, 200, 200, 200)])
def test_several_submits_with_a_sync_mid_job(log_on, n_sets):
    import ngs_barcode_count_amd as pkg
    w = workloads.make("config3", n_sets=n_sets)
    eng = pkg.Engine(w.plan, device=0)
    n = 120_000
    _submit(w, eng, 0, n // 2, chunk=n // 6)
    assert eng.counters()["total_reads"] == n // 2  # syncs: the bits so far are folded into the table
    _submit(w, eng, n // 2, n - n // 2, chunk=n // 5 + 3)
    _check(eng, _oracle(w, [(0, n)]))
    assert eng.count_log_folds() == 3 + 3  # one per submit
    eng.close()


def test_same_batch_twice_is_mostly_repeats(log_on):
    import ngs_barcode_count_amd as pkg
    w = workloads.make("config3", n_sets=(4, 200, 200, 200))
    eng = pkg.Engine(w.plan, device=0)
    n = 80_000
    _submit(w, eng, 0, n)
    _submit(w, eng, 0, n)
    _check(eng, _oracle(w, [(0, n), (0, n)]))
    assert eng.count_log_folds() == 2
    eng.close()


@pytest.mark.parametrize("n_sets", [(4, 3, 3, 3), (4, 12, 12, 12)])
def test_hot_tuples_and_an_oversized_bucket(log_on, n_sets):
    """a few hundred tuples, 700 k reads in one submit: one bucket holds every entry and is split over several apply
    items, which meet on the same bit-map words (and the hot-counter cache takes part of the adds)"""
    import ngs_barcode_count_amd as pkg
    w = workloads.make("config3", n_sets=n_sets)
    eng = pkg.Engine(w.plan, device=0)
    n = 700_000
    _submit(w, eng, 0, n, chunk=n)
    _submit(w, eng, n, n // 7, chunk=n)
    _check(eng, _oracle(w, [(0, n + n // 7)]))
    assert eng.count_log_folds() == 2
    eng.close()


def test_chunks_that_do_not_line_up(log_on):
    import ngs_barcode_count_amd as pkg
    log_chunk = 64 * 311
    log_on.setenv("BC_COUNT_LOG_CHUNK", str(log_chunk))
    w = workloads.make("config3", n_sets=(4, 60, 60, 60))
    eng = pkg.Engine(w.plan, device=0)
    n = 100_003
    _submit(w, eng, 0, n, chunk=50_001)
    _check(eng, _oracle(w, [(0, n)]))
    assert eng.count_log_folds() == sum(-(-m // log_chunk) for m in (50_001, 50_001, 1))
    eng.close()


def test_submits_either_side_of_the_threshold(monkeypatch):
    import ngs_barcode_count_amd as pkg
    monkeypatch.setenv("BC_BITMAP_MIN_ENTRIES", "1")
    monkeypatch.setenv("BC_COUNT_LOG", "auto")
    monkeypatch.setenv("BC_COUNT_LOG_MIN_READS", "20000")
    w = workloads.make("config3", n_sets=(4, 60, 60, 60))
    eng = pkg.Engine(w.plan, device=0)
    first = 0
    for m in (30_000, 5_000, 19_999, 20_000, 7_001, 44_444):
        _submit(w, eng, first, m, chunk=m)
        first += m
    _check(eng, _oracle(w, [(0, first)]))
    assert eng.count_log_folds() == 3  # the submits of 30000, 20000 and 44444 reads
    eng.close()


def test_submit_host(log_on):
    import ngs_barcode_count_amd as pkg
    w = workloads.make("config3", n_sets=(4, 40, 40, 40))
    n, R = 90_000, w.read_len
    seq, qual = w.synth.generate_host(0, n)
    eng = pkg.Engine(w.plan, device=0)
    eng.submit_host(seq, qual, R, R)
    _check(eng, _oracle(w, [(0, n)]))
    assert eng.count_log_folds() > 0
    eng.close()


def test_reset_results_between_jobs(log_on):
    """the bench's own pattern: job B after reset_results equals job B alone"""
    import ngs_barcode_count_amd as pkg
    w = workloads.make("config3", n_sets=(4, 60, 60, 60))
    eng = pkg.Engine(w.plan, device=0)
    _submit(w, eng, 0, 70_000)
    eng.sync()
    eng.reset_results()
    _submit(w, eng, 200_000, 60_000)
    assert eng.result_rows() == _oracle(w, [(200_000, 60_000)]).rows()
    assert eng.count_log_folds() == 2  # (reset_results keeps the count: it is the engine's, not the job's)
    eng.close()


def test_one_timing_entry_per_submit(log_on):
    import ngs_barcode_count_amd as pkg
    log_chunk = 64 * 100
    log_on.setenv("BC_COUNT_LOG_CHUNK", str(log_chunk))
    w = workloads.make("config3", n_sets=(4, 30, 30, 30))
    eng = pkg.Engine(w.plan, device=0)
    eng.timing(True)
    for k in range(3):
        _submit(w, eng, k * 20_000, 20_000, chunk=20_000)  # four chunks and folds each
    each = eng.kernel_ms_each()
    assert len(each) == 3 and all(x > 0 for x in each)
    assert "match_count" in eng.kernel_name()
    assert eng.count_log_folds() == 3 * -(-20_000 // log_chunk)
    eng.close()


def test_full_size_config3_log_equals_atomic(monkeypatch):
    """100 M config-3 reads into caller-owned tables: the atomic path, the log path, and the log path with chunk
    boundaries that line up with nothing give equal tables"""
    import torch
    import ngs_barcode_count_amd as pkg
    w = workloads.make("config3")
    entries = w.plan.table_entries
    n, piece, R = 100_000_000, 25_000_000, w.read_len
    modes = [("0", None), ("1", None), ("1", str(64 * 411_523))]
    tables = [torch.zeros(entries, dtype=torch.int32, device="cuda") for _ in modes]
    torch.cuda.synchronize()
    engs = []
    for (mode, chunk), t in zip(modes, tables):
        monkeypatch.setenv("BC_COUNT_LOG", mode)
        if chunk:
            monkeypatch.setenv("BC_COUNT_LOG_CHUNK", chunk)
        else:
            monkeypatch.delenv("BC_COUNT_LOG_CHUNK", raising=False)
        engs.append(pkg.Engine(w.plan, device=0, table_ptr=t.data_ptr()))
    dseq = torch.empty(piece * R, dtype=torch.uint8, device="cuda")
    dqual = torch.empty(piece * R, dtype=torch.uint8, device="cuda")
    for first in range(0, n, piece):
        w.synth.generate_device(0, None, first, piece, dseq.data_ptr(), dqual.data_ptr())
        torch.cuda.synchronize()
        for e in engs:
            e.submit_device(dseq.data_ptr(), dqual.data_ptr(), piece, R, R)
            e.sync()
    counters = [e.counters() for e in engs]
    assert counters[0] == counters[1] == counters[2]
    assert counters[0]["total_reads"] == n
    assert int(tables[0].sum(dtype=torch.int64)) == counters[0]["matched"]
    assert torch.equal(tables[0], tables[1])
    assert torch.equal(tables[0], tables[2])
    # one fold per submit: each 25 M-read piece fits one log chunk (2^27 reads, and 64 * 411523)
    assert [e.count_log_folds() for e in engs] == [0, n // piece, n // piece]
    for e in engs:
        e.close()


def _multirank(tmp_path, case, world, n, root):
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mp_rank
    cdir = tmp_path / "comm"
    cdir.mkdir()
    out = tmp_path / "job.json"
    env = dict(os.environ, BC_COMM_TIMEOUT_S="120", BC_COMM_VERBOSE="1", BC_BITMAP_MIN_ENTRIES="1", BC_COUNT_LOG="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_rank.py"), case, str(r), str(world), str(cdir),
                               str(n), str(root), str(out)], env=env, stderr=subprocess.PIPE) for r in range(world)]
    errs = []
    for r, p in enumerate(procs):
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (r, err.decode()[-1500:])
        errs.append(err.decode())
    job = json.load(open(out))
    w = mp_rank.make_case(case)
    o = _oracle(w, [(0, n)])
    assert {k: job["counters"][k] for k in o.counters} == o.counters
    assert [tuple(r) for r in job["rows"]] == o.rows()
    assert job["log_folds"] == 1  # the root's one submit went through the log
    return job, errs[root]


def test_multirank_exchange_with_log_mode(tmp_path):
    """one case of test_gpu_multirank.py with the log path forced on in every rank"""
    _multirank(tmp_path, "dense", 2, 60_001, 1)


@pytest.mark.parametrize("case,world,n,root", [("dense_hot", 3, 50_000, 0), ("dense_big", 3, 90_000, 2)])
def test_multirank_exchange_with_log_mode_more_tables(tmp_path, case, world, n, root):
    """counts above 255 (dense_hot: the exchange's overflow side list) and a table sparse enough for the bit-map form
    of the exchange (dense_big), both counted through the log in every rank"""
    job, err = _multirank(tmp_path, case, world, n, root)
    if case == "dense_hot":
        assert max(r[2] for r in job["rows"]) > 255 * world
    else:
        assert "bit-map slices" in err and "two bit planes" in err, err[-400:]


# ---------------------------------------------------------------------------------------------------------------------
# the other workloads in log mode: each against the oracle, with the fold count asserted

@pytest.mark.parametrize("name,n_sets,zipf,n", [("config2", (4, 60, 60, 60), False, 150_000),
                                                ("config5", (20_000,), False, 60_000),
                                                ("config5", (20_000,), True, 60_000)])
def test_workloads_in_log_mode(log_on, name, n_sets, zipf, n):
    """config 2 (exact matching), config 5 uniform and Zipf (the deferred search queue adds to the table directly while
    the launch's other reads go through the log)"""
    import ngs_barcode_count_amd as pkg
    w = workloads.make(name, n_sets=n_sets, zipf=zipf)
    eng = pkg.Engine(w.plan, device=0)
    _submit(w, eng, 0, n, chunk=n // 2)
    _check(eng, _oracle(w, [(0, n)]))
    assert eng.count_log_folds() == 2
    eng.close()


def test_config3_specialised_kernel_log_store(log_on):
    """the scheme-specialised (JIT) kernel's log store below 2^20 reads, where it only runs when forced"""
    import ngs_barcode_count_amd as pkg
    log_on.setenv("BC_JIT", "force")
    w = workloads.make("config3", n_sets=(4, 60, 60, 60))
    eng = pkg.Engine(w.plan, device=0)
    n = 120_000
    _submit(w, eng, 0, n, chunk=n // 3)
    assert eng.kernel_name().startswith("bc_jit_match_count"), eng.kernel_name()
    _check(eng, _oracle(w, [(0, n)]))
    assert eng.count_log_folds() == 3
    eng.close()


@pytest.mark.parametrize("name,n_sets,zipf,n", [("config3", (4, 12, 12, 12), False, 300_000),
                                                ("config5", (20_000,), True, 60_000)])
def test_hot_counter_cache_in_log_mode(log_on, name, n_sets, zipf, n):
    """BC_COUNT_LOG_HOT=1: the hot-counter cache takes part of the adds while the rest go through the log"""
    import ngs_barcode_count_amd as pkg
    log_on.setenv("BC_COUNT_LOG_HOT", "1")
    w = workloads.make(name, n_sets=n_sets, zipf=zipf)
    eng = pkg.Engine(w.plan, device=0)
    _submit(w, eng, 0, n, chunk=n)
    _check(eng, _oracle(w, [(0, n)]))
    assert eng.count_log_folds() == 1
    eng.close()
