"""Log-mode counting (bc_fold.h): the match kernel writes one slot per read and the fold kernels apply the log to the
first-occurrence bit map + table.  Forced on (BC_COUNT_LOG=1) for small tables with the bit map forced too
(BC_BITMAP_MIN_ENTRIES=1), every counter and row must equal the oracle's, and at config 3's full size the table must
equal the atomic path's bit for bit."""
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
    eng.close()


def test_same_batch_twice_is_mostly_repeats(log_on):
    import ngs_barcode_count_amd as pkg
    w = workloads.make("config3", n_sets=(4, 200, 200, 200))
    eng = pkg.Engine(w.plan, device=0)
    n = 80_000
    _submit(w, eng, 0, n)
    _submit(w, eng, 0, n)
    _check(eng, _oracle(w, [(0, n), (0, n)]))
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
    eng.close()


def test_chunks_that_do_not_line_up(log_on):
    import ngs_barcode_count_amd as pkg
    log_on.setenv("BC_COUNT_LOG_CHUNK", str(64 * 311))
    w = workloads.make("config3", n_sets=(4, 60, 60, 60))
    eng = pkg.Engine(w.plan, device=0)
    n = 100_003
    _submit(w, eng, 0, n, chunk=50_001)
    _check(eng, _oracle(w, [(0, n)]))
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
    eng.close()


def test_submit_host(log_on):
    import ngs_barcode_count_amd as pkg
    w = workloads.make("config3", n_sets=(4, 40, 40, 40))
    n, R = 90_000, w.read_len
    seq, qual = w.synth.generate_host(0, n)
    eng = pkg.Engine(w.plan, device=0)
    eng.submit_host(seq, qual, R, R)
    _check(eng, _oracle(w, [(0, n)]))
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
    eng.close()


def test_one_timing_entry_per_submit(log_on):
    import ngs_barcode_count_amd as pkg
    log_on.setenv("BC_COUNT_LOG_CHUNK", str(64 * 100))
    w = workloads.make("config3", n_sets=(4, 30, 30, 30))
    eng = pkg.Engine(w.plan, device=0)
    eng.timing(True)
    for k in range(3):
        _submit(w, eng, k * 20_000, 20_000, chunk=20_000)  # three chunks and folds each
    each = eng.kernel_ms_each()
    assert len(each) == 3 and all(x > 0 for x in each)
    assert "match_count" in eng.kernel_name()
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
    for e in engs:
        e.close()


def test_multirank_exchange_with_log_mode(tmp_path):
    """one case of test_gpu_multirank.py with the log path forced on in every rank"""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mp_rank
    case, world, n, root = "dense", 2, 60_001, 1
    cdir = tmp_path / "comm"
    cdir.mkdir()
    out = tmp_path / "job.json"
    env = dict(os.environ, BC_COMM_TIMEOUT_S="120", BC_BITMAP_MIN_ENTRIES="1", BC_COUNT_LOG="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mp_rank.py"), case, str(r), str(world), str(cdir),
                               str(n), str(root), str(out)], env=env, stderr=subprocess.PIPE) for r in range(world)]
    for r, p in enumerate(procs):
        _, err = p.communicate(timeout=300)
        assert p.returncode == 0, (r, err.decode()[-1500:])
    job = json.load(open(out))
    w = mp_rank.make_case(case)
    o = _oracle(w, [(0, n)])
    assert {k: job["counters"][k] for k in o.counters} == o.counters
    assert [tuple(r) for r in job["rows"]] == o.rows()
