"""A reset that is owed (bc_engine.hip: bc_engine::owed_*).  bc_engine_reset / bc_engine_reset_results zero nothing at
once: the next path that touches table, dirty map or bit map settles the debt first, except a log-mode submit, which
runs the table's part beside its match kernel (BC_COUNT_LOG_DEFER_RESET) and folds onto a bit map nobody zeroed
(BC_COUNT_LOG_FRESH; the fold on its own: tests/test_gpu_fold_fresh.py).  Every order in which an owed reset can meet
a consumer is run here, with each switch on and off, and compared with the atomic path (BC_COUNT_LOG=0) and the CPU
oracle; Engine.count_log_folds shows that the log path really ran."""
import pytest

import test_gpu_count_log as cl
import workloads

pytestmark = pytest.mark.gpu

SWITCHES = [{}, {"BC_COUNT_LOG_DEFER_RESET": "0"}, {"BC_COUNT_LOG_FRESH": "0"},
            {"BC_COUNT_LOG_DEFER_RESET": "0", "BC_COUNT_LOG_FRESH": "0"}]
IDS = ["default", "no-defer", "no-fresh", "neither"]
SMALL = (4, 60, 60, 60)


@pytest.fixture(params=SWITCHES, ids=IDS)
def log_on(request, monkeypatch):
    monkeypatch.setenv("BC_BITMAP_MIN_ENTRIES", "1")
    monkeypatch.setenv("BC_COUNT_LOG", "1")
    for k, v in request.param.items():
        monkeypatch.setenv(k, v)
    return monkeypatch


def _engine(w, env=None, **kw):
    """an engine created under `env` (the switches are read at creation), the environment put back afterwards"""
    import os
    import ngs_barcode_count_amd as pkg
    old = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    try:
        return pkg.Engine(w.plan, device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _atomic(w, spans, chunk=1 << 20):
    """counters and rows of `spans` alone on the atomic path"""
    eng = _engine(w, {"BC_COUNT_LOG": "0"})
    for first, n in spans:
        cl._submit(w, eng, first, n, chunk=chunk)
    out = eng.counters(), eng.result_rows()
    assert eng.count_log_folds() == 0
    eng.close()
    return out


def _check_job(w, eng, spans):
    """rows of `spans` (the job since the last reset) against oracle and atomic path; the counters of both agree"""
    o = cl._oracle(w, spans)
    a_counters, a_rows = _atomic(w, spans)
    assert {k: a_counters[k] for k in o.counters} == o.counters
    rows = eng.result_rows()
    assert rows == o.rows()
    assert rows == a_rows
    return o


@pytest.mark.parametrize("full", [False, True])
def test_reset_then_log_submit(log_on, full):
    w = workloads.make("config3", n_sets=SMALL)
    eng = _engine(w)
    cl._submit(w, eng, 0, 70_000, chunk=70_000)
    first = eng.counters()
    eng.reset() if full else eng.reset_results()
    cl._submit(w, eng, 200_000, 60_000, chunk=60_000)
    o = _check_job(w, eng, [(200_000, 60_000)])
    got = eng.counters()
    for k, v in o.counters.items():  # (reset_results lets the outcome counters run on)
        assert got[k] == v + (0 if full else first[k])
    assert eng.count_log_folds() == 2
    eng.close()


def test_reset_then_atomic_submit(log_on):
    log_on.setenv("BC_COUNT_LOG", "auto")
    log_on.setenv("BC_COUNT_LOG_MIN_READS", "50000")
    w = workloads.make("config3", n_sets=SMALL)
    eng = _engine(w)
    cl._submit(w, eng, 0, 60_000, chunk=60_000)
    eng.reset_results()
    cl._submit(w, eng, 100_000, 20_000, chunk=20_000)  # below the threshold: per-read atomics on bit map and table
    _check_job(w, eng, [(100_000, 20_000)])
    assert eng.count_log_folds() == 1
    eng.reset_results()
    cl._submit(w, eng, 300_000, 55_000, chunk=55_000)  # and a log job after an atomic one
    _check_job(w, eng, [(300_000, 55_000)])
    assert eng.count_log_folds() == 2
    eng.close()


def test_reset_twice_then_submit(log_on):
    w = workloads.make("config3", n_sets=SMALL)
    eng = _engine(w)
    cl._submit(w, eng, 0, 70_000, chunk=35_000)
    eng.reset_results()
    eng.reset()
    cl._submit(w, eng, 500_000, 40_000, chunk=40_000)
    o = _check_job(w, eng, [(500_000, 40_000)])
    got = eng.counters()
    assert {k: got[k] for k in o.counters} == o.counters
    assert eng.count_log_folds() == 3
    eng.close()


def test_reset_then_readers(log_on):
    """finish, nonzero_entries, table_ptr and the counters right after a reset: an empty Results"""
    import torch
    w = workloads.make("config3", n_sets=SMALL)
    eng = _engine(w)
    for reader in ("finish", "nonzero_entries", "table_ptr", "counters"):
        cl._submit(w, eng, 0, 50_000, chunk=50_000)
        eng.reset()
        if reader == "finish":
            assert eng.result_rows() == []
        elif reader == "nonzero_entries":
            assert eng.nonzero_entries() == 0
        elif reader == "table_ptr":
            ptr = eng.table_ptr  # (from here on the table counts as handed out: resets zero it at once)
            torch.cuda.synchronize()

            class Table:
                __cuda_array_interface__ = {"shape": (w.plan.table_entries,), "typestr": "<i4", "data": (ptr, False), "version": 2}

            assert int(torch.as_tensor(Table(), device="cuda").count_nonzero()) == 0
        else:
            assert not any(eng.counters().values())
        assert eng.result_rows() == []
    cl._submit(w, eng, 100_000, 50_000, chunk=50_000)
    _check_job(w, eng, [(100_000, 50_000)])
    assert eng.count_log_folds() == 5
    eng.close()


def test_reset_then_close(log_on):
    w = workloads.make("config3", n_sets=SMALL)
    eng = _engine(w)
    cl._submit(w, eng, 0, 50_000, chunk=50_000)
    eng.reset_results()
    eng.close()
    eng = _engine(w)  # and one that never ran anything
    eng.reset()
    eng.close()
    eng = _engine(w)
    cl._submit(w, eng, 0, 30_000, chunk=30_000)
    _check_job(w, eng, [(0, 30_000)])
    eng.close()


def test_finish_between_jobs(log_on):
    """rows read while the bits are still apart from the table, then the next job on top of an owed reset"""
    w = workloads.make("config3", n_sets=SMALL)
    eng = _engine(w)
    cl._submit(w, eng, 0, 60_000, chunk=60_000)
    _check_job(w, eng, [(0, 60_000)])
    eng.reset_results()
    cl._submit(w, eng, 60_000, 60_000, chunk=60_000)
    cl._submit(w, eng, 0, 30_000, chunk=30_000)  # (a second submit of the job: an ordinary fold onto the first one's bits)
    _check_job(w, eng, [(60_000, 60_000), (0, 30_000)])
    assert eng.count_log_folds() == 3
    eng.close()


def test_caller_owned_table(log_on):
    import torch
    w = workloads.make("config3", n_sets=SMALL)
    tables = [torch.zeros(w.plan.table_entries, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    eng = _engine(w, table_ptr=tables[0].data_ptr())
    ref = _engine(w, {"BC_COUNT_LOG": "0"}, table_ptr=tables[1].data_ptr())
    for e in (eng, ref):
        cl._submit(w, e, 0, 70_000, chunk=70_000)
    assert torch.equal(tables[0], tables[1]) and int(tables[0].sum()) == eng.counters()["matched"]
    for e in (eng, ref):
        e.reset_results()
        e.sync()
    assert int(tables[0].count_nonzero()) == 0  # reset(); sync() means what it did
    for e in (eng, ref):
        e.reset_results()  # (twice in a row, and then straight into a job)
        cl._submit(w, e, 200_000, 60_000, chunk=60_000)
    assert torch.equal(tables[0], tables[1])
    o = cl._oracle(w, [(200_000, 60_000)])
    assert int(tables[0].sum()) == o.counters["matched"]
    assert eng.result_rows() == o.rows()
    assert (eng.count_log_folds(), ref.count_log_folds()) == (2, 0)
    eng.close()
    ref.close()


def test_multi_chunk_submit_after_reset(log_on):
    log_chunk = 64 * 311
    log_on.setenv("BC_COUNT_LOG_CHUNK", str(log_chunk))
    w = workloads.make("config3", n_sets=SMALL)
    eng = _engine(w)
    cl._submit(w, eng, 0, 50_000, chunk=50_000)
    eng.reset_results()
    n = 100_003
    cl._submit(w, eng, 150_000, n, chunk=n)  # one submit: the first chunk's fold is the fresh one, five ordinary ones follow
    _check_job(w, eng, [(150_000, n)])
    assert eng.count_log_folds() == -(-50_000 // log_chunk) + -(-n // log_chunk)
    eng.close()


@pytest.mark.parametrize("name,n_sets,hot", [("config3", (4, 12, 12, 12), True), ("config5", (20_000,), False)])
def test_kernels_that_write_the_table_settle_first(log_on, name, n_sets, hot):
    """the hot-counter cache's flush and config 5's search queue add to the table from inside the log-mode match kernel:
    the reset may not run beside them"""
    if hot:
        log_on.setenv("BC_COUNT_LOG_HOT", "1")
    w = workloads.make(name, n_sets=n_sets)
    eng = _engine(w)
    cl._submit(w, eng, 0, 80_000, chunk=80_000)
    eng.reset_results()
    cl._submit(w, eng, 80_000, 60_000, chunk=60_000)
    _check_job(w, eng, [(80_000, 60_000)])
    assert eng.count_log_folds() == 2
    eng.close()


def test_job_two_empties_buckets_and_splits_one(log_on):
    """Eight fold buckets.  Job 1 fills buckets 0, 2, 3, 5 and 7; after reset_results job 2 puts more than kFoldChunk
    entries into bucket 1 (split over several apply items, on a map nobody zeroed) and some into bucket 6, and leaves the
    others empty: none of job 1's bits or counts may survive."""
    import numpy as np
    import torch
    import test_gpu_fold as tg
    k = tg.K()
    w = workloads.make("config3", n_sets=(4, 200, 200, 200))
    assert -(-w.plan.table_entries >> k["bucket_shift"]) == 8
    R, pool = w.read_len, 1_500_000
    dseq = torch.empty(pool * R, dtype=torch.uint8, device="cuda")
    dqual = torch.empty(pool * R, dtype=torch.uint8, device="cuda")
    w.synth.generate_device(0, None, 0, pool, dseq.data_ptr(), dqual.data_ptr())
    outcome = torch.full((pool,), 255, dtype=torch.uint8, device="cuda")
    index = torch.zeros(pool, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    tracer = _engine(w, {"BC_COUNT_LOG": "0"})
    tracer.trace(outcome.data_ptr(), index.data_ptr())
    tracer.submit_device(dseq.data_ptr(), dqual.data_ptr(), pool, R, R)
    tracer.sync()
    tracer.close()
    bucket = torch.where(outcome == 0, index >> k["bucket_shift"], torch.full_like(index, -1))  # -1: not counted
    in_b = lambda *bs: torch.nonzero(sum(bucket == b for b in bs)).flatten()
    one = in_b(1)
    reps = -(-(k["chunk"] + 50_000) // one.numel())
    sel1 = torch.cat([in_b(0, 2, 3, 5, 7), in_b(-1)[:20_000]])
    sel2 = torch.cat([one.repeat(reps), in_b(6), in_b(-1)[20_000:30_000]])
    sel2 = sel2[torch.randperm(sel2.numel(), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))]
    assert one.numel() * reps > k["chunk"] and in_b(6).numel() > 0 and min(in_b(b).numel() for b in (0, 2, 3, 5, 7)) > 1000
    jobs = []
    for sel in (sel1, sel2):
        rows = sel[:, None] * R + torch.arange(R, device="cuda")[None, :]
        jobs.append((dseq[rows].contiguous(), dqual[rows].contiguous(), sel.numel()))
    torch.cuda.synchronize()
    eng, ref = _engine(w), _engine(w, {"BC_COUNT_LOG": "0"})
    for j, (s, q, n) in enumerate(jobs):
        for e in (eng, ref):
            if j:
                e.reset_results()
            e.submit_device(s.data_ptr(), q.data_ptr(), n, R, R)
            e.sync()
    o = workloads.oracle_for(w)
    o.process_batch(jobs[1][0].cpu().numpy(), jobs[1][1].cpu().numpy(), R, R)
    rows = eng.result_rows()
    assert rows == ref.result_rows()
    assert rows == o.rows()
    assert (eng.count_log_folds(), ref.count_log_folds()) == (2, 0)
    a, b = eng.counters(), ref.counters()
    assert a == b
    eng.close()
    ref.close()
