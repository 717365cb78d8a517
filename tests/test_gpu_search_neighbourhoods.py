"""The barcode search over whole mismatch neighbourhoods, device half (tests/search_cases.py has the inputs; the host
half, tests/test_search_neighbourhoods.py, checks the brute force against the oracle and the lane code against it).

Every configuration sits on one layer of the search stack of bc_kernel.h -- direct table, plain scan, tier, coarse,
middle and full index, the search queue, the batched coarse probe of multi-group plans -- and its captures are the
complete mismatch neighbourhoods of chosen centre references: every mismatch position, block boundaries and the bases
no block covers included, against sets with buckets of 5 to 257 references and tie partners behind the bucket heads.
One traced submit per test; every read's outcome and dense index against the numpy brute force, then the six counters
and the result rows against the C oracle.  Two arrangements of the same reads: packed (all 64 lanes of a wavefront
search) and sparse (1, 2, 3, 5 ... 33 searching lanes among exact reads: groups of four with every remainder, and more
than the queue's 16 entries).

This proves the search over complete neighbourhoods of the chosen centres, not over every capture of the space."""
import functools

import numpy as np
import pytest

import emu_lib
import search_cases as sc
from test_gpu_parity import make_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=list(sc.CONFIGS))
def cfg(request):
    """(module scope: pytest runs the tests configuration by configuration, so each is built once)"""
    c = sc.build(request.param)
    got = sc.floors(c.brute, c.captures, c.budget)
    assert min(got.values()) >= sc.FLOOR, got  # from the brute force alone, before the kernel's answers are looked at
    sc.check_layout(c, emu_lib.group_layout(emu_lib.make_plan(c.case)))  # the layer the configuration is there for
    return c


@functools.lru_cache(maxsize=4)
def _oracle(name, kind):
    c = sc.build(name)
    return sc.oracle_run(c, sc.arrangement(c, kind), threads=8)


def _run(c, kind, kernel, monkeypatch, tmp_path_factory, log=False):
    import torch
    import ngs_barcode_count_amd as pkg
    monkeypatch.setenv("BC_JIT", "force" if kernel == "specialised" else "0")
    monkeypatch.setenv("BC_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit_cache"))
    a = sc.arrangement(c, kind)
    n = len(a.seq)
    plan = make_plan(c.case)
    dseq = torch.from_numpy(a.seq.reshape(-1)).cuda()
    outc = torch.zeros(n, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng = pkg.Engine(plan, device=0)
    try:
        eng.trace(outc.data_ptr(), idx.data_ptr())
        eng.submit_device(dseq.data_ptr(), None, n, a.stride, a.stride, None)
        eng.sync()
        name = eng.kernel_name()
        assert name.startswith("bc_jit_match_count" if kernel == "specialised" else "match_count_kernel"), name
        outcomes, index = outc.cpu().numpy(), idx.cpu().numpy()
        # every read against the brute force
        bad = np.flatnonzero((outcomes != a.outcome) | ((a.outcome == 0) & (index != a.index)))
        assert len(bad) == 0, (len(bad), int(bad[0]), a.seq[bad[0]].tobytes(), int(outcomes[bad[0]]), int(a.outcome[bad[0]]),
                               int(index[bad[0]]), int(a.index[bad[0]]))
        # counters and rows against the oracle
        o_outcomes, o_counters, o_rows = _oracle(c.name, kind)
        assert (o_outcomes == a.outcome).all()
        got = eng.counters()
        assert {k: got[k] for k in o_counters} == o_counters
        assert got["total_reads"] == n and got["unsupported_reads"] == 0
        assert eng.result_rows() == o_rows
        assert eng.count_log_folds() == (1 if log else 0)
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["packed", "sparse"])
def test_generic_kernel(cfg, kind, monkeypatch, tmp_path_factory):
    _run(cfg, kind, "generic", monkeypatch, tmp_path_factory)


@pytest.mark.parametrize("kind", ["packed", "sparse"])
@pytest.mark.parametrize("cfg", sc.SPECIALISED, indirect=True)
def test_specialised_kernel(cfg, kind, monkeypatch, tmp_path_factory):
    _run(cfg, kind, "specialised", monkeypatch, tmp_path_factory)


@pytest.mark.parametrize("kind", ["packed", "sparse"])
@pytest.mark.parametrize("cfg", ["h20b3"], indirect=True)
def test_queued_verdicts_count_beside_the_log(cfg, kind, monkeypatch, tmp_path_factory):
    """the one-group plan with a search queue, counting through the log: the verdicts that come out of the queue are
    counted beside it"""
    monkeypatch.setenv("BC_BITMAP_MIN_ENTRIES", "1")
    monkeypatch.setenv("BC_COUNT_LOG", "1")
    _run(cfg, kind, "generic", monkeypatch, tmp_path_factory, log=True)
