"""Wide-key plans on the lane-per-read kernel (BC_WIDE_LANE=1; csrc/bc_lane.h process_read<.., kWide>, csrc/bc_long.h
wide_insert_lanes).  Every case with the generic kernel (BC_JIT=0) and the scheme-specialised one (BC_JIT=force), against
the CPU oracle: per-read outcomes, counters and every (sample, tuple, count) row -- and against the wave-per-read kernel
(switch 0) read by read through trace_idx, which is word 0 of the key: a fingerprint of every payload word.
tests/test_wide_lane_emulation.py runs the same schemes through the lane code on the host."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_wide_keys as twk
import wide_lane_cases as wlc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 104  # one batch shape for every lane batch of a scheme: one specialised kernel per scheme
JIT = ["0", "force"]
UNSUPPORTED = 7
CONTENTION_LIMIT_S = 180  # a contention submit in its child process: import, engine, one kernel compile, one launch


@pytest.fixture(autouse=True)
def _own_jit_cache(monkeypatch, tmp_path_factory):
    """the specialised kernels of this file go to the session's temporary cache, not next to the library"""
    monkeypatch.setenv("BC_JIT_CACHE", str(tmp_path_factory.getbasetemp() / "jit_cache"))


def _lane(monkeypatch, jit, switch="1"):
    monkeypatch.setenv("BC_WIDE_LANE", switch)
    monkeypatch.setenv("BC_JIT", jit)


def _is_lane_kernel(eng, jit):
    name = eng.kernel_name()
    return name.startswith("bc_jit_match_count<" if jit == "force" else "match_count_kernel<")


class Batch:
    """reads on the device, one stride, per-read lengths, with room for the trace"""

    def __init__(self, reads, stride=STRIDE, repeat=1):
        """repeat: the reads that many times over, one after the other"""
        import torch
        assert max(len(r) for r in reads) <= stride
        n = len(reads)
        seq = np.full((n, stride), ord("\n"), dtype=np.uint8)
        lens = np.zeros(n, dtype=np.uint16)
        for i, r in enumerate(reads):
            seq[i, :len(r)] = np.frombuffer(r.encode(), dtype=np.uint8)
            lens[i] = len(r)
        if repeat > 1:
            seq, lens, n = np.tile(seq, (repeat, 1)), np.tile(lens, repeat), n * repeat
        self.n, self.stride = n, stride
        self.dseq = torch.from_numpy(seq.reshape(-1)).cuda()
        self.dlens = torch.from_numpy(lens.view(np.int16)).cuda()
        self.d_out = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
        self.d_idx = torch.zeros(n, dtype=torch.int64, device="cuda")

    def submit(self, eng, cuts=None, trace=True):
        """cuts: read numbers (multiples of 8: batches start 16-byte aligned) at which a new submit begins"""
        cuts = [0] + list(cuts or []) + [self.n]
        for a, b in zip(cuts, cuts[1:]):
            if b > a:
                if trace:
                    eng.trace(self.d_out.data_ptr() + a, self.d_idx.data_ptr() + 8 * a)
                else:
                    eng.trace(None, None)  # (an earlier batch's buffers are not this one's size)
                eng.submit_device(self.dseq.data_ptr() + a * self.stride, None, b - a, self.stride, self.stride,
                                  d_lens=self.dlens.data_ptr() + 2 * a)
        eng.sync()
        return self.d_out.cpu().numpy(), self.d_idx.cpu().numpy().view(np.uint64)


def _engine(plan):
    import ngs_barcode_count_amd as pkg
    return pkg.Engine(plan, device=0)


def _same_outcomes(outcomes, o, reads):
    """per read, matched and duplicate are one outcome (which read of several with one key is the duplicate depends on
    the order they are counted in); the counters tell them apart"""
    exp = [twk.parity_code(o.process(r)) for r in reads]
    same = lambda a, b: a == b or {int(a), int(b)} == {0, 4}
    bad = [i for i in range(len(reads)) if not same(outcomes[i], exp[i])]
    assert not bad, (bad[:5], [(int(outcomes[i]), exp[i], reads[i]) for i in bad[:3]])


def _check_oracle(eng, o, n):
    got = eng.counters()
    assert {k: got[k] for k in o.counters} == o.counters
    assert got["total_reads"] == n
    assert eng.result_rows() == o.rows()


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("name", sorted(wlc.SCHEMES))
def test_schemes_vs_oracle(name, jit, monkeypatch):
    """6,000 reads with substitutions and 'N' in three submits into one table: later submits find the keys of earlier ones
    (for the random-barcode plans every key of the set is looked up again).  The table starts at 2^20 slots and is not
    rebuilt by 6,000 reads: test_lane_inserts_into_a_rehashed_table grows it"""
    _lane(monkeypatch, jit)
    n = 6000
    c, pools, reads = wlc.pools_and_reads(name, n, 7)
    plan, o = wlc.plan_of(c, pools), wlc.oracle_of(c, pools)
    assert plan.mode == "sparse"
    eng = _engine(plan)
    outcomes, _ = Batch(reads).submit(eng, cuts=[856, 3000])
    assert _is_lane_kernel(eng, jit), eng.kernel_name()
    assert eng.wide_lane_reads() == n
    _same_outcomes(outcomes, o, reads)
    _check_oracle(eng, o, n)
    if "random" in name:
        assert eng.counters()["duplicates"] > 100
    eng.close()


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("name", ["raw_28", "known_plus_random_30", "set_20_plus_random_32", "three_raw_20"])
def test_keys_are_bit_identical_across_the_two_kernels(name, jit, monkeypatch):
    """the same reads through a switch-0 engine (long_match_kernel) and a switch-1 engine: trace_idx -- word 0 of the key,
    the fingerprint of its payload -- read by read, and the rows"""
    c, pools, reads = wlc.pools_and_reads(name, 3000, 13)
    got = {}
    for switch in ("0", "1"):
        _lane(monkeypatch, jit, switch)
        eng = _engine(wlc.plan_of(c, pools))
        outcomes, idx = Batch(reads).submit(eng, cuts=[1000])
        assert (eng.kernel_name() == "long_match_kernel") if switch == "0" else _is_lane_kernel(eng, jit), eng.kernel_name()
        assert eng.wide_lane_reads() == (3000 if switch == "1" else 0)
        got[switch] = (outcomes, idx, eng.result_rows(), eng.counters())
        eng.close()
    counted = np.isin(got["0"][0], (0, 4))
    assert counted.sum() > 1000 and (got["0"][1][counted] != 0).all() and (got["0"][1][~counted] == 0).all()
    assert (got["0"][1] == got["1"][1]).all()
    assert (np.isin(got["1"][0], (0, 4)) == counted).all() and (got["0"][0][~counted] == got["1"][0][~counted]).all()
    assert got["0"][2] == got["1"][2] and got["0"][3] == got["1"][3]


def _contention_reads(with_random, n, keys):
    """clean reads of raw_32 (a raw 32-mer) or raw_plus_random_28 (a raw 24-mer and a 28-base random barcode), read i
    carrying key i % keys -- for the random-barcode plan the random barcode takes the key and the tuple is one"""
    rng = np.random.default_rng(keys)
    mers = lambda k, ln: ["".join(rng.choice(list("ACGT"), ln)) for _ in range(k)]
    if with_random:
        tup, rnd = mers(1, 24)[0], mers(keys, 28)
        assert len(set(rnd)) == keys
        return ["GA" + "CCTAGG" + tup + "AATT" + rnd[i % keys] + "GGATCC" + "T" for i in range(n)]
    caps = mers(keys, 32)
    assert len(set(caps)) == keys
    return ["GA" + "GTACCAGTC" + caps[i % keys] + "TGCATGGAC" + "T" for i in range(n)]


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("with_random", [False, True], ids=["counts", "random"])
@pytest.mark.parametrize("n,keys", [(64, 1), (4096, 3), (4096, 4096)], ids=["64x1", "4096x3", "4096_distinct"])
def test_contention_in_one_submit(n, keys, with_random, jit, monkeypatch, tmp_path):
    """one wavefront whose 64 lanes all carry one key; 4,096 reads over three keys; 4,096 distinct keys into a fresh
    table: one winner per key, everyone else finds it.  One submit each, in a child process of its own under a time
    limit: an insert that waited for a lane of its own wavefront would never end, so a child that runs out of time is
    killed, that is the finding, and the session ends there -- nothing more is started on a card with a kernel stuck."""
    _lane(monkeypatch, jit)
    out = tmp_path / "contention.json"
    cmd = [sys.executable, os.path.abspath(__file__), "contention", str(n), str(keys), str(int(with_random)), jit, str(out)]
    try:
        p = subprocess.run(cmd, stderr=subprocess.PIPE, timeout=CONTENTION_LIMIT_S)
    except subprocess.TimeoutExpired:
        pytest.exit("wide_insert_lanes: the contention submit (%d reads, %d keys, random=%s, BC_JIT=%s) did not end within "
                    "%d s and was killed -- a hang in the insert; no further GPU test is started"
                    % (n, keys, with_random, jit, CONTENTION_LIMIT_S), returncode=3)
    if p.returncode in (-6, -11, 134, 139):
        pytest.exit("the contention submit ended with status %d: no further GPU test is started\n%s"
                    % (p.returncode, p.stderr.decode(errors="replace")[-1500:]), returncode=3)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-1500:]
    got = json.load(open(out))
    reads = _contention_reads(with_random, n, keys)
    assert got["lane_kernel"] and got["wide_lane_reads"] == n, got["kernel"]
    counters, rows = got["counters"], [tuple(r) for r in got["rows"]]
    if with_random:
        assert (counters["matched"], counters["duplicates"]) == (keys, n - keys)
        assert rows == [("barcode", reads[0][8:32], keys)]
        assert got["distinct_idx"] == keys
    else:
        assert (counters["matched"], counters["duplicates"]) == (n, 0)
        per_key = {}
        for r in reads:
            per_key[r[11:43]] = per_key.get(r[11:43], 0) + 1
        assert rows == sorted(("barcode", k, v) for k, v in per_key.items())
    assert got["all_counted"]
    o = wlc.oracle_of(wlc.SCHEMES["raw_plus_random_28" if with_random else "raw_32"], [])
    for r in reads:
        o.process(r)
    assert {k: counters[k] for k in o.counters} == o.counters and counters["total_reads"] == n
    assert rows == o.rows()


def _contention_main():
    """the child of test_contention_in_one_submit: one engine, one submit, what came of it as JSON"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    n, keys, with_random, jit, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4] == "1", sys.argv[5], sys.argv[6]
    import torch  # noqa: F401 -- before the engine library (see tests/test_gpu_wide_keys.py)
    c = wlc.SCHEMES["raw_plus_random_28" if with_random else "raw_32"]
    eng = _engine(wlc.plan_of(c, []))
    outcomes, idx = Batch(_contention_reads(with_random, n, keys)).submit(eng)
    json.dump({"kernel": eng.kernel_name(), "lane_kernel": _is_lane_kernel(eng, jit), "wide_lane_reads": eng.wide_lane_reads(),
               "counters": eng.counters(), "rows": eng.result_rows(), "distinct_idx": len(set(idx.tolist())),
               "all_counted": bool(np.isin(outcomes, (0, 4)).all())}, open(out, "w"))
    eng.close()


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("name", ["raw_28", "known_plus_random_30"])
def test_lane_inserts_into_a_rehashed_table(name, jit, monkeypatch):
    """set_reserve keeps the table at most half full for every read submitted so far, starting at 2^20 slots: a second
    submit that takes the reads past 2^19 makes it allocate 2^21 slots and re-insert the published keys with
    wide_insert_kernel (payload, count and ready flag of every slot written anew) before the lane kernel runs.  Submit 1:
    4,096 reads; submit 2: the same reads 130 times over (532,480 reads, no new key: every insert is a find in the
    rebuilt table); submit 3: 2,048 other reads (finds and fresh claims in it)."""
    _lane(monkeypatch, jit)
    times = 130
    c, pools, first = wlc.pools_and_reads(name, 4096, 61)
    last = twk._reads(c["parts"], 2048, 62, pools)
    assert 4096 < 2 ** 19 < 4096 * (1 + times)
    eng = _engine(wlc.plan_of(c, pools))
    Batch(first).submit(eng)
    Batch(first, repeat=times).submit(eng, trace=False)
    outcomes, _ = Batch(last).submit(eng)
    n = 4096 * (1 + times) + 2048
    assert _is_lane_kernel(eng, jit) and eng.wide_lane_reads() == n
    o_first, o_all = wlc.oracle_of(c, pools), wlc.oracle_of(c, pools)
    for r in first:
        o_first.process(r)
        o_all.process(r)
    _same_outcomes(outcomes, o_all, last)
    a, b = o_first.counters, o_all.counters
    exp = {k: b[k] + times * a[k] for k in b}
    if "random" in name:  # a repeated read's key is in the set: every counted read of the repeats is a duplicate
        exp["matched"], exp["duplicates"] = b["matched"], b["duplicates"] + times * (a["matched"] + a["duplicates"])
        exp_rows = o_all.rows()
    else:
        once = {(s, t): k for s, t, k in o_first.rows()}
        exp_rows = sorted((s, t, k + times * once.get((s, t), 0)) for s, t, k in o_all.rows())
    got = eng.counters()
    assert {k: got[k] for k in exp} == exp and got["total_reads"] == n
    assert eng.result_rows() == exp_rows and len(exp_rows) >= 10
    eng.close()


@pytest.mark.parametrize("jit", ["cached"])
def test_precompiled_kernel_of_a_wide_plan_is_loaded(jit, monkeypatch, tmp_path):
    """bc_plan_precompile under the switch builds the object an engine of the plan then finds in the cache (BC_JIT=cached:
    cache hits only, nothing is compiled at run time)"""
    import ngs_barcode_count_amd as pkg
    monkeypatch.setenv("BC_WIDE_LANE", "1")
    monkeypatch.setenv("BC_JIT", jit)
    monkeypatch.setenv("BC_JIT_CACHE", str(tmp_path))
    c, pools, reads = wlc.pools_and_reads("raw_28", 1000, 71)
    plan = wlc.plan_of(c, pools)
    eng = _engine(plan)
    Batch(reads).submit(eng, trace=False)
    assert eng.kernel_name().startswith("match_count_kernel<")  # nothing in the cache yet: the generic kernel
    eng.close()
    pkg.precompile(plan, stride=STRIDE, read_len=STRIDE, lens=True, cache_dir=str(tmp_path))
    o = wlc.oracle_of(c, pools)
    for r in reads:
        o.process(r)
    eng = _engine(plan)
    Batch(reads).submit(eng, trace=False)
    assert eng.kernel_name().startswith("bc_jit_match_count<"), eng.kernel_name()
    _check_oracle(eng, o, 1000)
    eng.close()


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("n", [1, 63, 65, 127])
def test_partial_tiles(n, jit, monkeypatch):
    _lane(monkeypatch, jit)
    c, pools, reads = wlc.pools_and_reads("raw_plus_random_28", n, 17)
    o = wlc.oracle_of(c, pools)
    eng = _engine(wlc.plan_of(c, pools))
    outcomes, _ = Batch(reads).submit(eng)
    assert _is_lane_kernel(eng, jit) and eng.wide_lane_reads() == n
    _same_outcomes(outcomes, o, reads)
    _check_oracle(eng, o, n)
    eng.close()


@pytest.mark.parametrize("jit", JIT)
def test_raw_captures_that_hold_n_and_foreign_bytes(jit, monkeypatch):
    """a leading, a trailing and an all-'N' raw capture are keys like any other (the N plane; planes 1 and 2 clear under
    it); one byte outside ACGTN inside the raw capture or the random barcode makes the read unsupported, and the rows
    are those of the other reads"""
    _lane(monkeypatch, jit)
    c, pools, reads = wlc.pools_and_reads("raw_plus_random_28", 200, 19, p_sub=0.0, p_n=0.0, flank=(3, 3))
    cap, rnd = slice(3 + 6, 3 + 6 + 24), slice(3 + 6 + 24 + 4, 3 + 6 + 24 + 4 + 28)
    put = lambda r, sl, s: r[:sl.start] + s + r[sl.stop:]
    reads[10] = put(reads[10], cap, "N" + reads[10][cap][1:])
    reads[11] = put(reads[11], cap, reads[11][cap][:-1] + "N")
    reads[12] = put(reads[12], cap, "N" * 24)
    reads[13] = put(reads[13], cap, "N" * 24)  # (the same key, another random barcode)
    reads[14] = put(reads[14], rnd, "N" * 28)
    foreign = {20: put(reads[20], cap, reads[20][cap][:7] + "x" + reads[20][cap][8:]),
               21: put(reads[21], rnd, reads[21][rnd][:27] + "R"),
               22: put(reads[22], rnd, "-" + reads[22][rnd][1:])}
    for i, r in foreign.items():
        reads[i] = r
    o = wlc.oracle_of(c, pools)
    for i, r in enumerate(reads):
        if i not in foreign:
            assert o.process(r) in ("matched", "duplicates")
    eng = _engine(wlc.plan_of(c, pools))
    outcomes, idx = Batch(reads).submit(eng)
    assert _is_lane_kernel(eng, jit)
    assert [int(outcomes[i]) for i in sorted(foreign)] == [UNSUPPORTED] * 3 and (idx[sorted(foreign)] == 0).all()
    assert np.isin(np.delete(outcomes, sorted(foreign)), (0, 4)).all()
    rows = eng.result_rows()
    assert rows == o.rows()
    texts = {t for _, t, _ in rows}
    assert {"N" * 24, reads[10][cap], reads[11][cap]} <= texts
    got = eng.counters()
    assert {k: got[k] for k in o.counters} == o.counters and got["total_reads"] == 200
    eng.close()


@pytest.mark.parametrize("jit", JIT)
def test_discard_counts_plan(jit, monkeypatch):
    """a sample file but no sample group in the scheme: reads are matched, nothing is counted (info.rs:762-766)"""
    _lane(monkeypatch, jit)
    import ngs_barcode_count_amd as pkg
    import oracle_lib
    scheme = "GTACCAGTC{30}TGCATGGAC"
    parts = [("const", "GTACCAGTC"), ("cap", 30, 0), ("const", "TGCATGGAC")]
    rng = np.random.default_rng(23)
    reads = twk._reads(parts, 500, 23, [twk._pool(rng, 50, 30)])
    plan = pkg.Plan(scheme)
    plan.add_sample("ACGTACGT", "only")
    o = oracle_lib.Oracle(scheme, samples={"ACGTACGT": "only"})
    eng = _engine(plan)
    outcomes, _ = Batch(reads).submit(eng)
    assert _is_lane_kernel(eng, jit) and eng.wide_lane_reads() == 500
    _same_outcomes(outcomes, o, reads)
    _check_oracle(eng, o, 500)
    assert eng.result_rows() == [] and eng.counters()["matched"] > 300
    eng.close()


def _seam_batches(c, pools):
    a = wlc.twk._reads(c["parts"], 700, 31, pools)
    b = wlc.twk._reads(c["parts"], 300, 32, pools)
    rng = np.random.default_rng(33)
    b[150] = b[150] + "".join(rng.choice(list("ACGT"), 321 - len(b[150])))  # one read of 321 bases: the batch is the long kernel's
    d = wlc.twk._reads(c["parts"], 600, 34, pools)
    return [(a, 100), (b, 324), (d, 100)]


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("name", ["raw_28", "known_plus_random_30"])
def test_seam_between_the_two_kernels(name, jit, monkeypatch):
    """one engine, one table: a lane batch, a batch with a 321-base read (long_match_kernel), a lane batch again; then a
    reset in the middle of a second such job and the same reads once more"""
    _lane(monkeypatch, jit)
    c = wlc.SCHEMES[name]
    rng = np.random.default_rng(1031)
    pools = [twk._pool(rng, k, ln) for k, ln in c["pools"]]
    batches = [(Batch(r, s), r) for r, s in _seam_batches(c, pools)]
    o = wlc.oracle_of(c, pools)
    eng = _engine(wlc.plan_of(c, pools))
    kernels = []
    for b, reads in batches:
        outcomes, _ = b.submit(eng)
        kernels.append(eng.kernel_name())
        _same_outcomes(outcomes, o, reads)
    assert kernels[1] == "long_match_kernel" and kernels[0] == kernels[2] and _is_lane_kernel(eng, jit), kernels
    assert eng.wide_lane_reads() == 1300
    _check_oracle(eng, o, 1600)
    rows = eng.result_rows()
    # a second job on the engine, abandoned after its long batch; then the whole job again
    eng.reset()
    for b, _ in batches[:2]:
        b.submit(eng)
    eng.reset()
    assert eng.result_rows() == [] and sum(eng.counters().values()) == 0
    for b, _ in batches:
        b.submit(eng)
    assert eng.result_rows() == rows
    assert eng.wide_lane_reads() == 1300 + 700 + 1300
    eng.close()


@pytest.mark.parametrize("jit", JIT)
def test_render_wide_counts_after_a_lane_job(jit, monkeypatch):
    c, pools, reads = wlc.pools_and_reads("raw_22_21", 3000, 41)
    texts = {}
    for switch in ("0", "1"):
        _lane(monkeypatch, jit, switch)
        eng = _engine(wlc.plan_of(c, pools))
        Batch(reads).submit(eng, cuts=[1504])
        assert (eng.kernel_name() == "long_match_kernel") == (switch == "0")
        texts[switch] = eng.render_wide_counts(0)
        eng.close()
    assert texts["0"] == texts["1"] and texts["1"].count(b"\n") > 500


@pytest.mark.parametrize("jit", JIT)
@pytest.mark.parametrize("name", ["barcode_seq_40", "samples_plus_raw_35"])
def test_ineligible_plans_stay_on_the_wave_per_read_kernel(name, jit, monkeypatch):
    """a group above 32 bases: the switch changes nothing"""
    _lane(monkeypatch, jit)
    plan, o, reads = twk._build(name, 3000, 7)
    eng = _engine(plan)
    outcomes, _ = Batch(reads).submit(eng, cuts=[1000])
    assert eng.kernel_name() == "long_match_kernel" and eng.wide_lane_reads() == 0
    _same_outcomes(outcomes, o, reads)
    _check_oracle(eng, o, 3000)
    eng.close()


@pytest.mark.parametrize("jit", JIT)
def test_two_ranks_on_one_gpu(tmp_path, jit):
    """the job's end-of-run exchange after lane-path counting: every rank's (tuple, random) keys sent whole to the root's
    set (bc_engine_finish_all over the message-file transport)"""
    name, n, world = "known_plus_random_30", 6000, 2
    cdir = tmp_path / "comm"
    cdir.mkdir()
    out = tmp_path / "job.json"
    env = dict(os.environ, BC_COMM_TIMEOUT_S="120", BC_WIDE_LANE="1", BC_JIT=jit)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), name, str(r), str(world), str(cdir), str(n), str(out), jit],
                              stderr=subprocess.PIPE, env=env) for r in range(world)]
    for r, p in enumerate(procs):
        _, err = p.communicate(timeout=600)
        assert p.returncode == 0, (r, err.decode()[-1500:])
    job = json.load(open(out))
    c, pools, reads = wlc.pools_and_reads(name, n, 7)
    o = wlc.oracle_of(c, pools)
    for r in reads:
        o.process(r)
    assert {k: job["counters"][k] for k in o.counters} == o.counters
    assert [tuple(r) for r in job["rows"]] == o.rows()


def _rank_main():
    """one rank of test_two_ranks_on_one_gpu"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    name, rank, world, cdir, n, out, jit = (sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]),
                                            sys.argv[6], sys.argv[7])
    import torch  # noqa: F401 -- before the engine library (see tests/test_gpu_wide_keys.py)
    import ngs_barcode_count_amd as pkg
    c, pools, reads = wlc.pools_and_reads(name, n, 7)
    a, b = n * rank // world, n * (rank + 1) // world
    eng = _engine(wlc.plan_of(c, pools))
    Batch(reads[a:b]).submit(eng)
    assert _is_lane_kernel(eng, jit) and eng.wide_lane_reads() == b - a, eng.kernel_name()
    comm = pkg.Comm.host(cdir, rank, world)
    counters, n_rows = eng.finish_all(comm, 0)
    if rank == 0:
        rows = eng.result_rows()
        assert len(rows) == n_rows
        json.dump({"counters": counters, "rows": rows}, open(out, "w"))
    comm.barrier()
    comm.close()
    eng.close()


if __name__ == "__main__":
    _contention_main() if sys.argv[1] == "contention" else _rank_main()
