"""bench.py --dump-outputs: the files hold what the timed path computed in its LAST step -- the outcome counters and the
rows of the reads that step counted -- and equal the CPU oracle over exactly those reads of the seeded stream, so
that two builds of the project can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("config,world", [("config3", 1), ("config4", 1), ("config3", 2)])
def test_dump_outputs_are_the_last_steps_results(tmp_path, config, world):
    import ngs_barcode_count_amd as pkg
    import parity
    import workloads
    reads, steps = 150_000, 3
    out = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--config", config, "--reads", str(reads),
           "--steps", str(steps), "--warmup", "1", "--no-extra", "--no-cpu", "--dump-outputs", str(out)]
    if world > 1:
        cmd.append("--selftest-one-gpu")  # (both ranks on this box's one GPU: the N > 1 path and its exchange)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert line["steps"] == steps and line["outcomes"]["total_reads"] == steps * reads * world
    got = {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert sorted(got) == ["outcome_counters", "rows_count", "rows_key", "rows_total"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the last step of rank r counted batch steps - 1 of its shard (bench.py: shard(reads * steps * world))
    w = workloads.make(config, geo_total=reads * world) if config == "config4" else workloads.make(config)
    o = workloads.oracle_for(w)
    for r in range(world):
        seq, qual = w.synth.generate_host((r * steps + steps - 1) * reads, reads)
        o.process_batch(seq, qual if w.min_quality > 0 else None, w.read_len, w.read_len)
    exp = [o.counters[k] for k in pkg.COUNTER_NAMES[:6]] + [reads * world, 0]
    assert got["outcome_counters"].tolist() == exp
    rows = o.rows()
    assert got["rows_total"].tolist() == [len(rows), sum(c for _, _, c in rows)]
    # (fewer rows than the sample's size: every row is in the files)
    keys = got["rows_key"].astype(np.uint64)
    assert np.all(np.diff(keys.astype(np.int64)) > 0)
    assert parity.decode_rows(w.plan, dict(zip(keys.tolist(), got["rows_count"].astype(np.int64).tolist())), False) == rows
