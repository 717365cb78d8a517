"""bench.py: a plain run does only what its headline needs -- set-up, warm-up, the timed steps and the one JSON line --;
--full adds what takes runs of its own (rows in the table at the end, the box's ceilings, the CPU baseline, and the
legs beside the headline after the line)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("table_rows_at_end", "table_entries", "box", "cpu_baseline")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "config3",
                        "--reads", "200000", "--steps", "2", "--warmup", "1"] + args,
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    extra = [l[len("BENCH_EXTRA "):] for l in p.stderr.splitlines() if l.startswith("BENCH_EXTRA ")]
    return json.loads(lines[0]), [json.loads(e) for e in extra]


def test_plain_run_is_the_headline_alone():
    line, extra = _bench([])
    assert all(k in line for k in CONTRACT)
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert line["outcomes"]["total_reads"] == 2 * 200_000
    assert line["roofline"]["launches"] > 0  # (HIP events of the timed steps themselves: no run of its own)
    assert not [k for k in FULL_ONLY if k in line]
    assert "box_copy_GBps" not in line["roofline"]
    assert extra == []


def test_full_adds_the_measurements_beside_the_headline():
    plain, _ = _bench([])
    line, extra = _bench(["--full", "--cpu-sample", "20000"])
    assert all(k in line for k in CONTRACT)
    assert line["outcomes"] == plain["outcomes"]  # the same reads through the same timed steps
    assert 0 < line["table_rows_at_end"] <= line["outcomes"]["matched"]
    assert line["box"]["copy_GBps"] > 0 and line["box"]["atomic_Gps"] > 0
    assert line["roofline"]["box_copy_GBps"] == line["box"]["copy_GBps"]
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["independent_contexts"]["value"] > 0
    assert len(extra) == 1
    ex = extra[0]
    assert ex["of"] == {"config": "config3", "steps": 2, "warmup": 1}
    for k in ("finish", "end_to_end", "ingest"):
        assert "error" not in ex[k], (k, ex[k])
    assert ex["finish"]["finish_rows"] == line["table_rows_at_end"]
    assert [e.get("config") for e in ex["extra"]] == ["config2", "config4", "config5", "config5z"]
    assert all("error" not in e and e["value"] > 0 for e in ex["extra"]), ex["extra"]

    # --no-cpu / --no-extra leave their parts out of a --full run
    line, extra = _bench(["--full", "--no-cpu", "--no-extra"])
    assert "cpu_baseline" not in line and "box" in line and "table_rows_at_end" in line
    assert extra == []
