"""bc_plan_precompile and BC_WIDE_LANE (no GPU needed: the hook cross-compiles for gfx950): with the switch on, the
specialised kernel of an eligible wide-key plan is built into the cache; with it off, or for a plan the lane kernel
cannot run, the plan is refused as it always was.  tests/test_gpu_wide_lane.py sees an engine load such an object."""
import os

import pytest

import ngs_barcode_count_amd as pkg

SCHEME_30 = "GTACCAGTC{30}TGCATGGAC"   # Barcode-seq, a 30-base raw capture: wide, and within the lane kernel's widths
SCHEME_40 = "GTACCAGTC{40}TGCATGGAC"   # a group above 32 bases: the wave-per-read kernel's, whatever the switch says


def _objects(d):
    return sorted(f for f in os.listdir(d) if f.startswith("bcjit_") and f.endswith(".co"))


@pytest.mark.parametrize("switch", [None, "0"])
def test_refused_with_the_switch_off(switch, monkeypatch, tmp_path):
    if switch is None:
        monkeypatch.delenv("BC_WIDE_LANE", raising=False)
    else:
        monkeypatch.setenv("BC_WIDE_LANE", switch)
    with pytest.raises(pkg.BarcodeCountError) as err:
        pkg.precompile(pkg.Plan(SCHEME_30), stride=100, read_len=100, cache_dir=str(tmp_path))
    assert "at most 27 bases" in str(err.value)
    assert _objects(str(tmp_path)) == []


def test_built_with_the_switch_on(monkeypatch, tmp_path):
    monkeypatch.setenv("BC_WIDE_LANE", "1")
    with pytest.raises(pkg.BarcodeCountError) as err:
        pkg.precompile(pkg.Plan(SCHEME_40), stride=100, read_len=100, cache_dir=str(tmp_path))
    assert "1..32 bases" in str(err.value) and _objects(str(tmp_path)) == []
    plan = pkg.Plan(SCHEME_30)
    assert plan.mode == "sparse" and plan.table_entries == 0  # (the plan's own queries do not depend on the switch)
    pkg.precompile(plan, stride=100, read_len=100, cache_dir=str(tmp_path))
    objs = _objects(str(tmp_path))
    assert objs and all(os.path.getsize(os.path.join(str(tmp_path), f)) > 4096 for f in objs)
