"""Which writer `barcode-count` gives a run's files (csrc/bc_cli_writers.hpp: choose_writers, writer_reports,
enrichment_report), over all 2^15 combinations of the fifteen facts, against a transcription of the rule as main() of
csrc/barcode_count_main.cpp held it before the decision had a header of its own.  The header runs in
tests/cli/writers_host.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, a child process with nothing preloaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cli", "writers_host.cpp")
EXE = os.path.join(ROOT, "tests", "cli", "writers_host")
DEPS = [SRC, os.path.join(ROOT, "ngs-barcode-count_amd", "csrc", "bc_cli_writers.hpp")]

# bit k of a combination's number (the order of writers_host.cpp)
FACTS = ["dense", "raw", "enrich", "counted_named_all", "counted_whole", "sample_group", "sample_ids", "plain_ids",
         "no_empty_id", "wide", "enrich_entries_ok", "dense_text_off", "dense_enrich_text_off", "raw_text_on",
         "raw_enrich_text_on"]


def old_main(f):
    """The old main(), from `const bool sample_group` to the `enrichment:` report, with its own names; what it read from
    the plan, the engine and the environment comes from the facts.  -> (counts writer, enrichment writer, stderr lines)

    Two things it could not hold as booleans:
    - bc_plan_mode() is one number, so `dense` and `raw_plan` were never both true.  Of the two facts, dense is read first.
    - fill_enrichment() succeeds here.  Its failure is known only at run time; main() then went back to the rows, and
      the caller of choose_writers does the same."""
    mode = 1 if f["dense"] else (2 if f["raw"] else 0)
    args_enrich = f["enrich"]
    counted_size_is_barcode_num = f["counted_named_all"]
    sample_group = f["sample_group"]
    samples_empty = not f["sample_ids"]
    plain_ids, no_empty_id = f["plain_ids"], f["no_empty_id"]
    dw_is_0, de_is_0 = f["dense_text_off"], f["dense_enrich_text_off"]
    rw_is_1, re_is_1 = f["raw_text_on"], f["raw_enrich_text_on"]
    state = {"enrich_filled": False}

    def fill_enrichment():
        state["enrich_filled"] = True
        return True

    device_writers = device_enrich = raw_writers = raw_enrich = wide_keys = False
    dense = mode == 1
    enrich_tried = False
    device_writers = dense and not dw_is_0 and counted_size_is_barcode_num and (sample_group or samples_empty)
    if device_writers and args_enrich:
        device_enrich = plain_ids and no_empty_id and not de_is_0 and f["enrich_entries_ok"]
        if not device_enrich:
            enrich_tried = plain_ids
            device_writers = plain_ids and fill_enrichment()
    raw_plan = mode == 2
    if raw_plan:
        counted_whole = f["counted_whole"]
        wide_keys = f["wide"]
        raw_enrich_ok = re_is_1 and not wide_keys
        raw_writers = (rw_is_1 and (not sample_group or not samples_empty) and (sample_group or samples_empty)
                       and (not args_enrich or raw_enrich_ok) and counted_whole)
        raw_enrich = device_enrich = raw_writers and args_enrich
    lines = ["[barcode-count] writers: " + ("device text (bc_engine_render_counts)" if device_writers else "per-row strings")]
    if args_enrich:
        lines.append("[barcode-count] enrichment writers: " +
                     ("device text (bc_engine_render_raw_enriched)" if raw_enrich
                      else "device text (bc_engine_render_enriched)" if device_enrich else "per-row strings"))
    if raw_plan:
        lines.append("[barcode-count] raw writers: " +
                     ("per-row strings" if not raw_writers
                      else "device text (bc_engine_render_wide_counts)" if wide_keys
                      else "device text (bc_engine_render_raw_counts)"))
    if args_enrich and not device_enrich and dense and counted_size_is_barcode_num and plain_ids and not enrich_tried:
        fill_enrichment()
    if args_enrich:
        lines.append("[barcode-count] enrichment: " +
                     ("device run sums (bc_engine_render_raw_enriched)" if raw_enrich
                      else "device marginal sums (bc_engine_render_enriched)" if device_enrich
                      else "device marginal sums (bc_engine_enrich)" if state["enrich_filled"] else "per-row string adds"))
    # the writers those booleans sent a file to (render_file, write_counts_files, write_enriched_files, add_counts_string)
    counts = ("WideText" if raw_writers and wide_keys else "RawText" if raw_writers
              else "DenseText" if device_writers else "Rows")
    enrich = ("None" if not args_enrich else "RawText" if raw_enrich else "DenseText" if device_enrich
              else "Marginals" if state["enrich_filled"] else "RowAdds")
    return counts, enrich, lines


@pytest.fixture(scope="module")
def decided():
    """{combination number: (counts writer, enrichment writer, report lines)} as the header decides"""
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", EXE, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([EXE], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and not p.stderr, "exit %d\n%s" % (p.returncode, p.stderr.decode(errors="replace")[-4000:])
    out = {}
    for line in p.stdout.decode().split("\n")[:-1]:
        if line.startswith("\t"):
            out[bits][2].append(line[1:])
        else:
            bits, counts, enrich = line.split(" ")
            bits = int(bits)
            assert bits not in out
            out[bits] = (counts, enrich, [])
    return out


def test_every_combination_against_the_old_main(decided):
    assert sorted(decided) == list(range(1 << len(FACTS)))
    wrong = []
    for bits in range(1 << len(FACTS)):
        f = {name: bool(bits >> k & 1) for k, name in enumerate(FACTS)}
        want = old_main(f)
        if decided[bits] != want:
            wrong.append((sorted(k for k in f if f[k]), decided[bits], want))
    assert not wrong, "%d combinations differ, the first: %r" % (len(wrong), wrong[0])


DENSE = ["dense", "counted_named_all", "counted_whole", "sample_group", "sample_ids", "plain_ids", "no_empty_id", "enrich_entries_ok"]
# (a raw-key plan's facts without a counted file: no ID to be empty or to hold a comma; the engine has no marginal sums)
RAW = ["raw", "counted_whole", "sample_group", "sample_ids", "plain_ids", "no_empty_id"]
BOTH_SWITCHES = ["raw_text_on", "raw_enrich_text_on"]


@pytest.mark.parametrize("name,on,off,counts,enrich", [
    ("dense, all files on the device", DENSE + ["enrich"], [], "DenseText", "DenseText"),
    ("dense without -e", DENSE, [], "DenseText", "None"),
    ("an empty ID", DENSE + ["enrich"], ["no_empty_id"], "DenseText", "Marginals"),
    ("an ID with a comma", DENSE + ["enrich"], ["plain_ids"], "Rows", "RowAdds"),
    ("a sample file without a sample group", DENSE + ["enrich"], ["sample_group"], "Rows", "Marginals"),
    ("BC_DEVICE_WRITERS=0", DENSE + ["enrich", "dense_text_off"], [], "Rows", "Marginals"),
    ("BC_DEVICE_ENRICH_WRITERS=0", DENSE + ["enrich", "dense_enrich_text_off"], [], "DenseText", "Marginals"),
    ("raw, default", RAW, [], "Rows", "None"),
    ("raw -e, default", RAW + ["enrich"], [], "Rows", "RowAdds"),
    ("raw, the counts switch", RAW + ["raw_text_on"], [], "RawText", "None"),
    ("raw -e, the counts switch alone", RAW + ["enrich", "raw_text_on"], [], "Rows", "RowAdds"),
    ("raw -e, both switches", RAW + ["enrich"] + BOTH_SWITCHES, [], "RawText", "RawText"),
    ("wide, the counts switch", RAW + ["wide", "raw_text_on"], [], "WideText", "None"),
    ("wide -e, both switches", RAW + ["wide", "enrich"] + BOTH_SWITCHES, [], "Rows", "RowAdds"),
    ("raw -e, the enrichment switch alone", RAW + ["enrich", "raw_enrich_text_on"], [], "Rows", "RowAdds"),
    ("raw, a sample barcode kept raw", RAW + ["raw_text_on"], ["sample_ids"], "Rows", "None"),
])
def test_named_rows(decided, name, on, off, counts, enrich):
    """the combinations the GPU tests of the command line run"""
    assert set(on + off) <= set(FACTS)
    bits = sum(1 << FACTS.index(k) for k in set(on) - set(off))
    assert decided[bits][:2] == (counts, enrich), (name, decided[bits])
