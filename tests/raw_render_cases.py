"""Workloads and the expected text of the raw-key renderer's GPU tests (tests/test_gpu_raw_render.py,
tests/mp_rank_raw_render.py).  The expected text is built from the engine's ROWS (bc_engine_finish + bc_engine_row_text,
what the host path writes from), never from the renderer: rows are grouped by sample and ordered by the digit tuple
computed from the row's own text."""
import numpy as np

import cases
import readgen
import raw_render_lib as rrl

DEL_SAMPLES = ["ACGTACGT", "TTGCAAGC", "GGATCCAA", "CATGTTAG"]


def del_raw_case(n=30_000, seed=41):
    """DEL_SCHEME, a sample file of 4, no counted file: 3 x 8 raw bases (5^24 * 4 < 2^63); the captures are drawn at
    random, so roughly one row per matched read"""
    rng = np.random.default_rng(seed)
    c = {"scheme": cases.DEL_SCHEME, "samples": {s: "Sample_%d" % i for i, s in enumerate(DEL_SAMPLES)}, "counted": None,
         "kwargs": {}}
    c["reads"] = readgen.gen_reads(rng, cases.DEL_SCHEME, n, 100, DEL_SAMPLES, None, p_sub=0.004, p_n=0.002)
    return c


def random_raw_case(n=6_000, seed=43):
    """random barcode + known sample + raw counted: the count of a tuple is the number of its distinct random barcodes"""
    rng = np.random.default_rng(seed)
    scheme = "[8]AGCTACGAATCG{6}TGGA{5}ACTAGAT(6)TAGA"
    samples = DEL_SAMPLES[:3]
    pool = [readgen.make_set(rng, 9, 6, 2), readgen.make_set(rng, 4, 5, 2)]
    c = {"scheme": scheme, "samples": {s: "S%d" % i for i, s in enumerate(samples)}, "counted": None, "kwargs": {}}
    c["reads"] = readgen.gen_reads(rng, scheme, n, 80, samples, pool, p_sub=0.01, p_n=0.004, dup_frac=0.3)
    return c


def groups_of(plan, scheme):
    """the counted groups as raw_render_lib describes them: the capture length of a raw group, the IDs of a known one"""
    lens = [v for k, v in readgen.scheme_layout(scheme) if k == "B"]
    out = []
    for g in range(plan.barcode_num):
        ids = [i.encode() for _, i in plan.counted(g)]
        out.append(ids if ids else lens[g])
    return out


def rows_of(plan, scheme, result_rows):
    """[(sample key, "b1,b2,..", count)] -> raw_render_lib rows (sample index, digits, count); known groups come as
    their sequences in a row's text, raw ones as the capture"""
    groups = groups_of(plan, scheme)
    samples = {x: i for i, (x, _) in enumerate(plan.samples())} if plan.sample_barcode else {}
    sets = [{x: i for i, (x, _) in enumerate(plan.counted(g))} for g in range(plan.barcode_num)]
    out = []
    for sample, tup, cnt in result_rows:
        digits = tuple(rrl.code_of(x) if isinstance(groups[g], int) else sets[g][x] for g, x in enumerate(tup.split(",")))
        out.append((samples[sample] if samples else 0, digits, int(cnt)))
    return groups, out


def expected(plan, scheme, result_rows, cols, merged):
    groups, rows = rows_of(plan, scheme, result_rows)
    return rrl.render_py(groups, rows, cols, merged)[0]
