"""The raw-key enrichment renderer's lane code (csrc/bc_raw_enrich_render.h: projection, segment search, run lookup,
line length, line write) on the host under AddressSanitizer + UBSan, against the Python formatter of
tests/raw_enrich_render_lib.py, which builds the Single / Double maps from the rows as add_single / add_double do.  The
harness projects every sorted pair with the header's code, sorts and sums the runs itself, and checks that the length
predicted for a line is the number of bytes written and that lines staged through small windows, as a wavefront stages
them, give the same text."""
import random

import pytest

import raw_enrich_render_lib as rel
import raw_render_lib as rrl

COUNTS = (1, 9, 10, 2 ** 32 - 1)
WINDOWS = ((4096, 0), (300, 3), (16, 1), (7, 2))
IDS_A = [b"first", b"second_id", b"x", b"last_one"]
IDS_B = [b"p", b"qq", b"rrr"]
SHARED = [b"one", b"two", b"one", b"three", b"two", b"one"]  # entries 0, 2, 5 are one key; so are 1 and 4


def check(groups, rows, cols, merged, kind, S, tmp_path, tag, **kw):
    exp, exp_lines = rel.render_py(groups, rows, cols, merged, kind)
    got, lines = rel.run(groups, rows, cols, merged, kind, S, tmp_path, tag, **kw)
    assert got == exp, tag
    assert lines == exp_lines == got.count(b"\n")
    return got


def random_rows(groups, S, n, seed, samples=None, pool=12):
    """n distinct (sample, tuple) rows; every group draws from a small pool of digits (both ends of its radix among
    them), so that the projections have runs longer than one"""
    rng = random.Random(seed)
    pools = []
    for g in groups:
        r = rrl.radix(g)
        pools.append(sorted({0, r - 1} | {rng.randrange(r) for _ in range(min(pool, r))}))
    space = len(samples if samples is not None else range(S))
    for p in pools:
        space *= len(p)
    n = min(n, space * 3 // 4)  # (what the pools can give)
    seen, rows = set(), []
    while len(rows) < n:
        s = rng.choice(samples if samples is not None else range(S))
        digits = tuple(rng.choice(p) for p in pools)
        if (s, digits) not in seen:
            seen.add((s, digits))
            rows.append((s, digits, rng.choice(COUNTS)))
    return rows


def all_views(groups, rows, S, tmp_path, tag, windows=WINDOWS[:2], merged_cols=None):
    merged_cols = merged_cols if merged_cols is not None else [list(range(S)), list(range(S))[::-1], [S - 1, S - 1, 0]]
    for kind in (rel.SINGLE, rel.DOUBLE):
        for win, pad in windows:
            for s in range(S):
                check(groups, rows, [s], False, kind, S, tmp_path, "%s_k%d_s%d_w%d" % (tag, kind, s, win), win=win, pad=pad)
            for ci, cols in enumerate(merged_cols):
                check(groups, rows, cols, True, kind, S, tmp_path, "%s_k%d_m%d_w%d" % (tag, kind, ci, win), win=win, pad=pad)


@pytest.mark.parametrize("name,groups", [
    ("g1_raw", [8]), ("g1_known", [IDS_A]),
    ("g2_raw", [5, 7]), ("g2_known", [IDS_A, IDS_B]), ("g2_mixed", [IDS_B, 6]),
    ("g3_raw", [8, 8, 8]), ("g3_known", [IDS_A, IDS_B, SHARED]), ("g3_mixed", [SHARED, 8, 8]), ("g3_mixed2", [4, IDS_A, 3]),
    ("g4_raw", [3, 4, 5, 6]), ("g4_known", [IDS_A, IDS_B, IDS_B, IDS_A]), ("g4_mixed", [2, SHARED, 9, IDS_B]),
])
def test_group_counts_and_kinds(tmp_path, name, groups):
    S = 4
    assert rrl.tuple_number(groups, [rrl.radix(g) - 1 for g in groups]) * S + S - 1 < 2 ** 63
    space = 1
    for g in groups:
        space *= min(rrl.radix(g), 13)
    rows = random_rows(groups, S, min(150, space * S // 2), seed=len(name) * 7 + len(groups))
    all_views(groups, rows, S, tmp_path, name)


def test_the_example_lines(tmp_path):
    """the lines of the DEL scheme's three raw 8-base groups, written out by hand (captures compare from their LAST base
    backwards with A < C < T < G < N, so TTGCAAGC comes before ACGTACGT)"""
    groups = [8, 8, 8]
    a, b, c = (rrl.code_of(x) for x in ("ACGTACGT", "TTGCAAGC", "GGATCCAA"))
    rows = [(0, (a, a, b), 3), (0, (a, b, b), 4), (1, (a, a, b), 5)]
    assert check(groups, rows, [0], False, rel.SINGLE, 2, tmp_path, "ex_s") == (
        b"ACGTACGT,,,7\n" b",TTGCAAGC,,4\n" b",ACGTACGT,,3\n" b",,TTGCAAGC,7\n")
    assert check(groups, rows, [1, 0], True, rel.DOUBLE, 2, tmp_path, "ex_d") == (
        b"ACGTACGT,TTGCAAGC,,0,4\n" b"ACGTACGT,ACGTACGT,,5,3\n" b"ACGTACGT,,TTGCAAGC,5,7\n"
        b",TTGCAAGC,TTGCAAGC,0,4\n" b",ACGTACGT,TTGCAAGC,5,3\n")
    rows.append((1, (c, a, a), 2 ** 32 - 1))
    got = check(groups, rows, [1], False, rel.DOUBLE, 2, tmp_path, "ex_d1")
    assert b"GGATCCAA,,ACGTACGT,4294967295\n" in got and got.count(b"\n") == 6


def test_shared_id_is_one_key(tmp_path):
    """two sequences of a known set under one ID: one line that holds both sums"""
    groups = [SHARED, 3, 3]
    rows = [(0, (0, 1, 2), 5), (0, (2, 1, 2), 7), (0, (5, 4, 2), 11), (1, (2, 1, 2), 1), (0, (1, 0, 0), 2), (1, (4, 0, 0), 3)]
    got = check(groups, rows, [0], False, rel.SINGLE, 2, tmp_path, "shared_s")
    assert got.startswith(b"one,,,23\ntwo,,,2\n") and got.count(b"one") == 1
    got = check(groups, rows, [0, 1], True, rel.SINGLE, 2, tmp_path, "shared_m")
    assert got.startswith(b"one,,,23,1\ntwo,,,2,3\n")
    got = check(groups, rows, [0, 1], True, rel.DOUBLE, 2, tmp_path, "shared_d", win=16, pad=3)
    assert b"one,CAA,,12,1\n" in got and b"one,NAA,,11,0\n" in got and b"two,AAA,,2,3\n" in got
    all_views(groups, rows, 2, tmp_path, "shared")


def test_keys_at_the_top_of_the_word(tmp_path):
    """A 27-base capture fills a word alone (5^27 < 2^63 < 5^27 * 2 < 2^64 < 5^27 * 4): beside S = 4 the plan's key would
    not fit one word, so the capture comes with S = 1 (the key just below 2^63) and S = 2 (bit 63 is set); 26 bases are the
    longest capture S = 4 leaves room for."""
    assert 5 ** 27 < 2 ** 63 < 5 ** 27 * 2 < 2 ** 64 < 5 ** 27 * 4 and 5 ** 26 * 4 < 2 ** 63
    top = "N" * 27
    for S, groups in ((1, [27]), (2, [27]), (4, [26]), (4, [IDS_B, 24, 1]), (4, [1, 1, 24])):
        rows = random_rows(groups, S, 40, seed=S + len(groups))
        ends = tuple(rrl.radix(g) - 1 for g in groups)
        if (S - 1, ends) not in {(s, d) for s, d, _ in rows}:
            rows.append((S - 1, ends, 2 ** 32 - 1))
        assert max(rrl.tuple_number(groups, d) * S + s for s, d, _ in rows) == rrl.tuple_number(groups, ends) * S + S - 1
        all_views(groups, rows, S, tmp_path, "top%d_%d" % (S, len(groups)), windows=((4096, 0), (16, 3)))
    got = check([27], [(1, (5 ** 27 - 1,), 2 ** 32 - 1), (0, (5 ** 27 - 1,), 1)], [1, 0], True, rel.SINGLE, 2, tmp_path, "top")
    assert got == top.encode() + b",4294967295,1\n"


def test_sums_pass_32_bits(tmp_path):
    groups = [2, 2, 2]
    rows = [(0, (d, e, 3), 2 ** 32 - 1) for d in range(25) for e in range(25)]
    got = check(groups, rows, [0], False, rel.SINGLE, 1, tmp_path, "big", win=16, pad=1)
    assert (",,GA,%d\n" % (625 * (2 ** 32 - 1))).encode() in got and 625 * (2 ** 32 - 1) > 2 ** 41
    check(groups, rows, [0, 0], True, rel.DOUBLE, 1, tmp_path, "big_d", win=300, pad=2)


def test_no_sample_group(tmp_path):
    for groups in ([8, 8, 8], [IDS_A, 5], [SHARED, IDS_B, 2]):
        rows = random_rows(groups, 1, 80, seed=len(groups))
        all_views(groups, rows, 1, tmp_path, "s1_%d" % len(groups), merged_cols=[[0], [0, 0]])


def test_a_sample_that_counts_nothing(tmp_path):
    S = 4
    groups = [6, IDS_A, 6]
    rows = random_rows(groups, S, 120, seed=3, samples=[0, 1, 3])
    for kind in (rel.SINGLE, rel.DOUBLE):
        assert check(groups, rows, [2], False, kind, S, tmp_path, "none_k%d" % kind) == b""
        assert check(groups, rows, [2, 2], True, kind, S, tmp_path, "none_m_k%d" % kind) == b""
        got = check(groups, rows, [3, 2, 0], True, kind, S, tmp_path, "none_c_k%d" % kind, win=300, pad=1)
        assert all(line.split(b",")[-2] == b"0" for line in got.split(b"\n")[:-1])
    all_views(groups, rows, S, tmp_path, "none")


def test_lines_straddle_small_windows_and_many_chunks(tmp_path):
    """more than 64 positions per segment (several chunks of a wavefront), windows of a few hundred bytes and of a few"""
    S = 3
    groups = [4, [b"id_%03d_of_a_longer_kind" % i for i in range(40)], 4]
    rows = random_rows(groups, S, 900, seed=17, pool=30)
    for kind in (rel.SINGLE, rel.DOUBLE):
        for win, pad in ((300, 0), (257, 3), (16, 2)):
            check(groups, rows, [1], False, kind, S, tmp_path, "win_k%d_%d" % (kind, win), win=win, pad=pad)
            check(groups, rows, [2, 0, 1, 2], True, kind, S, tmp_path, "win_m_k%d_%d" % (kind, win), win=win, pad=pad)


def test_empty_inputs(tmp_path):
    groups = [4, 4, 4]
    rows = random_rows(groups, 2, 30, seed=1)
    for kind in (rel.SINGLE, rel.DOUBLE):
        assert check(groups, [], [0], False, kind, 2, tmp_path, "empty_k%d" % kind) == b""
        assert check(groups, rows, [], True, kind, 2, tmp_path, "nocols_k%d" % kind) == b""
    # no Double file below three counted barcodes
    assert check([4, 4], random_rows([4, 4], 2, 30, seed=2), [0, 1], True, rel.DOUBLE, 2, tmp_path, "g2_double") == b""
