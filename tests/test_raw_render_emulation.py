"""The raw-key renderer's lane code (csrc/bc_raw_render.h: digit decode, base decode, run lookup, line length, line write)
on the host under AddressSanitizer, against the Python formatter of tests/raw_render_lib.py.  The harness itself checks
that the length predicted for a line is the number of bytes written and that lines staged through small windows, as a
wavefront stages them, give the same text."""
import itertools
import random

import pytest

import raw_render_lib as rrl

COUNTS = (0, 9, 10, 2 ** 32 - 1)
WINDOWS = ((4096, 0), (16, 3), (7, 1), (1, 2))


def check(groups, rows, cols, merged, S, tmp_path, tag, **kw):
    exp, exp_lines = rrl.render_py(groups, rows, cols, merged)
    got, lines = rrl.run(groups, rows, cols, merged, S, tmp_path, tag, **kw)
    assert got == exp, tag
    assert lines == exp_lines == got.count(b"\n")
    return got


def end_digits(groups):
    """digit tuples at both ends of every radix"""
    return list(itertools.product(*[sorted({0, rrl.radix(g) - 1}) for g in groups]))


@pytest.mark.parametrize("S", [1, 4])
def test_both_ends_of_every_radix(tmp_path, S):
    ids = [b"first", b"", b"mid,dle", b"last_one"]
    # (every key space stays below 2^63, as a plan's does: 27 bases fill it alone, so they come without samples)
    longest = [27] if S == 1 else [26]
    for gi, groups in enumerate(([1, 25], [25, 1], [ids, 24, 1], [1, ids, 8], longest, [ids], [8, 8, 8])):
        assert 5 ** 27 < 2 ** 63 and rrl.tuple_number(groups, [rrl.radix(g) - 1 for g in groups]) * S + S - 1 < 2 ** 63
        rows, k = [], 0
        for digits in end_digits(groups):
            for s in sorted({0, S - 1}):
                rows.append((s, digits, COUNTS[k % 4]))
                k += 1
        for s in range(S):
            for win, pad in WINDOWS:
                check(groups, rows, [s], False, S, tmp_path, "ends%d_%d_%d_%d" % (gi, S, s, win), win=win, pad=pad)
        for cols in ([0], list(range(S)), [S - 1, 0, S - 1]):
            for win, pad in WINDOWS:
                check(groups, rows, cols, True, S, tmp_path, "ends%d_%d_m%d_%d" % (gi, S, len(cols), win), win=win, pad=pad)


def test_capture_text_and_order(tmp_path):
    """first base first in the text, least significant in the order; the largest key of a 27-base capture"""
    groups = [27]
    seqs = ["A" * 27, "N" * 27, "C" + "A" * 26, "A" * 26 + "C", "ACTGN" * 5 + "AC"]
    rows = [(0, (rrl.code_of(s),), i + 1) for i, s in enumerate(seqs)]
    got = check(groups, rows, [0], False, 1, tmp_path, "text")
    assert got.split(b"\n")[:-1] == [b"A" * 27 + b",1", b"C" + b"A" * 26 + b",3", b"A" * 26 + b"C,4",
                                     b"ACTGN" * 5 + b"AC,5", b"N" * 27 + b",2"]
    assert rrl.code_of("N" * 27) == 5 ** 27 - 1
    one = [1]
    got = check(one, [(0, (d,), 10 + d) for d in range(5)], [0], False, 1, tmp_path, "one")
    assert got == b"A,10\nC,11\nT,12\nG,13\nN,14\n"


def test_counts_at_every_digit_boundary(tmp_path):
    groups = [3]
    values = sorted({10 ** k - 1 for k in range(1, 10)} | {10 ** k for k in range(1, 10)} | {1, 2 ** 32 - 1})
    rows = [(0, (i,), x) for i, x in enumerate(values)]
    got = check(groups, rows, [0], False, 1, tmp_path, "digits", win=5, pad=1)
    assert b",4294967295\n" in got and b",1000000000\n" in got
    # the same values as the columns of one merged line; a zero count among them, a sample listed twice
    S = len(values) + 1
    rows = [(s, (124,), x) for s, x in enumerate(values)]
    cols = list(range(S)) + [0]
    got = check(groups, rows, cols, True, S, tmp_path, "digits_m", win=9, pad=3)
    assert got == b"NNN," + b",".join(b"%d" % x for x in values) + b",0,1\n"


def test_merged_runs(tmp_path):
    """runs of every length 1 .. S, a tuple that only unlisted samples count (no line), zero counts held in the map"""
    S = 4
    groups = [2, [b"x", b"yy"]]
    rng = random.Random(5)
    rows = []
    for t in range(25):
        for s in rng.sample(range(S), rng.randint(1, S)):
            rows.append((s, (t, t & 1), rng.choice(COUNTS)))
    for cols in ([0, 1, 2, 3], [3, 1], [2, 2, 0], [1]):
        for win, pad in WINDOWS[:3]:
            check(groups, rows, cols, True, S, tmp_path, "runs%d_%d" % (len(cols), win), win=win, pad=pad)
    for s in range(S):
        check(groups, rows, [s], False, S, tmp_path, "runs_s%d" % s, win=16, pad=3)


def test_more_than_one_chunk_and_empty(tmp_path):
    groups = [4, 4]
    rng = random.Random(9)
    seen = rng.sample(range(625 * 625), 300)
    rows = [(rng.randrange(2), (t // 625, t % 625), rng.choice((1, 12, 345))) for t in seen]
    check(groups, rows, [0], False, 2, tmp_path, "chunks0", win=64, pad=2)
    check(groups, rows, [1, 0], True, 2, tmp_path, "chunksm", win=64, pad=2)
    assert check(groups, [], [0], False, 2, tmp_path, "empty") == b""
    assert check(groups, rows, [], True, 2, tmp_path, "nocols") == b""
