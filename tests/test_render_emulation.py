"""The text renderer's lane code (csrc/bc_render.h: digit count, u32 -> decimal, line length, line write) on the host
under AddressSanitizer, against the Python rendering of tests/render_lib.py.  The harness itself checks that the length
predicted for a line is the number of bytes written, and that lines staged through small windows, as a wavefront stages
them, give the same text."""
import random

import pytest

import render_lib

BOUNDARIES = [1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999,
              100000000, 999999999, 1000000000, 4294967295]


def check(ids, table, n_samples, cols, tmp_path, tag, **kw):
    T = len(table) // n_samples
    counts = [table[s * T:(s + 1) * T] for s in range(n_samples)]
    if kw.get("bits") is not None:
        counts = [[(c + ((kw["bits"][(s * T + t) >> 5] >> ((s * T + t) & 31)) & 1)) & 0xFFFFFFFF for t, c in enumerate(row)]
                  for s, row in enumerate(counts)]
    exp, exp_lines = render_lib.render_py(ids, counts, cols)
    got, lines = render_lib.run(ids, table, n_samples, cols, tmp_path, tag, **kw)
    assert got == exp, tag
    assert lines == exp_lines == got.count(b"\n")
    return got


def test_every_digit_count_boundary(tmp_path):
    ids = [[b"x%d" % i for i in range(len(BOUNDARIES) + 3)]]
    table = [0] + BOUNDARIES + [0, 7]  # (0 is never a line)
    got = check(ids, table, 1, [0], tmp_path, "digits")
    assert got.split(b"\n")[:3] == [b"x1,1", b"x2,9", b"x3,10"]
    assert b"x20,4294967295\n" in got and b"x0," not in got and b"x21," not in got


def test_bit_map_adds_one_and_wraps_like_the_table_readers(tmp_path):
    ids = [[b"a", b"b", b"c", b"d"]]
    table = [0, 9, 0, 4294967295]
    check(ids, table, 1, [0], tmp_path, "bits", bits=[0b1011])  # -> 1, 10, 0, 0 (u32 arithmetic, as compact_range_kernel)


@pytest.mark.parametrize("G", [1, 3, 4])
def test_ids_of_every_kind(tmp_path, G):
    odd = [b"", b"Z" * 300, b"a,b", b'say "hi"', "é中".encode(), bytes([0x80, 0xFF, 0xFE]), b"plain"]
    rng = random.Random(G)
    ids = []
    for g in range(G):
        pool = odd[:]
        rng.shuffle(pool)
        ids.append(pool[:3 + g] if G > 1 else pool)
    T = 1
    for g in ids:
        T *= len(g)
    table = [rng.choice([0, 0, 1, 12, 345, 4294967295]) for _ in range(2 * T)]
    table[0], table[T - 1], table[T], table[2 * T - 1] = 5, 6, 0, 8
    for win, pad in ((4096, 0), (16, 3), (7, 1), (1, 2)):
        check(ids, table, 2, [0], tmp_path, "ids%d_%d" % (G, win), win=win, pad=pad)
        check(ids, table, 2, [1], tmp_path, "ids%d_%d_s1" % (G, win), win=win, pad=pad)


def test_merged_rows(tmp_path):
    ids = [[b"p", b"", b"qq"], [b"1", b"2"]]
    T, S = 6, 4
    table = [0] * (S * T)
    table[0 * T + 1] = 3            # only sample 0
    table[1 * T + 1] = 1000000000   # samples 0 and 1 share tuple 1
    table[2 * T + 4] = 77           # only sample 2
    table[3 * T + 5] = 9            # only sample 3: absent unless listed
    got = check(ids, table, S, [0, 1, 2], tmp_path, "m012")
    assert got == b"p,2,3,1000000000,0\nqq,1,0,0,77\n"
    check(ids, table, S, [2, 0, 1], tmp_path, "shuffled")
    assert check(ids, table, S, [1, 1, 0], tmp_path, "repeat") == b"p,2,1000000000,1000000000,3\n"
    assert check(ids, table, S, [3], tmp_path, "one") == b"qq,2,9\n"
    assert check(ids, table, S, [], tmp_path, "none") == b""
    for win in (5, 13):
        check(ids, table, S, [3, 2, 1, 0, 3], tmp_path, "mwin%d" % win, win=win, pad=2)


def test_many_chunks_with_gaps(tmp_path):
    rng = random.Random(5)
    ids = [[b"i%d" % i for i in range(7)], [b"j%d" % i for i in range(61)]]  # T = 427: chunk ends inside the last axis
    T = 7 * 61
    table = [rng.choice([0, 0, 0, rng.randrange(1, 10 ** rng.randrange(1, 10))]) for _ in range(3 * T)]
    for t in range(64, 200):
        table[t] = 0  # two empty chunks
    check(ids, table, 3, [0], tmp_path, "gaps", win=64, pad=1)
    check(ids, table, 3, [2, 0], tmp_path, "gaps_m", win=257, pad=3)
