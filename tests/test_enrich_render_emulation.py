"""The enrichment renderer's lane code (csrc/bc_enrich_render.h: key decode, u64 digit count, u64 -> decimal, line length,
line write, fold target) on the host under AddressSanitizer, against the Python rendering of tests/enrich_render_lib.py.
The harness itself checks that the length predicted for a line is the number of bytes written, that every key decodes to
itself, and that lines staged through small windows, as a wavefront stages them, give the same text."""
import random

import pytest

import enrich_render_lib as erl
from enrich_render_lib import DOUBLE, SINGLE

BOUNDARIES = sorted({10 ** k - 1 for k in range(1, 20)} | {10 ** k for k in range(1, 20)} | {2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1})
WINDOWS = ((4096, 0), (16, 3), (7, 1), (1, 2))


def n_keys(ids, kind):
    return len(erl.keys(ids, kind))


def check(ids, sums, kind, cols, tmp_path, tag, **kw):
    exp, exp_lines = erl.render_py(ids, sums, kind, cols)
    got, lines = erl.run(ids, sums, kind, cols, tmp_path, tag, **kw)
    assert got == exp, tag
    assert lines == exp_lines == got.count(b"\n")
    return got


def test_every_u64_digit_boundary(tmp_path):
    assert len(BOUNDARIES) == 41
    ids = [[b"x%d" % i for i in range(len(BOUNDARIES) + 3)]]
    sums = [[0] + BOUNDARIES + [0, 7]]  # (0 is never a line)
    got = check(ids, sums, SINGLE, [0], tmp_path, "digits")
    assert got.split(b"\n")[:3] == [b"x1,9", b"x2,10", b"x3,99"]
    for k, x in enumerate(BOUNDARIES):
        assert b"x%d,%d\n" % (k + 1, x) in got
    assert b"18446744073709551615\n" in got and b"x0," not in got and b"x42," not in got
    # the same values as the columns of one merged line, and through windows that cut the digits
    ids3 = [[b"a"], [b"b", b"c"], [b"d"]]
    sums3 = [[0, 0, 0, x, 0] for x in BOUNDARIES]  # pair (0,2) = key 2 .. : K = 1*2 + 1*1 + 2*1 = 5, key 3 = (1,2) i=0
    for win, pad in WINDOWS:
        got = check(ids3, sums3, DOUBLE, list(range(len(BOUNDARIES))), tmp_path, "digits_m%d" % win, win=win, pad=pad)
        assert got == b",b,d," + b",".join(b"%d" % x for x in BOUNDARIES) + b"\n"


@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_field_layout_for_every_group_count(tmp_path, G):
    ids = [[b"g%d_%d" % (g, i) for i in range(2 + g)] for g in range(G)]
    rng = random.Random(G)
    for kind in (SINGLE, DOUBLE):
        K = n_keys(ids, kind)
        sums = [[rng.choice([0, 3, 2 ** 40 + 5]) for _ in range(K)] for _ in range(2)]
        if K:
            sums[0][0], sums[0][K - 1] = 1, 2
        got = check(ids, sums, kind, [0], tmp_path, "layout%d_%d" % (G, kind))
        check(ids, sums, kind, [1, 0], tmp_path, "layout%d_%d_m" % (G, kind), win=9, pad=3)
        if kind == DOUBLE and G < 3:
            assert K == 0 and got == b""  # no Double lines below three counted barcodes
        elif kind == SINGLE:
            assert got.split(b"\n")[0] == b"g0_0" + b"," * (G - 1) + b",1"
            assert got.split(b"\n")[-2] == b"," * (G - 1) + b"g%d_%d,2" % (G - 1, G)
        else:
            assert got.split(b"\n")[0] == b"g0_0,g1_0" + b"," * (G - 2) + b",1"
            assert got.split(b"\n")[-2] == b"," * (G - 2) + b"g%d_%d,g%d_%d,2" % (G - 2, G - 1, G - 1, G)
    if G == 3:
        assert erl.run(ids, [[0, 0, 5, 0, 0, 0, 0, 0, 0]], SINGLE, [0], tmp_path, "mid")[0] == b",g1_0,,5\n"


@pytest.mark.parametrize("G", [1, 3, 4])
def test_ids_of_every_kind(tmp_path, G):
    odd = [b"", b"Z" * 300, b"a,b", b'say "hi"', "é中".encode(), bytes([0x80, 0xFF, 0xFE]), b"plain"]
    rng = random.Random(10 + G)
    ids = []
    for g in range(G):
        pool = odd[:]
        rng.shuffle(pool)
        ids.append(pool[:3 + g] if G > 1 else pool)
    for kind in (SINGLE, DOUBLE):
        K = n_keys(ids, kind)
        sums = [[rng.choice([0, 0, 1, 12, 345, 4294967296, 2 ** 64 - 1]) for _ in range(K)] for _ in range(2)]
        for win, pad in WINDOWS:
            check(ids, sums, kind, [0], tmp_path, "ids%d_%d_%d" % (G, kind, win), win=win, pad=pad)
            check(ids, sums, kind, [1, 0], tmp_path, "ids%d_%d_%d_m" % (G, kind, win), win=win, pad=pad)


def test_shared_ids_fold_onto_the_smallest_index(tmp_path):
    ids = [[b"A", b"B", b"A", b"C", b"B"], [b"x", b"x", b"y"], [b"p", b"q", b"p"]]
    assert erl.canon_of(ids) == [0, 1, 0, 3, 1, 0, 0, 2, 0, 1, 0]
    # singles: SUM = 11
    s0 = [0, 2, 5, 0, 40, 0, 7, 0, 1, 0, 9]     # A only through entry 2; B = 2 + 40; x only through entry 1; p = 1 + 9
    s1 = [2 ** 63, 0, 2 ** 63 - 1, 0, 0, 0, 0, 0, 0, 0, 0]  # A = 2^64 - 1
    got = check(ids, [s0, s1], SINGLE, [0], tmp_path, "fold_s")
    assert got == b"A,,,5\nB,,,42\n,x,,7\n,,p,10\n"
    assert check(ids, [s0, s1], SINGLE, [1], tmp_path, "fold_s1") == b"A,,,18446744073709551615\n"
    assert check(ids, [s0, s1], SINGLE, [1, 0], tmp_path, "fold_sm", win=5, pad=1).startswith(b"A,,,18446744073709551615,5\nB,,,0,42\n")
    # doubles: pairs (0,1) 15 keys, (0,2) 15, (1,2) 9
    K = n_keys(ids, DOUBLE)
    assert K == 39
    d = [0] * K
    d[2 * 3 + 1] = 4        # (A#2, x#1) -> (A#0, x#0): non-zero only through a folded entry
    d[0 * 3 + 0] = 0
    d[4 * 3 + 2] = 6        # (B#4, y) -> (B#1, y)
    d[1 * 3 + 2] = 10       # (B#1, y) itself
    d[15 + 3 * 3 + 2] = 8   # (C, p#2) -> (C, p#0)
    d[30 + 1 * 3 + 2] = 3   # (x#1, p#2) -> (x#0, p#0)
    d[30 + 2 * 3 + 1] = 11  # (y, q): canonical
    got = check(ids, [d, [0] * K], DOUBLE, [0], tmp_path, "fold_d")
    assert got == b"A,x,,4\nB,y,,16\nC,,p,8\n,x,p,3\n,y,q,11\n"
    for win, pad in WINDOWS:
        check(ids, [d, d[::-1]], DOUBLE, [1, 0, 1], tmp_path, "fold_dm%d" % win, win=win, pad=pad)
    # a plan without shared IDs never folds: the same sums, no map
    plain = [[b"A", b"B"], [b"x"], [b"p", b"q"]]
    assert erl.canon_of(plain) is None
    check(plain, [[1, 2, 3, 4, 5]], SINGLE, [0], tmp_path, "nofold")


def test_merged_columns(tmp_path):
    ids = [[b"p", b"", b"qq"], [b"1", b"2"], [b"z"]]
    S = 4
    for kind in (SINGLE, DOUBLE):
        K = n_keys(ids, kind)
        sums = [[0] * K for _ in range(S)]
        sums[0][1] = 3
        sums[1][1] = 10 ** 19
        sums[2][4] = 77
        sums[3][5] = 9  # only sample 3: absent unless listed
        got = check(ids, sums, kind, [0, 1, 2], tmp_path, "m012_%d" % kind)
        assert got.count(b"\n") == 2 and b",3,10000000000000000000,0\n" in got and b",0,0,77\n" in got
        check(ids, sums, kind, [2, 0, 1], tmp_path, "shuffled_%d" % kind)
        rep = check(ids, sums, kind, [1, 1, 0], tmp_path, "repeat_%d" % kind)
        assert rep.count(b"\n") == 1 and rep.endswith(b",10000000000000000000,10000000000000000000,3\n")
        one = check(ids, sums, kind, [3], tmp_path, "one_%d" % kind)
        assert one.count(b"\n") == 1 and one.endswith(b",9\n")
        assert check(ids, sums, kind, [], tmp_path, "none_%d" % kind) == b""
        for win in (5, 13):
            check(ids, sums, kind, [3, 2, 1, 0, 3], tmp_path, "mwin%d_%d" % (win, kind), win=win, pad=2)
    # the empty ID: the same text in different groups stays two lines
    assert check(ids, [[0, 5, 0, 0, 0, 0]], SINGLE, [0], tmp_path, "empty") == b",,,5\n"


def test_key_ranges_with_empty_chunks(tmp_path):
    rng = random.Random(5)
    ids = [[b"i%d" % i for i in range(7)], [b"j%d" % i for i in range(61)], [b"k%d" % i for i in range(5)]]
    for kind in (SINGLE, DOUBLE):
        K = n_keys(ids, kind)
        sums = [[rng.choice([0, 0, 0, rng.randrange(1, 10 ** rng.randrange(1, 20))]) for _ in range(K)] for _ in range(3)]
        for s in range(3):
            for k in range(64, min(K, 200) if kind == DOUBLE else 64):
                sums[s][k] = 0  # two empty chunks
        if kind == SINGLE:
            sums = [[0] * K for _ in range(3)]
            sums[1][70] = 12  # 73 keys: the first chunk is empty for every sample
        check(ids, sums, kind, [0], tmp_path, "gaps_%d" % kind, win=64, pad=1)
        check(ids, sums, kind, [2, 0, 1], tmp_path, "gaps_m_%d" % kind, win=257, pad=3)
