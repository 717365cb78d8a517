"""The wide-key renderer's lane code (csrc/bc_wide_render.h: payload -> order key, plane reads across word boundaries, run
lookup, line length, line write) on the host under AddressSanitizer + UBSan, in two steps:
    payload -> order-key words   sorting by the order key is sorting by (digit tuple, sample), the digits computed with
                                 Python integers of any size (raw_render_lib.code_of);
    view -> text                 against raw_render_lib.render_py.
The harness itself checks that the length predicted for a line is the number of bytes written and that lines staged
through small windows, as a wavefront stages them, give the same text."""
import random

import raw_render_lib as rrl
import wide_render_lib as wrl

WINDOWS = ((4096, 0), (16, 3), (7, 1))
COUNTS = (1, 9, 10, 2 ** 32 - 1)


def check(groups, rows, cols, merged, S, has_sample, tmp_path, tag, **kw):
    got, lines, shuffled, okeys = wrl.run(groups, rows, cols, merged, S, has_sample, tmp_path, tag, **kw)
    # step 1: the order keys order the rows as (digits, s) does, and equal nothing that differs
    want = [(wrl.digits(groups, f), s) for s, f, _ in shuffled]
    by_key = sorted(range(len(shuffled)), key=lambda i: okeys[i])
    assert [want[i] for i in by_key] == sorted(want), tag
    assert len(set(okeys)) == len(set(want)), tag
    # step 2: the text
    exp, exp_lines = rrl.render_py(groups, [(s, wrl.digits(groups, f), c) for s, f, c in rows], cols, merged)
    assert got == exp, tag
    assert lines == exp_lines == got.count(b"\n")
    return got


def variants(master, alphabet="ACGTN"):
    out = [master]
    for k in range(len(master)):
        for c in alphabet:
            if c != master[k]:
                out.append(master[:k] + c + master[k + 1:])
    return out


def test_forty_bases_every_single_base_variant(tmp_path):
    """one 40-base capture: the planes lie at payload bits 0, 40 and 80, so the second crosses a word, and the order key
    (120 bits) has a base astride its two words; every single-base variant, N included"""
    rng = random.Random(3)
    master = "".join(rng.choice("ACGT") for _ in range(40))
    seqs = variants(master)
    assert len(seqs) == 161
    rows = [(0, (s,), COUNTS[i % 4]) for i, s in enumerate(seqs)]
    for win, pad in WINDOWS:
        got = check([40], rows, [0], False, 1, False, tmp_path, "v40_%d" % win, win=win, pad=pad)
    lines = got.split(b"\n")[:-1]
    codes = [rrl.code_of(x.split(b",")[0].decode()) for x in lines]
    assert codes == sorted(codes) and len(set(codes)) == 161
    assert check([40], rows, [0], True, 1, False, tmp_path, "v40_m") == got  # S = 1: the merged file is the sample's
    # both ends of the space
    ends = [(0, ("A" * 40,), 1), (0, ("N" * 40,), 2), (0, ("A" * 39 + "C",), 3), (0, ("C" + "A" * 39,), 4)]
    got = check([40], ends, [0], False, 1, False, tmp_path, "v40_ends")
    assert got == b"A" * 40 + b",1\n" + b"C" + b"A" * 39 + b",4\n" + b"A" * 39 + b"C,3\n" + b"N" * 40 + b",2\n"


def test_sample_field_and_35_bases(tmp_path):
    """a 32-bit sample field, then 35 bases whose planes start at payload bit 32: merged views with columns repeated and
    reordered, runs of every length"""
    S = 5
    rng = random.Random(7)
    master = "".join(rng.choice("ACGT") for _ in range(35))
    rows = []
    for i, seq in enumerate(variants(master)[::3]):
        for s in rng.sample(range(S), rng.randint(1, S)):
            rows.append((s, (seq,), rng.choice(COUNTS)))
    for s in range(S):
        check([35], rows, [s], False, S, True, tmp_path, "s35_%d" % s, win=16, pad=3)
    for cols in ([0, 1, 2, 3, 4], [3, 1], [2, 2, 0], [4]):
        for win, pad in WINDOWS:
            check([35], rows, cols, True, S, True, tmp_path, "s35_m%d_%d" % (len(cols), win), win=win, pad=pad)
    assert check([35], rows, [], True, S, True, tmp_path, "s35_nocols") == b""
    assert check([35], [], [0], False, S, True, tmp_path, "s35_empty") == b""


def test_two_raw_groups_first_group_leads(tmp_path):
    """[24] [28]: the first counted group is the most significant, whatever the second holds"""
    rng = random.Random(11)
    a = ["".join(rng.choice("ACGTN") for _ in range(24)) for _ in range(6)]
    b = ["".join(rng.choice("ACGTN") for _ in range(28)) for _ in range(9)]
    rows = [(0, (x, y), 1 + i + 10 * j) for i, x in enumerate(a) for j, y in enumerate(b)]
    got = check([24, 28], rows, [0], False, 1, False, tmp_path, "two", win=64, pad=2)
    firsts = [rrl.code_of(x.split(b",")[0].decode()) for x in got.split(b"\n")[:-1]]
    assert firsts == sorted(firsts)
    # the same behind 84 bits of a random barcode's cleared planes (the key is a word wider, the order key is not)
    assert check([24, 28], rows, [0], False, 1, False, tmp_path, "two_tail", tail_bits=84) == got


def test_known_group_between_raw_ones(tmp_path):
    """raw 30, a known set of 5 (IDs of every length, one empty, one with a comma), raw 22, with 3 samples"""
    ids = [b"first", b"", b"mid,dle", b"x", b"last_one"]
    groups = [30, ids, 22]
    S = 3
    rng = random.Random(13)
    a = ["".join(rng.choice("ACGTN") for _ in range(30)) for _ in range(5)]
    c = ["".join(rng.choice("ACGT") for _ in range(22)) for _ in range(4)] + ["N" * 22, "A" * 22]
    rows = []
    for x in a:
        for k in range(len(ids)):
            for z in rng.sample(c, 3):
                for s in rng.sample(range(S), rng.randint(1, S)):
                    rows.append((s, (x, k, z), rng.choice(COUNTS)))
    for s in range(S):
        check(groups, rows, [s], False, S, True, tmp_path, "mix_%d" % s, win=16, pad=1)
    for cols in ([0, 1, 2], [2, 0], [1, 1]):
        check(groups, rows, cols, True, S, True, tmp_path, "mix_m%d" % len(cols), win=7, pad=3)
    # a known set of one entry takes no bit of the order key
    one = [30, [b"only"], 22]
    uniq = {(x, z): (0, (x, 0, z), c) for _, (x, _, z), c in rows}
    check(one, list(uniq.values()), [0], False, 1, False, tmp_path, "mix_one")


def test_widest_key(tmp_path):
    """seven payload words: raw groups of 36, 36, 36 and 30 bases and a sample field; the order key takes seven words too"""
    S = 300
    groups = [36, 36, 36, 30]
    assert wrl.layout(groups, True)[1] == 7 and (wrl.order_bits(groups, S, True) + 63) // 64 == 7
    rng = random.Random(17)
    pool = ["".join(rng.choice("ACGTN") for _ in range(36)) for _ in range(3)] + ["N" * 36, "A" * 36]
    rows = [(rng.choice((0, 1, 255, 256, 299)), tuple(rng.choice(pool)[:g] for g in groups), rng.choice(COUNTS)) for _ in range(150)]
    rows = list({(s, f): (s, f, c) for s, f, c in rows}.values())
    check(groups, rows, [299], False, S, True, tmp_path, "widest_s", win=64, pad=0)
    check(groups, rows, [256, 0, 299, 1, 255], True, S, True, tmp_path, "widest_m", win=16, pad=2)
