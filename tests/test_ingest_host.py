"""The host-only logic of the FASTQ ingest (csrc/bc_fastq_host.hpp): the gzip member header, the first-record check, the
end-of-stream rules, the cut of a BGZF index into chunks and shards, and the shard scanner on a truncated file.  It runs in
tests/ingest/ingest_host, a stand-alone program built with sanitizers (ingest_lib.py); every expected value is worked
out here, without the C++."""
import bisect
import random
import struct

import pytest

import ingest_lib


# ---- gzip_member_header

def gzip_header(fextra, fname, fcomment, fhcrc, cm=8, magic=b"\x1f\x8b", more_flags=0):
    flg = 4 * fextra | 8 * fname | 16 * fcomment | 2 * fhcrc | more_flags
    h = magic + bytes([cm, flg]) + b"\0\0\0\0" + b"\0\3"
    if fextra:
        h += struct.pack("<H", 5) + b"ab\0cd"   # (a zero byte inside the field: not a terminator)
    if fname:
        h += b"reads.fastq\0"
    if fcomment:
        h += b"a comment\0"
    if fhcrc:
        h += b"\x12\x34"
    return h


PAYLOAD = bytes(range(1, 21))   # 20 bytes behind the header, none of them zero


def test_gzip_member_header_on_every_prefix_of_every_flag_combination(tmp_path):
    queries, expected = [], []
    for bits in range(16):
        h = gzip_header(bits & 1, bits >> 1 & 1, bits >> 2 & 1, bits >> 3 & 1)
        blob = h + PAYLOAD
        for n in range(len(blob) + 1):
            for file_end in (0, 1):
                queries.append("header %d %s" % (file_end, ingest_lib.hexed(blob[:n])))
                expected.append(len(h) if n >= len(h) else -1 if file_end else 0)
    got = [int(a) for a in ingest_lib.ask(tmp_path, queries)]
    assert got == expected


def test_gzip_member_header_refuses_what_is_not_a_deflate_member(tmp_path):
    cases = [(gzip_header(0, 0, 0, 0, magic=b"\x1f\x8c"), -1), (gzip_header(0, 1, 0, 0, magic=b"BZ"), -1),
             (gzip_header(0, 0, 0, 0, cm=7), -2), (gzip_header(1, 1, 0, 0, cm=9), -2)]
    cases += [(gzip_header(0, 1, 0, 0, more_flags=bit), -2) for bit in (0x20, 0x40, 0x80)]
    queries = ["header %d %s" % (file_end, ingest_lib.hexed(h + PAYLOAD)) for h, _ in cases for file_end in (0, 1)]
    got = [int(a) for a in ingest_lib.ask(tmp_path, queries)]
    assert got == [want for _, want in cases for _ in (0, 1)]


# ---- first_record_check

def looks_like_sequence(line):
    return not sum(c in b"AGCTN" for c in line) < len(line) // 2


def first_record_model(text, eof, gz_rules):
    """0 ok (or not looked at), 1 the first line is a sequence, 2 the second line is not"""
    *whole, rest = text.split(b"\n")
    if len(whole) < 3 or not (len(whole) >= 4 or (eof and not gz_rules and len(whole) == 3 and rest)):
        return 0
    l1, l2 = whole[0], whole[1]
    if not gz_rules:
        l1, l2 = (l[:-1] if l.endswith(b"\r") else l for l in (l1, l2))
    return 1 if looks_like_sequence(l1) else 0 if looks_like_sequence(l2) else 2


def crlf(text):
    return text.replace(b"\n", b"\r\n")


GOOD = b"@read1 x\nACGTACGT\n+\nIIIIIIII\n"
DNA_FIRST = b"ACGTACGT\nACGTACGT\n+\nIIIIIIII\n"
SECOND_NOT_DNA = b"@read1 x\n########\n+\nIIIIIIII\n"
# lines whose verdict a kept '\r' changes: "@A#" is half DNA, "@A#\r" is not; "A#x" likewise
CR_FIRST = b"@A#\r\nACGT\r\n+\r\nIIII\r\n"
CR_SECOND = b"@read1 x\r\nA#x\r\n+\r\nIII\r\n"
# (text, eof, gz_rules, expected)
FIRST_RECORD_CASES = [
    (GOOD, 0, 0, 0), (DNA_FIRST, 0, 0, 1), (SECOND_NOT_DNA, 0, 0, 2),
    (GOOD, 1, 1, 0), (DNA_FIRST, 1, 1, 1), (SECOND_NOT_DNA, 1, 1, 2),
    (crlf(GOOD), 0, 0, 0), (crlf(DNA_FIRST), 0, 0, 1), (crlf(SECOND_NOT_DNA), 0, 0, 2),
    (CR_FIRST, 0, 0, 1), (CR_FIRST, 0, 1, 0),      # plain rules trim the CR, gz rules keep it
    (CR_SECOND, 0, 0, 0), (CR_SECOND, 0, 1, 2),
    (DNA_FIRST[:DNA_FIRST.index(b"IIII")], 0, 0, 0), (DNA_FIRST[:DNA_FIRST.index(b"IIII")], 1, 0, 0),   # three lines only: not looked at
    (DNA_FIRST[:DNA_FIRST.index(b"IIII")], 1, 1, 0),
    # four lines, the last without its newline: a record only at the end of a plain file
    (DNA_FIRST[:-1], 1, 0, 1), (DNA_FIRST[:-1], 0, 0, 0), (DNA_FIRST[:-1], 1, 1, 0), (DNA_FIRST[:-1], 0, 1, 0),
    (SECOND_NOT_DNA[:-1], 1, 0, 2), (SECOND_NOT_DNA[:-1], 1, 1, 0),
    (b"", 1, 0, 0), (b"\n\n\n\n", 0, 0, 1),   # (an empty line counts as a sequence: parse.rs:414-427)
]


def test_first_record_check(tmp_path):
    for text, eof, gz_rules, want in FIRST_RECORD_CASES:
        assert first_record_model(text, eof, gz_rules) == want, (text, eof, gz_rules)
    queries = ["first %d %d %s" % (eof, gz_rules, ingest_lib.hexed(text)) for text, eof, gz_rules, _ in FIRST_RECORD_CASES]
    got = [int(a) for a in ingest_lib.ask(tmp_path, queries)]
    assert got == [want for *_, want in FIRST_RECORD_CASES]


# ---- stream_tail

# (seen, gz_end) -> (extra_total, post_partial_record):
#   extra_total = (seen is 1, 2 or 3) + (gz_end and seen % 4 == 0),  post_partial_record = gz_end and seen == 3
STREAM_TAIL = {(0, 0): (0, 0), (1, 0): (1, 0), (2, 0): (1, 0), (3, 0): (1, 0),
               (0, 1): (1, 0), (1, 1): (1, 0), (2, 1): (1, 0), (3, 1): (1, 1)}


def test_stream_tail(tmp_path):
    keys = sorted(STREAM_TAIL)
    got = [tuple(int(x) for x in a.split()) for a in ingest_lib.ask(tmp_path, ["tail %d %d" % k for k in keys])]
    assert got == [STREAM_TAIL[k] for k in keys]


# ---- bgzf_next_run, bgzf_shard_members

def member_lists():
    """lists of 200 (isize, total) blocks: text sizes from {0, 1, 700, 65280}, with runs of empty blocks"""
    out = []
    for seed in (1, 2, 3):
        rng = random.Random(seed)
        sizes = []
        while len(sizes) < 200:
            isize = rng.choice((0, 1, 700, 700, 65280))
            sizes += [isize] * (rng.randint(2, 9) if isize == 0 and rng.random() < 0.5 else 1)
        out.append([(isize, 28 + isize // 3) for isize in sizes[:200]])
    out.append([(0, 28)] * 200)
    return out


def members_query(blocks):
    return "members %d %s" % (len(blocks), " ".join("%d %d" % b for b in blocks))


def runs_model(blocks, start, end, fill_cap, chunk, blk_cap):
    runs = []
    while start < end:
        upto, text, comp = start, 0, 0
        while upto < end:
            isize, total = blocks[upto]
            if upto > start and (text + isize > fill_cap or comp + total > chunk or upto - start >= blk_cap):
                break
            upto, text, comp = upto + 1, text + isize, comp + total
        runs.append((upto, text, comp))
        start = upto
    return runs


# (fill_cap, chunk, blk_cap): roomy; fill_cap below one block; one block a run; bound by compressed bytes; three blocks
RUN_SETTINGS = [(1 << 20, 1 << 20, 4160), (4096, 65552, 80), (200000, 70000, 1), (1 << 20, 40000, 1000), (3000, 1 << 20, 3)]


def test_bgzf_next_run_tiles_the_index(tmp_path):
    queries, asked = [], []
    for blocks in member_lists():
        queries.append(members_query(blocks))
        asked.append(None)
        for fill_cap, chunk, blk_cap in RUN_SETTINGS:
            for start, end in ((0, 200), (17, 150), (199, 200)):
                queries.append("runs %d %d %d %d %d" % (start, end, fill_cap, chunk, blk_cap))
                asked.append((blocks, start, end, fill_cap, chunk, blk_cap))
    answers = ingest_lib.ask(tmp_path, queries)
    for a, q in zip(answers, asked):
        if q is None:
            continue
        blocks, start, end, fill_cap, chunk, blk_cap = q
        nums = [int(x) for x in a.split()]
        runs = list(zip(nums[0::3], nums[1::3], nums[2::3]))
        at = start
        for upto, text, comp in runs:
            assert upto > at, "an empty run"
            assert text == sum(b[0] for b in blocks[at:upto]) and comp == sum(b[1] for b in blocks[at:upto])
            if upto - at > 1:
                assert text <= fill_cap and comp <= chunk and upto - at <= blk_cap
            at = upto
        assert at == end, "the runs leave a gap"
        assert runs == runs_model(blocks, start, end, fill_cap, chunk, blk_cap)


def test_bgzf_shard_members_cover_the_shard(tmp_path):
    queries, asked = [], []
    for blocks in member_lists()[:3]:
        queries.append(members_query(blocks))
        asked.append(None)
        starts = [0]
        for isize, _ in blocks:
            starts.append(starts[-1] + isize)
        inflated = starts.pop()
        rng = random.Random(len(queries))
        big = [k for k, b in enumerate(blocks) if b[0] >= 700]
        # offsets on block starts (those of empty blocks among them) and inside blocks
        marks = sorted({0, inflated} | {starts[k] for k in rng.sample(range(200), 12)} | {starts[k] + rng.randint(1, 699) for k in rng.sample(big, 12)})
        for n_shards in (1, 2, 3, 4):
            for shard in range(n_shards):
                pairs = [tuple(sorted(rng.sample(marks, 2))) for _ in range(12)] + [(marks[5], marks[5]), (0, inflated)]
                for text_a, text_b in pairs:
                    queries.append("shard %d %d %d %d" % (text_a, text_b, shard, n_shards))
                    asked.append((blocks, starts, text_a, text_b, shard, n_shards))
    answers = ingest_lib.ask(tmp_path, queries)
    for a, q in zip(answers, asked):
        if q is None:
            continue
        blocks, starts, text_a, text_b, shard, n_shards = q
        first, end = (int(x) for x in a.split())
        assert 0 <= first <= end <= len(blocks), q[2:]
        # the blocks that hold a byte of [text_a, text_b)
        holding = [k for k in range(len(blocks)) if max(starts[k], text_a) < min(starts[k] + blocks[k][0], text_b)]
        assert all(first <= k < end for k in holding), q[2:]
        if shard == 0:
            assert first == 0
        if shard + 1 == n_shards:
            assert end == len(blocks)   # (the last shard also takes the empty blocks that end the file)
        elif text_a == text_b:
            assert first == end, q[2:]
        else:
            # nothing before the block that holds text_a, nothing from the first block that starts at or after text_b on
            assert end == bisect.bisect_left(starts, text_b)
        if shard != 0:
            assert first == bisect.bisect_right(starts, text_a) - 1


# ---- record_start_at_or_after

def test_record_start_gives_up_when_a_read_delivers_nothing(tmp_path):
    """(a file truncated between measuring it and reading it.)  The answer is -1 and the scanner stops asking: at the
    first read, and at a later one -- the scanner reads 1 MiB a time, and a stretch without a newline makes it read on"""
    queries = ["start_empty 100 1000 0", "start_empty 1 2 0", "start_empty 100 %d 1" % (3 << 20), "start_empty 100 %d 2" % (3 << 20)]
    assert ingest_lib.ask(tmp_path, queries) == ["-1 1", "-1 1", "-1 2", "-1 3"]
