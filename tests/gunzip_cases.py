"""The inputs of the span inflater's tests: the same scenarios go through the host build of the lane code
(test_gunzip_host.py, with sanitizers) and through the device (test_gpu_gunzip.py).  A scenario is a function of `run`:
run(src, start_bit, hist, capacity, part_bytes) -> (Result, text image of `capacity` bytes, 0xAA where nothing was
written) is one bc_gunzip_span_device call.  Every stream is made here with zlib; the expected text is zlib's own.
TEST-ONLY."""
import collections
import functools
import struct
import zlib

import inflate_cases

PART = 1024
OK, OUTPUT_FULL, BAD_STREAM = 0, 1, 2
Result = collections.namedtuple("Result", "status detail text_bytes end_bit member_end segments rejected crc32")
HISTORY = 32768


def pack_input(src, start_bit, hist, capacity, part_bytes):
    hist = hist or b""
    return struct.pack("<5Q", len(src), start_bit, len(hist), capacity, part_bytes) + hist + src


def unpack_output(raw):
    f = struct.unpack_from("<IIQQIIII", raw, 0)
    return Result(*f), raw[struct.calcsize("<IIQQIIII"):]


def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None, flush=zlib.Z_SYNC_FLUSH):
    """raw deflate stream (no header, no trailer)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if not flush_every:
        return c.compress(text) + c.flush()
    out = b""
    for i in range(0, len(text), flush_every):
        out += c.compress(text[i:i + flush_every]) + c.flush(flush)
    return out + c.flush()


def gzip_member(text, level=6, name=None, extra=None):
    flg = (8 if name else 0) | (4 if extra else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\x03"
    if extra:
        head += struct.pack("<H", len(extra)) + extra
    if name:
        head += name + b"\0"
    return head + deflate(text, level) + struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF)


def header_bytes(blob, at):
    """length of the gzip header at blob[at:], or None when there is none (or one this project refuses)"""
    if len(blob) - at < 10 or blob[at:at + 2] != b"\x1f\x8b" or blob[at + 2] != 8 or blob[at + 3] & 0xE0:
        return None
    flg, p = blob[at + 3], at + 10
    if flg & 4:
        p += 2 + struct.unpack_from("<H", blob, p)[0]
    for bit in (8, 16):
        if flg & bit:
            p = blob.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    return p - at


def history_of(text):
    """the 32 KiB before the next byte of a member whose text so far is `text` (None at its start)"""
    if not text:
        return None
    return (b"\0" * HISTORY + text)[-HISTORY:]


def gunzip_file(run, blob, span_bytes=None, capacity=None, part=PART):
    """A whole .gz file through spans, the way the ingest drives them -> (None | what went wrong, text, results)."""
    text, results, at = b"", [], 0
    while at < len(blob):
        hb = header_bytes(blob, at)
        if hb is None:
            break  # (trailing garbage is ignored, as zlib's gzread does)
        comp, bit, member, crc = at + hb, 0, b"", 0
        span = span_bytes or len(blob)
        while True:
            src = blob[comp:comp + span]
            cap = capacity or 1 << 22
            r, image = run(src, bit, history_of(member), cap, part)
            results.append(r)
            if r.status == OUTPUT_FULL:
                if r.text_bytes == 0:
                    return "a block larger than the text buffer", text, results
                cut = blob[comp:comp + (r.end_bit + 7) // 8]
                want = r
                r, image = run(cut, bit, history_of(member), cap, part)
                results.append(r)
                assert (r.status, r.text_bytes, r.end_bit) == (OK, want.text_bytes, want.end_bit), (want, r)
            if r.status != OK:
                return "bad stream (%s)" % r.detail, text, results
            assert image[r.text_bytes:] == b"\xAA" * (cap - r.text_bytes)
            assert r.crc32 == zlib.crc32(image[:r.text_bytes])
            member += image[:r.text_bytes]
            crc = zlib.crc32(image[:r.text_bytes], crc)
            if r.member_end:
                comp += (r.end_bit + 7) // 8
                break
            if r.end_bit == bit:  # no whole block in the span: more bytes, or none left
                if comp + span >= len(blob):
                    return "the stream ends inside a block", text, results
                span *= 2
                continue
            comp, bit = comp + r.end_bit // 8, r.end_bit % 8
        if len(blob) - comp < 8:
            return "no trailer", text, results
        want_crc, want_len = struct.unpack_from("<II", blob, comp)
        text += member
        if (want_crc, want_len) != (crc, len(member) & 0xFFFFFFFF):
            return "trailer mismatch", text, results
        at = comp + 8
    return None, text, results


def whole(run, stream, text, part=PART):
    """a member's whole deflate stream (plus a trailer's worth of bytes) as one span"""
    cap = len(text) + 16
    r, image = run(stream + b"\0" * 8, 0, None, cap, part)
    assert r.status == OK and r.member_end == 1, r
    assert r.text_bytes == len(text) and image[:len(text)] == text
    assert image[len(text):] == b"\xAA" * 16
    assert (r.end_bit + 7) // 8 == len(stream) and r.crc32 == zlib.crc32(text)
    return r


@functools.lru_cache(maxsize=None)
def fastq(n_bytes, seed=1):
    return inflate_cases.fastq_text(n_bytes, seed=seed)


def level_case(level):
    def scenario(run):
        text = fastq(300000, seed=level + 1)
        r = whole(run, deflate(text, level), text)
        assert r.segments >= 2, r
    return scenario


def fixed_blocks(run):
    text = fastq(60000, seed=5)
    r = whole(run, deflate(text, 6, zlib.Z_FIXED), text)
    assert r.segments == 1, r  # (fixed blocks are never searched for)


def stored_only(run):
    text = fastq(300000, seed=6)
    r = whole(run, deflate(text, 0), text)
    assert r.segments == 1, r  # no candidate at all that the chain lands on


SYNC_EVERY = 3000


def sync_flush(run):
    text = fastq(300000, seed=7)
    r = whole(run, deflate(text, 6, flush_every=SYNC_EVERY), text)
    flushes = (len(text) + SYNC_EVERY - 1) // SYNC_EVERY
    assert 2 * r.segments >= flushes, (r, flushes)


def run_of_one_byte(run):
    """100 KB of one byte, flushed every 3 KB: distance 1, length 258, from a block's first symbol on.  (zlib writes such
    blocks with the fixed code, which is not searched for: see interrupted_runs for the same across segment starts.)"""
    text = b"A" * 100000
    r = whole(run, deflate(text, 6, flush_every=SYNC_EVERY), text)
    assert r.segments >= 1, r


def interrupted_runs(run):
    # runs with a little FASTQ between them, so that zlib writes dynamic blocks: blocks, and with them segments, begin
    # in the middle of a run: distance 1, length 258, reaching before a segment's start
    text = b"".join(b"A" * 5000 + fastq(12000, seed=8)[200 * i:200 * i + 200] for i in range(20))
    assert len(text) >= 100000
    r = whole(run, deflate(text, 6, flush_every=SYNC_EVERY), text)
    assert r.segments >= 4, r


def far_distances(run):
    """matches at distance exactly 32768 and 32769 - 258 from a segment that does not hold their source: zlib's deflate
    never reaches that far, so the last block is written by hand (fixed code)"""
    first = fastq(40000, seed=9)
    a = inflate_cases.Bits()
    a.header(0, 1)
    for ch in first:
        a.lit(ch)
    a.lit(256)
    a.stored(0, b"")  # (to a byte boundary)
    middle = fastq(6000, seed=10)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    b = c.compress(middle) + c.flush(zlib.Z_FULL_FLUSH)
    t = inflate_cases.Bits()
    t.header(1, 1)
    t.match(258, 32768)
    t.match(258, 32769 - 258)
    t.match(100, 32768)
    t.lit(ord("\n"))
    t.lit(256)
    t.align()
    stream = bytes(a.out) + b + bytes(t.out)
    text = zlib.decompress(stream, -15)
    assert len(text) == 40000 + 6000 + 258 + 258 + 100 + 1
    r = whole(run, stream, text)
    assert r.segments >= 2, r


def stream_inside_a_stored_block(run):
    """a stored block whose payload is a valid dynamic deflate stream: candidates the chain walks past"""
    inner = deflate(fastq(40000, seed=11), 6, flush_every=8000)  # (non-final dynamic blocks: BFINAL = 0 is searched for)
    assert 3000 < len(inner) < 60000
    head = fastq(30000, seed=12)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    first = c.compress(head) + c.flush(zlib.Z_FULL_FLUSH)
    s = inflate_cases.Bits()
    s.stored(0, inner)
    tail = fastq(30000, seed=13)
    stream = first + bytes(s.out) + deflate(tail, 6)
    text = head + inner + tail
    assert zlib.decompress(stream, -15) == text
    r = whole(run, stream, text)
    assert r.rejected >= 1, r


def cut_and_continue(run):
    """a span cut in the middle of a block ends at its last whole block; the next one starts there, at a bit offset that
    is no byte boundary, with the 32 KiB before it as history"""
    text = fastq(300000, seed=14)
    stream = deflate(text, 6) + b"\0" * 8
    cut = len(stream) * 2 // 3
    r, image = run(stream[:cut], 0, None, len(text), PART)
    assert r.status == OK and not r.member_end and 0 < r.text_bytes < len(text) and r.end_bit <= 8 * cut, r
    assert image[:r.text_bytes] == text[:r.text_bytes] and r.crc32 == zlib.crc32(text[:r.text_bytes])
    got, bit, at, unaligned = image[:r.text_bytes], r.end_bit % 8, r.end_bit // 8, 0
    for upto in (cut + (len(stream) - cut) // 2, len(stream)):  # twice: the second history is all markers' business
        unaligned += bit != 0
        r, image = run(stream[at:upto], bit, history_of(got), len(text) - len(got) + 5, PART)
        assert r.status == OK and r.text_bytes > 0, r
        assert image[:r.text_bytes] == text[len(got):len(got) + r.text_bytes]
        assert image[r.text_bytes:] == b"\xAA" * (len(image) - r.text_bytes)
        got += image[:r.text_bytes]
        at, bit = at + r.end_bit // 8, r.end_bit % 8
    assert r.member_end == 1 and got == text and unaligned >= 1


def two_members(run):
    a, b = fastq(90000, seed=15), fastq(70000, seed=16)
    blob = gzip_member(a, 6) + gzip_member(b, 9, name=b"reads.fastq", extra=b"XY\x02\x00ab")
    err, text, results = gunzip_file(run, blob)
    assert err is None and text == a + b
    assert [r.member_end for r in results] == [1, 1]
    err, text, results = gunzip_file(run, blob, span_bytes=8192)  # (and through spans that end inside blocks)
    assert err is None and text == a + b and len(results) > 4


def one_byte_short(run):
    text = fastq(300000, seed=17)
    stream = deflate(text, 6) + b"\0" * 8
    r, image = run(stream, 0, None, len(text) - 1, PART)
    assert r.status == OUTPUT_FULL and 0 < r.text_bytes < len(text) - 1 and not r.member_end, r
    assert image == b"\xAA" * len(image)  # nothing is written
    r2, image = run(stream[:(r.end_bit + 7) // 8], 0, None, len(text) - 1, PART)
    assert (r2.status, r2.text_bytes, r2.end_bit, r2.member_end) == (OK, r.text_bytes, r.end_bit, 0), (r, r2)
    assert image[:r2.text_bytes] == text[:r2.text_bytes]
    blob = gzip_member(text, 6)
    err, got, results = gunzip_file(run, blob, capacity=120000)  # the ingest's way: cut, then go on from there
    assert err is None and got == text and any(x.status == OUTPUT_FULL for x in results)


def damaged(where):
    def scenario(run):
        text = fastq(150000, seed=18)
        blob = bytearray(gzip_member(text, 6))
        at = {"header": 10 * 8 + 9, "distance": 8 * (len(blob) // 2) + 3, "trailer": 8 * (len(blob) - 7) + 2}[where]
        blob[at // 8] ^= 1 << (at % 8)
        for span in (None, 8192):
            err, got, results = gunzip_file(run, bytes(blob), span_bytes=span)
            assert err is not None, where
            if where == "trailer":
                assert err == "trailer mismatch" and got == text
    return scenario


def cases():
    out = [("level_%d" % lv, level_case(lv)) for lv in (1, 6, 9)]
    out += [("fixed_blocks", fixed_blocks), ("stored_only", stored_only), ("sync_flush", sync_flush),
            ("run_of_one_byte", run_of_one_byte), ("interrupted_runs", interrupted_runs), ("far_distances", far_distances),
            ("stream_inside_a_stored_block", stream_inside_a_stored_block), ("cut_and_continue", cut_and_continue),
            ("two_members", two_members), ("one_byte_short", one_byte_short)]
    out += [("damaged_" + w, damaged(w)) for w in ("header", "distance", "trailer")]
    return out
