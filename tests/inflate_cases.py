"""The inputs of the inflater tests: the same tables go through the host build of the decoder (test_inflate_emulation.py,
with sanitizers) and through the device (test_gpu_inflate.py).  A case is a table of blocks; a block is
(deflate stream, ISIZE, CRC32, expected text | None when the block is damaged and must be flagged).  TEST-ONLY."""
import random
import struct
import zlib

import bgzf


def fastq_text(n_bytes, seed=1, read_len=(80, 151)):
    rng = random.Random(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        n = rng.randint(*read_len)
        rec = "@M0%d:%d:000-FC%d:1:%d:%d:%d 1:N:0:%d\n%s\n+\n%s\n" % (
            seed, rng.randint(1, 99), seed, 1101 + i % 7, rng.randint(1000, 29999), rng.randint(1000, 29999), i % 97,
            "".join(rng.choice("ACGT" if rng.random() > 0.01 else "N") for _ in range(n)),
            "".join(chr(33 + min(40, max(2, int(rng.gauss(34, 6))))) for _ in range(n)))
        out.append(rec)
        size += len(rec)
        i += 1
    return "".join(out).encode()[:n_bytes]


class Bits:
    """deflate bit writer with the fixed Huffman code, for streams zlib's deflate never writes"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):  # least significant bit first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):  # Huffman codes go most significant bit first
        self.put(int(format(value, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def header(self, final, btype):
        self.put(final, 1)
        self.put(btype, 2)

    def stored(self, final, data, nlen=None):
        self.header(final, 0)
        self.align()
        self.put(len(data), 16)
        self.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += data

    def lit(self, sym):  # literal/length symbol of the fixed code
        if sym < 144:
            self.code(0x30 + sym, 8)
        elif sym < 256:
            self.code(0x190 + sym - 144, 9)
        elif sym < 280:
            self.code(sym - 256, 7)
        else:
            self.code(0xC0 + sym - 280, 8)

    def match(self, length, dist):
        lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
        lext = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
        dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                 6145, 8193, 12289, 16385, 24577]
        dext = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
        ls = max(i for i in range(29) if lbase[i] <= length) if length < 258 else 28
        self.lit(257 + ls)
        self.put(length - lbase[ls], lext[ls])
        ds = max(i for i in range(30) if dbase[i] <= dist)
        self.code(ds, 5)
        self.put(dist - dbase[ds], dext[ds])

    def done(self):
        self.align()
        return bytes(self.out)


def good(data, payload=None, **kw):
    if payload is None:
        payload = bgzf.deflate_raw(data, **kw)
    assert zlib.decompress(payload, -15) == data
    return (payload, len(data), zlib.crc32(data), data)


def bad(payload, isize, crc):
    return (payload, isize, crc, None)


def zlib_rejects(payload, data):
    """zlib's view of a damaged stream: an error, an unfinished stream, or other bytes than `data`"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload) + d.flush()
    except zlib.error:
        return True
    return not d.eof or out != data


def cases():
    rng = random.Random(20240607)
    text = fastq_text(65280, seed=3)
    randbytes = bytes(rng.getrandbits(8) for _ in range(65280))
    out = []
    for level in (0, 1, 6, 9):
        out.append(("fastq_level%d" % level, [good(text, level=level)]))
    out.append(("fastq_fixed", [good(text[:30000], strategy=zlib.Z_FIXED)]))
    out.append(("identical_bytes", [good(b"G" * 65280)]))
    out.append(("period3", [good(b"ACG" * (65280 // 3))]))
    out.append(("period70", [good((text[:70] * 933)[:65280])]))
    out.append(("random_level6", [good(randbytes)]))
    out.append(("sizes_0_1_2_65280", [good(b""), good(b"A"), good(b"A\n"), good(text), good(b"", level=0), good(b"x", level=0)]))
    half = len(text) // 2
    out.append(("sync_and_full_flush", [good(text, flush_at=[(half // 2, zlib.Z_SYNC_FLUSH), (half, zlib.Z_FULL_FLUSH),
                                                              (half, zlib.Z_SYNC_FLUSH)])]))
    # a match of 258 bytes that begins exactly 32768 bytes back (zlib's deflate stops at 32506: written by hand)
    b = Bits()
    b.stored(0, randbytes[:32768])
    b.header(1, 1)
    b.match(258, 32768)
    b.match(3, 32768)
    b.lit(ord("!"))
    b.match(258, 1)
    b.lit(256)
    far = randbytes[:32768] + randbytes[:258] + randbytes[258:261] + b"!" * 259
    out.append(("distance_32768", [good(far, payload=b.done())]))
    small = [fastq_text(700, seed=100 + i) for i in range(50)]
    out.append(("table_of_5000", [good(small[i % 50], level=(1, 6, 9)[i % 3]) for i in range(5000)]))

    # damaged blocks, each between two good neighbours that must still come out right
    nb1, nb2 = good(text[:5000]), good(text[5000:9000], level=1)
    part = text[:20000]
    pay = bgzf.deflate_raw(part)
    crc = zlib.crc32(part)

    def damaged(name, blk):
        out.append((name, [nb1, blk, nb2]))

    damaged("wrong_crc", bad(pay, len(part), crc ^ 0x00010000))
    damaged("isize_too_small", bad(pay, len(part) - 1, crc))
    damaged("isize_too_large", bad(pay, len(part) + 1, crc))
    damaged("payload_cut_short", bad(pay[:-5], len(part), crc))
    damaged("payload_empty", bad(b"", len(part), crc))
    damaged("btype3", bad(b"\x07" + pay[1:], len(part), crc))
    b = Bits()
    b.stored(1, b"ACGTN", nlen=(5 ^ 0xFFFF) ^ 0x0100)
    damaged("stored_len_nlen", bad(b.done(), 5, zlib.crc32(b"ACGTN")))
    b = Bits()
    b.header(1, 1)
    b.lit(ord("A"))
    b.match(3, 2)  # one byte made so far: reaches into the neighbour's text, were it followed
    b.lit(256)
    damaged("distance_before_start", bad(b.done(), 4, zlib.crc32(b"AAAA")))
    b = Bits()
    b.header(1, 1)
    b.match(258, 32768)
    b.lit(256)
    damaged("distance_before_start_far", bad(b.done(), 258, 0))
    # Single-bit flips in a dynamic-Huffman stream.  The flipped bit is drawn from every byte but the stream's last: that
    # byte may end in padding bits, which belong to no code and to no byte of the text, so that no inflater could tell.
    assert (pay[0] >> 1) & 3 == 2
    for k in range(32):
        bit = rng.randrange(8 * (len(pay) - 1))
        flipped = bytearray(pay)
        flipped[bit >> 3] ^= 1 << (bit & 7)
        assert zlib_rejects(bytes(flipped), part)
        damaged("bit_flip_%d_at_%d" % (k, bit), bad(bytes(flipped), len(part), crc))
    return out


def layout(blocks, src_gap=3, dst_gap=7):
    """-> (src bytes, [(src_off, dst_off, src_len, isize, crc)], dst_bytes): the blocks laid out with gaps between them"""
    src, table, dst_off = bytearray(b"\x55" * src_gap), [], dst_gap
    for payload, isize, crc, _ in blocks:
        table.append((len(src), dst_off, len(payload), isize, crc))
        src += payload + b"\x55" * src_gap
        dst_off += isize + dst_gap
    return bytes(src), table, dst_off


def check(name, blocks, table, status, dst):
    """status words and output image of a run against the case"""
    for i, ((payload, isize, crc, expect), (_, dst_off, _, _, _)) in enumerate(zip(blocks, table)):
        if expect is None:
            assert status[i] != 0, "%s: damaged block %d passed" % (name, i)
        else:
            assert status[i] == 0, "%s: good block %d got status %d" % (name, i, status[i])
            assert bytes(dst[dst_off:dst_off + isize]) == expect, "%s: block %d differs from zlib" % (name, i)


def pack(src, table, dst_bytes):
    """the input file of tests/inflate/inflate_host"""
    return (struct.pack("<QQQ", len(table), len(src), dst_bytes) +
            b"".join(struct.pack("<QQIIII", so, do, sl, isz, crc, 0) for so, do, sl, isz, crc in table) + src)
