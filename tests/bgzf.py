"""A BGZF writer on the standard zlib module (no bgzip needed), and a reader of its member headers.  TEST-ONLY."""
import struct
import zlib

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def deflate_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    """raw deflate stream of data; flush_at: [(offset, zlib.Z_SYNC_FLUSH | Z_FULL_FLUSH), ...] flushes in the middle"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = [], 0
    for off, mode in flush_at:
        out.append(c.compress(data[at:off]))
        out.append(c.flush(mode))
        at = off
    out.append(c.compress(data[at:]))
    out.append(c.flush())
    return b"".join(out)


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, extra_before=b"", extra_after=b"", payload=None, isize=None,
           crc=None):
    """one BGZF member; payload / isize / crc override what the data gives (for damaged members)"""
    if payload is None:
        payload = deflate_raw(data, level, strategy)
    extra = extra_before + b"BC" + struct.pack("<H", 2) + b"\0\0" + extra_after
    total = 12 + len(extra) + len(payload) + 8
    assert total <= 65536, total
    extra = extra_before + b"BC" + struct.pack("<HH", 2, total - 1) + extra_after
    head = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\x00\xff" + struct.pack("<H", len(extra)) + extra
    return head + payload + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def compress(data, block_size=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof_marker=True):
    out = [member(data[i:i + block_size], level, strategy) for i in range(0, len(data), block_size)]
    if eof_marker:
        out.append(EOF_MARKER)
    return b"".join(out)


def write(path, data, **kw):
    with open(path, "wb") as f:
        f.write(compress(data, **kw))


def members(blob):
    """[(file offset, payload offset, payload length, crc32, isize)] of a BGZF blob (trusting it)"""
    out, off = [], 0
    while off < len(blob):
        xlen = struct.unpack_from("<H", blob, off + 10)[0]
        x, bsize = 0, None
        while x < xlen:
            si, slen = blob[off + 12 + x:off + 14 + x], struct.unpack_from("<H", blob, off + 14 + x)[0]
            if si == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", blob, off + 16 + x)[0]
            x += 4 + slen
        total = bsize + 1
        crc, isize = struct.unpack_from("<II", blob, off + total - 8)
        out.append((off, off + 12 + xlen, total - 12 - xlen - 8, crc, isize))
        off += total
    return out
