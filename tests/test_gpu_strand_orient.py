"""bc_strand_orient_device against the Python rc(): every byte value, the lengths around the dword and wave edges, strides
that are and are not multiples of 4, fixed and ragged batches, quality lines shorter and longer than their sequence
lines, index lists that repeat, skip and reorder, the padding, and the bytes around the output."""
import numpy as np
import pytest

import strand_cases

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 64  # poisoned bytes kept on either side of every output buffer


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def expect_line(line, n, pad, complement):
    body = bytes(line[:n])
    body = strand_cases.rc_seq(body) if complement else body[::-1]
    return np.frombuffer(body + bytes([pad]) * (len(line) - n), dtype=np.uint8)


def orient(seq, qual, stride, read_len=0, lens=None, qlens=None, index=None, n_out=None):
    """runs the kernel on host arrays; -> (seq_out, qual_out, lens_out, qlens_out), the guards checked"""
    import torch
    pkg = _pkg()
    n_out = len(index) if index is not None else (seq.size // stride if n_out is None else n_out)
    dev = lambda a, t=None: None if a is None else torch.from_numpy(a if t is None else a.view(t)).cuda()
    d_seq, d_qual = dev(seq.reshape(-1)), dev(None if qual is None else qual.reshape(-1))
    d_lens, d_qlens = dev(lens, np.int16), dev(qlens, np.int16)
    d_index = dev(None if index is None else np.asarray(index, dtype=np.uint32), np.int32)
    # 16-byte aligned outputs inside poisoned buffers (GUARD is a multiple of 16; torch allocations are 256-aligned)
    out = lambda nbytes: torch.full((nbytes + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
    o_seq, o_qual = out(n_out * stride), (out(n_out * stride) if qual is not None else None)
    o_lens, o_qlens = (out(n_out * 2) if lens is not None else None), (out(n_out * 2) if qlens is not None else None)
    ptr = lambda t, off=0: None if t is None else t.data_ptr() + off
    torch.cuda.synchronize()
    pkg.orient_device(ptr(d_seq), ptr(d_qual), stride, read_len, n_out, ptr(o_seq, GUARD), ptr(o_qual, GUARD), d_lens=ptr(d_lens),
                      d_qlens=ptr(d_qlens), d_index=ptr(d_index), d_lens_out=ptr(o_lens, GUARD), d_qlens_out=ptr(o_qlens, GUARD))
    torch.cuda.synchronize()
    res = []
    for t, nbytes in ((o_seq, n_out * stride), (o_qual, n_out * stride), (o_lens, n_out * 2), (o_qlens, n_out * 2)):
        if t is None:
            res.append(None)
            continue
        h = t.cpu().numpy()
        assert (h[:GUARD] == POISON).all() and (h[GUARD + nbytes:] == POISON).all(), "wrote outside its output"
        res.append(h[GUARD:GUARD + nbytes])
    res[0] = res[0].reshape(n_out, stride)
    if res[1] is not None:
        res[1] = res[1].reshape(n_out, stride)
    for k in (2, 3):
        if res[k] is not None:
            res[k] = res[k].view(np.uint16)
    return res


def check(seq, qual, stride, got, read_len=0, lens=None, qlens=None, index=None):
    g_seq, g_qual, g_lens, g_qlens = got
    src = index if index is not None else range(len(g_seq))
    for j, i in enumerate(src):
        n = int(lens[i]) if lens is not None else read_len
        qn = int(qlens[i]) if qlens is not None else n
        assert (g_seq[j] == expect_line(seq[i], n, strand_cases.PAD_SEQ, True)).all(), (j, i, n, bytes(g_seq[j]), bytes(seq[i]))
        if qual is not None:
            assert (g_qual[j] == expect_line(qual[i], qn, strand_cases.PAD_QUAL, False)).all(), (j, i, qn)
        if lens is not None:
            assert g_lens[j] == lens[i]
        if qlens is not None:
            assert g_qlens[j] == qlens[i]


def edge_lengths(stride):
    return sorted({v for v in (0, 1, 2, 3, 4, 5, 63, 64, 65, stride - 1, stride) if 0 <= v <= stride})


def test_all_byte_values_in_one_read():
    seq = np.arange(256, dtype=np.uint8).reshape(1, 256)
    qual = np.arange(256, dtype=np.uint8)[::-1].copy().reshape(1, 256)
    got = orient(seq, qual, 256, read_len=256)
    check(seq, qual, 256, got, read_len=256)
    assert bytes(got[0][0]) == strand_cases.rc_seq(bytes(range(256)))


@pytest.mark.parametrize("stride", [16, 100, 321])
def test_fixed_length_batches(stride):
    rng = np.random.default_rng(stride)
    for read_len in edge_lengths(stride):
        n = 67
        seq = rng.integers(0, 256, (n, stride), dtype=np.uint8)
        qual = rng.integers(33, 127, (n, stride), dtype=np.uint8)
        check(seq, qual, stride, orient(seq, qual, stride, read_len=read_len), read_len=read_len)
    seq = rng.integers(0, 256, (5, stride), dtype=np.uint8)  # (no quality buffer at all)
    check(seq, None, stride, orient(seq, None, stride, read_len=stride), read_len=stride)


@pytest.mark.parametrize("stride", [16, 100, 321])
@pytest.mark.parametrize("with_qlens", [False, True])
def test_ragged_batches(stride, with_qlens):
    """every edge length somewhere in the batch; with_qlens: quality lines shorter and longer than their sequence lines"""
    rng = np.random.default_rng(1000 + stride)
    edges = edge_lengths(stride)
    n = 300
    lens = np.array([edges[i % len(edges)] if i < 4 * len(edges) else rng.integers(0, stride + 1) for i in range(n)], dtype=np.uint16)
    qlens = None
    if with_qlens:
        qlens = np.array([edges[(i // len(edges)) % len(edges)] if i < 4 * len(edges) else rng.integers(0, stride + 1) for i in range(n)],
                         dtype=np.uint16)
        assert (qlens < lens).any() and (qlens > lens).any()
    seq = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    qual = rng.integers(33, 127, (n, stride), dtype=np.uint8)
    check(seq, qual, stride, orient(seq, qual, stride, lens=lens, qlens=qlens), lens=lens, qlens=qlens)


@pytest.mark.parametrize("n_out", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("stride", [16, 100, 321])
def test_index_lists(n_out, stride):
    """lists that repeat, skip and reorder the reads of a 90-read ragged batch"""
    rng = np.random.default_rng(n_out * 1000 + stride)
    n = 90
    lens = rng.integers(0, stride + 1, n).astype(np.uint16)
    qlens = rng.integers(0, stride + 1, n).astype(np.uint16)
    seq = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    qual = rng.integers(33, 127, (n, stride), dtype=np.uint8)
    index = rng.integers(0, n, n_out)
    index[0] = n - 1  # the batch's last read first
    if n_out > 2:
        index[1] = index[2] = 0  # a repeat
    check(seq, qual, stride, orient(seq, qual, stride, lens=lens, qlens=qlens, index=index), lens=lens, qlens=qlens, index=index)
    # ... and of a fixed-length one
    check(seq, qual, stride, orient(seq, qual, stride, read_len=stride - 1, index=index), read_len=stride - 1, index=index)


def test_in_order_prefix_and_refusals():
    pkg = _pkg()
    rng = np.random.default_rng(5)
    seq = rng.integers(0, 256, (40, 100), dtype=np.uint8)
    got = orient(seq, None, 100, read_len=77, n_out=13)  # reads 0 .. 13 of 40
    check(seq, None, 100, got, read_len=77)
    import torch
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for kw in (dict(d_seq=a.data_ptr() + 4, d_seq_out=b.data_ptr()), dict(d_seq=a.data_ptr(), d_seq_out=a.data_ptr()),
               dict(d_seq=a.data_ptr(), d_seq_out=b.data_ptr(), read_len=101), dict(d_seq=a.data_ptr(), d_seq_out=None)):
        with pytest.raises(pkg.BarcodeCountError):
            pkg.orient_device(kw["d_seq"], None, 100, kw.get("read_len", 100), 4, kw["d_seq_out"], None)
