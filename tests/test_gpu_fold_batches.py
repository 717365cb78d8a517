"""The count-log fold (csrc/bc_fold.h) where its loads run ahead of their use.  bc_fold_scatter keeps a tile's sixteen
entries per thread in registers, takes every tile but the last without a bounds test and requests the workgroup's next
tile before it writes the current one out; bc_fold_apply requests a batch of 16384 entries (sixteen per thread, four
16-byte loads from the aligned-down start of the item) before it processes the batch ahead of it -- the next batch of
the quarter, the first batch of the next quarter, the first batch of the workgroup's next item -- and issues a batch's
sixteen LDS atomics together.  The cases sit on the edges of tiles, batches, items and quarters, with one workgroup
walking all of them in order (scatter_grid = 1, apply_grid = 1) and with two; every fold is checked word for word by
test_gpu_fold.Fold.fold (bit map, table, dirty map, grouped log, meta buffer, canaries), once onto random bits (the
ordinary fold) and once in fresh mode (test_gpu_fold_fresh.FreshFold: the map counts as zero and holds 0xFF words).
Tables have three or four buckets."""
import numpy as np
import pytest

import test_gpu_fold as tg
import test_gpu_fold_fresh as tf

MODES = ["ordinary", "fresh"]


def _fold(mode, entries, log, seed, scatter_grid=0, apply_grid=0, prep=None):
    log = np.ascontiguousarray(log, dtype=np.uint32)
    if mode == "fresh":
        assert prep is None  # (a fresh fold starts from zeros whatever was preset)
        tf.FreshFold(entries, log.size, seed).fold(log, scatter_grid, apply_grid)
    else:
        f = tg.Fold(entries, log.size, seed)
        if prep:
            prep(f)
        f.fold(log, scatter_grid, apply_grid)


def _sizes():
    k = tg.K()
    return 1 << k["bucket_shift"], 1 << k["quarter_shift"], k["tile"], k["chunk"], k["none"]


def _random_log(rng, entries, n, none_every=0):
    log = rng.integers(0, entries, n).astype(np.uint32)
    if n > 8:
        log[3::7] = log[1::7][:log[3::7].size]  # repeats
    if none_every:
        log[::none_every] = tg.K()["none"]
    return log


# ---------------------------------------------------------------------------------------------------------------------
# scatter: tile edges, one workgroup walking (and prefetching) every tile, and two

# (the last four: n % 4 = 2, 3, 3, 2; none of the others leaves 2)
TILE_EDGES = {"tile-1": lambda t: t - 1, "tile": lambda t: t, "tile+1": lambda t: t + 1, "2*tile-1": lambda t: 2 * t - 1,
              "2*tile": lambda t: 2 * t, "2*tile+1": lambda t: 2 * t + 1, "3*tile+5": lambda t: 3 * t + 5,
              "tile+2": lambda t: t + 2, "2*tile+3": lambda t: 2 * t + 3, "7": lambda t: 7, "4098": lambda t: 4098}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("edge", TILE_EDGES)
def test_scatter_tile_edges(edge, mode):
    bs, _, tile, _, _ = _sizes()
    n = TILE_EDGES[edge](tile)
    entries = 3 * bs + 1000
    rng = np.random.default_rng(n)
    log = _random_log(rng, entries, n, none_every=53)
    log[-1] = entries - 1  # the log's last entry counts
    for sg in (1, 2):
        _fold(mode, entries, log, seed=n % 1000, scatter_grid=sg)


def test_tile_edges_cover_every_residue():
    """no GPU needed: the sizes above leave every n % 4, and both sides of every tile edge"""
    tile = 16384
    ns = [f(tile) for f in TILE_EDGES.values()]
    assert {n % 4 for n in ns} == {0, 1, 2, 3}
    assert {n % tile for n in ns} >= {tile - 1, 0, 1, 2, 3, 5}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ["none-tile-between-full-tiles", "full-tile-then-one-entry", "none-tile-last"])
def test_scatter_tiles_of_nothing(shape, mode):
    bs, _, tile, _, none = _sizes()
    entries = 4 * bs - 7
    rng = np.random.default_rng(41)
    full = lambda: _random_log(rng, entries, tile)
    nothing = np.full(tile, none, dtype=np.uint32)
    log = {"none-tile-between-full-tiles": lambda: np.concatenate([full(), nothing, full()]),
           "full-tile-then-one-entry": lambda: np.concatenate([full(), [entries - 1]]),
           "none-tile-last": lambda: np.concatenate([full(), nothing[:tile - 3]])}[shape]()
    for sg in (1, 2):
        _fold(mode, entries, log, seed=42, scatter_grid=sg)


# ---------------------------------------------------------------------------------------------------------------------
# apply: one workgroup walks every item in order (apply_grid = 1)

def _bucket_entries(rng, bs, b, count, lo=0, hi=None):
    """count entries of bucket b, tuples drawn from [lo, hi) of the bucket, some of them repeated"""
    hi = bs if hi is None else hi
    t = b * bs + rng.integers(lo, hi, count)
    if count > 4:
        t[2::5] = t[0::5][:t[2::5].size]
    return t


# entries per bucket; the items' first entries in the grouped log (the running sums) take every residue mod 4
BATCH_COUNTS = [(1, 16383, 16384, 16385), (16385, 32769, 0, 32768), (1, 1, 1, 16383), (16383, 32769, 16385, 1),
                (0, 16385, 1, 32768), (32768, 0, 32769, 16384)]


def test_batch_counts_cover_every_case():
    """no GPU needed: every count around the batch size is there, and every residue of an item's first entry"""
    assert {c for row in BATCH_COUNTS for c in row} == {0, 1, 16383, 16384, 16385, 32768, 32769}
    firsts = {int(s) % 4 for row in BATCH_COUNTS for s, c in zip(np.r_[0, np.cumsum(row)[:-1]], row) if c}
    assert firsts == {0, 1, 2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("counts", BATCH_COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_apply_items_around_the_batch(counts, mode):
    bs, _, tile, chunk, none = _sizes()
    assert tile == 16384 and chunk >= 2 * tile + 1  # what the counts above are about
    entries = 4 * bs - 3
    rng = np.random.default_rng(sum(counts))
    parts = [_bucket_entries(rng, bs, b, c, hi=bs - 3 if b == 3 else bs) for b, c in enumerate(counts)]
    log = np.concatenate(parts + [np.full(11, none)]).astype(np.uint32)
    rng.shuffle(log)
    _fold(mode, entries, log, seed=7, apply_grid=1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", ["split-then-single", "single-then-split"])
def test_apply_split_bucket_beside_a_single_item(order, mode):
    """kFoldChunk + 1 entries: two items, the second of one entry; its neighbour has one item"""
    bs, _, _, chunk, _ = _sizes()
    entries = 3 * bs + 64
    rng = np.random.default_rng(50)
    split, single = (0, 1) if order == "split-then-single" else (1, 0)
    log = np.concatenate([_bucket_entries(rng, bs, split, chunk + 1), _bucket_entries(rng, bs, single, 5000),
                          _bucket_entries(rng, bs, 2, 3)]).astype(np.uint32)
    rng.shuffle(log)
    for ag in (1, 2):
        _fold(mode, entries, log, seed=51, apply_grid=ag)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("quarter", [0, 3])
def test_apply_buckets_of_one_quarter(quarter, mode):
    """every entry of every bucket in the same quarter: the other three passes find nothing to do"""
    bs, qs, _, _, _ = _sizes()
    entries = 3 * bs + (quarter + 1) * qs  # (the last bucket reaches just as far as that quarter)
    rng = np.random.default_rng(60 + quarter)
    log = np.concatenate([_bucket_entries(rng, bs, b, 20_000 + 4097 * b, lo=quarter * qs, hi=(quarter + 1) * qs)
                          for b in range(4)]).astype(np.uint32)
    rng.shuffle(log)
    _fold(mode, entries, log, seed=61, apply_grid=1)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_apply_table_ends_inside_quarter_one(mode):
    """the last bucket has two quarters, the second ragged, and entries in its first only: the batch requested for the
    quarter that does not exist must not be missed by the next item, nor the ragged quarter be written past its end"""
    bs, qs, _, _, _ = _sizes()
    entries = 2 * bs + qs + 12_345
    rng = np.random.default_rng(70)
    log = np.concatenate([_bucket_entries(rng, bs, 0, 40_000), _bucket_entries(rng, bs, 1, 17),
                          _bucket_entries(rng, bs, 2, 33_000, hi=qs)]).astype(np.uint32)
    rng.shuffle(log)
    for ag in (1, 2):
        _fold(mode, entries, log, seed=71, apply_grid=ag)


REPEATS = ["adjacent", "1024-apart", "4096-apart", "16384-apart", "everywhere"]


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["clear", "preset", "fresh"])
@pytest.mark.parametrize("neighbour", [False, True], ids=["alone", "with-neighbour-bit"])
@pytest.mark.parametrize("where", REPEATS)
def test_apply_same_tuple_within_a_batch(where, neighbour, state):
    """one tuple several times among the entries of its bucket: next to each other (one thread's 16 bytes), 1024 and
    4096 entries apart (other threads of the batch), 16384 apart (the next batch), and -- the order inside a bucket of
    the grouped log being free -- a bucket of nothing but three tuples, where every distance occurs whatever the order.
    Exactly one OR may see the bit clear: the table ends at + c - 1 (bit clear before) or + c (bit set before)."""
    bs, qs, tile, _, _ = _sizes()
    entries = 3 * bs + 5
    rng = np.random.default_rng(80)
    t = bs + 2 * qs + 32 * 1000 + 7  # bucket 1, quarter 2, bit 7 of its word
    others = [t + 1, t - 7] if neighbour else []  # bits 8 and 0 of the same word
    if where == "everywhere":
        bucket = rng.choice(np.array([t] + (others or [t + 64])), 2 * tile + 5)
    else:
        bucket = bs + rng.choice(bs // 64, 2 * tile + 8, replace=False) * 64 + 40  # distinct words, none of them t's
        p = 4 * 100
        gap = {"adjacent": 1, "1024-apart": 1024, "4096-apart": 4096, "16384-apart": 16384}[where]
        bucket[[p, p + gap]] = t
        bucket[p + 2 * gap if where != "16384-apart" else p + 2] = t
        for j, o in enumerate(others):
            bucket[[p + 8 + j, p + 8 + j + gap]] = o
    # the bucket's entries keep their order in the log, one workgroup scatters: were the order kept, these were the
    # distances in the grouped log
    log = np.concatenate([_bucket_entries(rng, bs, 0, 4), bucket, _bucket_entries(rng, bs, 2, 6)]).astype(np.uint32)

    def prep(f):
        f.set_bits([t] + others, state == "preset")
        if state == "preset":
            f.table[t] = 1000

    _fold("fresh" if state == "fresh" else "ordinary", entries, log, seed=81, scatter_grid=1, apply_grid=1,
          prep=None if state == "fresh" else prep)


@pytest.mark.gpu
def test_a_log_off_its_16_byte_alignment_is_refused():
    """both kernels read the log and the grouped log as 16-byte groups: fold_launch returns hipErrorInvalidValue for a
    base that is not aligned so, and launches nothing"""
    import torch
    bs, _, _, _, _ = _sizes()
    k = tg.K()
    f = tg.Fold(3 * bs, 1000, seed=90)
    before = [t.clone() for t in (f.bits, f.table, f.dirty, f.grouped, f.meta)]
    d_log = torch.zeros(1004, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for log_off, grouped_off in ((4, 0), (8, 0), (0, 4)):
        rc = k["lib"].fold_harness_run(d_log.data_ptr() + log_off, 1000, f.grouped.data_ptr() + grouped_off, f.meta.data_ptr(),
                                       f.nb, f.bits.data_ptr(), f.n_words, f.table.data_ptr(), f.dirty.data_ptr(), 0, 0)
        assert rc == 1, "hipError %d" % rc  # hipErrorInvalidValue
    torch.cuda.synchronize()
    for t, b in zip((f.bits, f.table, f.dirty, f.grouped, f.meta), before):
        assert torch.equal(t, b)
