"""bc_fold_apply's units of work (csrc/bc_fold.h: fold_apply_unit): one quarter of one item's bucket per workgroup and
step, the four quarters of an item on four workgroups that read the same entries.  Whatever the grid, every quarter of
every item must be applied exactly once: tables of five buckets -- an empty one, one of a single entry, one whose
entries repeat their tuples within a batch and across batches, a split one of kFoldChunk + 1 entries and a last one
that the table ends in the second quarter of -- with entries either side of every quarter edge and kLogNone every
seventh entry, folded with grids of 1 to 256 apply workgroups and 1, 2 and the engine's number of scatter workgroups,
in the ordinary mode onto random bits and in the fresh mode onto a map of 0xFF.  The checks are those of
test_gpu_fold.py (bit map, table, dirty map, grouped log, meta buffer and canaries against numpy)."""
import numpy as np
import pytest

import test_gpu_fold as tg
from test_gpu_fold_fresh import FreshFold

APPLY_GRIDS = [1, 2, 3, 4, 5, 8, 31, 32, 33, 64, 96, 256]
SCATTER_GRIDS = [1, 2, 0]
# which bucket is which, in two orders (the last one is always the ragged one: the table ends in it)
TABLES = {"a": ("empty", "one", "repeats", "split", "ragged"), "b": ("split", "one", "empty", "repeats", "ragged")}

_CACHE = {}


def _with_none(valid, none):
    """the valid entries in order, kLogNone before every six of them: every seventh entry of the log"""
    n = valid.size + (valid.size + 5) // 6
    log = np.full(n, none, dtype=np.uint32)
    at = np.flatnonzero(np.arange(n) % 7 != 0)[:valid.size]
    assert at.size == valid.size
    log[at] = valid
    return log


def _table(name):
    """-> (entries, log, tuples of the split bucket)"""
    if name in _CACHE:
        return _CACHE[name]
    k = tg.K()
    bs, qs, ch = 1 << k["bucket_shift"], 1 << k["quarter_shift"], k["chunk"]
    order = TABLES[name]
    rng = np.random.default_rng(len(name) + sum(map(ord, name)))
    tail = qs + 1000 + (17 if name == "a" else 32 * 3 + 5)  # the table ends here, inside the last bucket's second quarter
    entries = 4 * bs + tail
    parts, split_tuples = [], None
    for b, kind in enumerate(order):
        lo = b * bs
        hi = lo + (tail if kind == "ragged" else bs)
        # both sides of every quarter edge of this bucket (its first tuple and its last included)
        edges = np.array([e for q in range(b * 4, b * 4 + 5) for e in (q * qs - 1, q * qs) if lo <= e < hi], dtype=np.int64)
        if kind == "empty":
            continue
        if kind == "one":
            parts.append(np.array([hi - 1]))  # an edge itself: the last tuple before the next bucket
        elif kind == "repeats":
            # 500 tuples 80 times each on average: several times within a batch of 16384 entries, and in all three batches
            tup = np.concatenate([lo + rng.choice(bs, 500, replace=False), edges])
            parts.append(np.concatenate([rng.choice(tup, 40_000), edges, edges]))
        elif kind == "split":
            split_tuples = np.unique(np.concatenate([lo + rng.choice(bs, 300, replace=False), edges]))
            parts.append(np.concatenate([rng.choice(split_tuples, ch + 1 - edges.size), edges]))
            assert parts[-1].size == ch + 1
        else:
            parts.append(np.concatenate([lo + rng.integers(0, tail, 6000), edges, [entries - 1, entries - 1]]))
    valid = np.concatenate(parts).astype(np.uint32)
    rng.shuffle(valid)
    log = _with_none(valid, k["none"])
    assert 250_000 < log.size < 400_000 and (log[::7] == k["none"]).all()
    per_bucket = np.bincount((valid >> np.uint32(k["bucket_shift"])).astype(np.int64), minlength=5)
    assert sorted(per_bucket.tolist())[:2] == [0, 1] and per_bucket.max() == ch + 1
    _CACHE[name] = (entries, log, split_tuples)
    return _CACHE[name]


@pytest.mark.gpu
@pytest.mark.parametrize("apply_grid", APPLY_GRIDS)
@pytest.mark.parametrize("table", sorted(TABLES))
def test_every_quarter_once_whatever_the_grid(table, apply_grid):
    entries, log, _ = _table(table)
    for sg in SCATTER_GRIDS:
        tg.Fold(entries, log.size, seed=40 + apply_grid).fold(log, sg, apply_grid)
        FreshFold(entries, log.size, seed=41 + apply_grid).fold(log, sg, apply_grid)


@pytest.mark.gpu
@pytest.mark.parametrize("apply_grid", [1, 5, 32, 256])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_split_bucket_with_bits_preset(table, apply_grid):
    """the ordinary mode: a third of the split bucket's tuples have their bit set already, the others have it clear"""
    entries, log, split_tuples = _table(table)
    f = tg.Fold(entries, log.size, seed=43)
    f.set_bits(split_tuples, False)
    f.set_bits(split_tuples[::3], True)
    f.fold(log, 0, apply_grid)


@pytest.mark.gpu
@pytest.mark.parametrize("fresh", [False, True])
def test_more_items_than_sibling_groups(fresh):
    """40 buckets of a few thousand entries on 32 workgroups: eight sibling groups, so every workgroup walks five units
    and the item published one unit ahead wraps round its two places"""
    k = tg.K()
    bs, qs = 1 << k["bucket_shift"], 1 << k["quarter_shift"]
    nb = 40
    entries = nb * bs - qs - 3  # the last bucket has three quarters
    rng = np.random.default_rng(44)
    parts = []
    for b in range(nb):
        hi = min((b + 1) * bs, entries)
        parts.append(rng.integers(b * bs, hi, 3000 + 101 * b))
        parts.append(np.array([e for q in range(b * 4, b * 4 + 5) for e in (q * qs - 1, q * qs) if b * bs <= e < hi], dtype=np.int64))
    valid = np.concatenate(parts).astype(np.uint32)
    valid = np.concatenate([valid, valid[:20_000]])  # repeats
    rng.shuffle(valid)
    log = _with_none(valid, k["none"])
    if fresh:
        FreshFold(entries, log.size, seed=45).fold(log, 0, 32)
    else:
        tg.Fold(entries, log.size, seed=45).fold(log, 0, 32)
