"""The barcode search over whole mismatch neighbourhoods, host half (tests/search_cases.py has the inputs).

For every configuration -- one per layer of the search that bc_plan::lower can choose -- three things are checked here:
the numpy brute force against the C oracle read by read (two independent references have to agree before any kernel is
judged), the invariants of the indexes lower() built, read from the arrays themselves, and the lane code (bc_lane.h,
through tests/emu) against the brute force per read, in both compiled forms.

What the host half covers of the search: the direct table, the LDS exact table, the exact hash and the tier lookups
(tier_lookup, tier_lookup_single_n) on crowded and compact buckets.  The emulation's `nearest` is a linear loop over
the references, so the wave-cooperative searches of bc_kernel.h (wave_scan_blocks, wave_scan_blocks_wide,
coarse_probe_x4, coarse_with_n, the search queue) do NOT run here: tests/test_gpu_search_neighbourhoods.py runs the
same inputs through them on the device."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import emu_lib
import search_cases as sc


@pytest.fixture(scope="module", params=list(sc.CONFIGS))
def cfg(request):
    """(module scope: pytest runs the tests configuration by configuration, so each is built once)"""
    c = sc.build(request.param)
    got = sc.floors(c.brute, c.captures, c.budget)
    assert min(got.values()) >= sc.FLOOR, got  # before anything else is looked at
    return c


def test_brute_force_agrees_with_the_oracle(cfg):
    a = sc.arrangement(cfg, "packed")
    outcomes, counters, rows = sc.oracle_run(cfg, a)
    bad = np.flatnonzero(outcomes != a.outcome)
    assert len(bad) == 0, (len(bad), a.seq[bad[0]].tobytes(), int(outcomes[bad[0]]), int(a.outcome[bad[0]]))
    assert rows == sc.expected_rows(cfg, a)
    assert counters["matched"] == int((a.outcome == 0).sum()) and sum(counters.values()) == len(a.seq)


def _planes(refs, L):
    """bit planes of N-free references of L bases: ASCII bit 1 and ASCII bit 2 of base i at bit i"""
    b = np.array([np.frombuffer(r.encode(), dtype=np.uint8) for r in refs]).astype(np.uint64)
    w = np.uint64(1) << np.arange(L, dtype=np.uint64)
    return (((b >> np.uint64(1)) & np.uint64(1)) * w).sum(axis=1), (((b >> np.uint64(2)) & np.uint64(1)) * w).sum(axis=1)


def test_index_invariants(cfg):
    plan = emu_lib.make_plan(cfg.case)
    lay = emu_lib.group_layout(plan)
    sc.check_layout(cfg, lay)
    L, n_idx = cfg.len, lay["n_idx"]
    if lay["mode"] != 2 or not lay["seed_nb"]:
        assert all(lay[k].size == 0 for k in ("seed_off", "seed2_off", "seed3_off", "tier_off", "tier_bkt"))
        return
    assert n_idx == cfg.n_plain
    r1, r2 = _planes(cfg.refs[:n_idx], L)
    assert (lay["r1"][:n_idx] == r1).all() and (lay["r2"][:n_idx] == r2).all()
    assert sorted(lay["odd_list"].tolist()) == list(range(n_idx, len(cfg.refs)))
    blocks = sc.index_blocks(L, cfg.budget, len(cfg.refs), lay["n_odd"])
    assert set(blocks) == {k for k in ("seed", "seed2", "seed3", "tier") if lay[k + "_off"].size}
    for key, bl in blocks.items():
        off = lay[key + "_off"].reshape(len(bl), -1).astype(np.int64)
        lst = lay[key + "_list"].reshape(len(bl), n_idx, 4)
        for b, (first, bases) in enumerate(bl):
            assert off.shape[1] == 4 ** bases + 1
            assert off[b][0] == 0 and off[b][-1] == n_idx and (np.diff(off[b]) >= 0).all(), (key, b)
            j = lst[b, :, 2].astype(np.int64)
            assert (np.sort(j) == np.arange(n_idx)).all(), (key, b)  # every plain reference exactly once
            assert (lst[b, :, 0] == r1[j]).all() and (lst[b, :, 1] == r2[j]).all() and (lst[b, :, 3] == 0).all()
            m = np.uint64((1 << bases) - 1)
            value = (((r1 >> np.uint64(first)) & m) | (((r2 >> np.uint64(first)) & m) << np.uint64(bases))).astype(np.int64)
            at = np.arange(n_idx)
            assert ((off[b][value[j]] <= at) & (at < off[b][value[j] + 1])).all(), (key, b)  # in its own value's bucket
            assert value[0] == sc.block_value(cfg.refs[0], first, bases)
            # ... and in the order of the set inside a bucket: what puts the near-pair partners behind the head
            same = np.searchsorted(off[b], at[1:], side="right") == np.searchsorted(off[b], at[:-1], side="right")
            assert (j[1:][same] > j[:-1][same]).all(), (key, b)
    if not lay["tier_blen"]:
        assert lay["tier_bkt"].size == 0
        return
    nbk = 4 ** lay["tier_blen"]
    off = lay["tier_off"].reshape(2, nbk + 1).astype(np.int64)
    lst = lay["tier_list"].reshape(2, n_idx, 4).astype(np.uint64)
    count = np.diff(off, axis=1)
    assert count.max() >= max(m for _, m in cfg.info["families"])
    if lay["tier_compact"]:
        e = lay["tier_bkt"].reshape(2, nbk, 4, 2).astype(np.uint64)
        e = e[..., 0] | (e[..., 1] << np.uint64(32))
        assert ((e[:, :, 0] >> np.uint64(61)) == np.minimum(count, 7)).all()  # the count, capped at 7
        assert (e[:, :, 1:] >> np.uint64(61) == 0).all()
        e &= np.uint64((1 << 61) - 1)
        lm = np.uint64((1 << L) - 1)
        head = np.stack([e & lm, (e >> np.uint64(L)) & lm, e >> np.uint64(2 * L)], axis=-1)
    else:
        e = lay["tier_bkt"].reshape(2, nbk, 4, 4).astype(np.uint64)
        assert (e[..., 3] == count[:, :, None]).all()
        head = e[..., :3]
    for k in range(4):  # the heads are the first four list entries; unused head slots are zero
        on = count > k
        pos = np.where(on, off[:, :-1] + k, 0)
        want = np.where(on[..., None], np.take_along_axis(lst[..., :3], pos[..., None], axis=1), 0)
        assert (head[:, :, k] == want).all(), k


@pytest.mark.parametrize("variant", ["generic", "static"])
def test_lane_code_agrees_with_the_brute_force(cfg, variant):
    a = sc.arrangement(cfg, "packed")
    plan = emu_lib.make_plan(cfg.case, variant)
    handle = emu_lib.open_plan(plan)
    n, threads = len(a.seq), 8
    cuts = [n * t // threads for t in range(threads + 1)]

    def one(t):
        part = np.ascontiguousarray(a.seq[cuts[t]:cuts[t + 1]]).reshape(-1)
        return emu_lib.emulate(plan, part, None, None, a.stride, a.stride, handle=handle)[:2]

    try:
        with ThreadPoolExecutor(threads) as pool:
            res = list(pool.map(one, range(threads)))
    finally:
        emu_lib.close_plan(plan, handle)
    outcomes = np.concatenate([r[0] for r in res])
    index = np.concatenate([r[1] for r in res]).astype(np.int64)
    bad = np.flatnonzero((outcomes != a.outcome) | ((a.outcome == 0) & (index != a.index)))
    assert len(bad) == 0, (len(bad), a.seq[bad[0]].tobytes(), int(outcomes[bad[0]]), int(a.outcome[bad[0]]),
                           int(index[bad[0]]), int(a.index[bad[0]]))
