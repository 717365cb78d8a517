"""Inputs for the barcode-search tests (test_search_neighbourhoods.py on the host, test_gpu_search_neighbourhoods.py on
the device): reference sets built by construction so that every index of bc_plan::lower gets crowded buckets and near
pairs, whole mismatch neighbourhoods of chosen centre references as captures, and a brute-force fix_error in numpy.

The brute force shares no code with the kernel, the lane code or the C oracle: it counts mismatches byte by byte with
one matrix product over one-hot letters and applies the reference's rule (parse.rs:553-593 with the set-membership
test in front, parse.rs:457/489): an exact member wins; otherwise the unique minimum of mismatches, counted where
neither side is 'N' and over the shorter of the two strings, if it is within the budget."""
import functools
import itertools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib

C1, C2 = "TTGTGGAAAGGACG", "GTTTTAGAGC"
FAMILY_SIZES = (5, 8, 33, 65, 129, 257)
SUFFIX_SIZE = 40        # more than the 32 entries per segment of coarse_probe_x4's first round trip
SCATTERED = 100         # scattered references of the "families" configurations
MIN_READ = 44
FLOOR = 20              # captures per class that every configuration must hold (asserted from the brute force alone)
SPARSE_PATTERN = (1, 2, 3, 5, 17, 6, 7, 33, 18, 19, 20, 4)  # searching lanes per wavefront of the sparse arrangement
SPARSE_READS = 48000    # neighbourhood reads in the sparse arrangement (about 6.5 exact reads go with each)
SECOND_LEN, SECOND_N = 8, 30  # the second group of the "two" configuration

# kind: which group the set is ("counted", "sample") or "two" (a second, small counted group behind it)
# n: references in all (None: families + SCATTERED); fams: prefix-family sizes; expect: what bc_plan::lower must choose
_F = FAMILY_SIZES
CONFIGS = {
    "d10": dict(len=10, n=300, budget=2, fams=(), expect=dict(mode=1, lhash=True)),
    "d10big": dict(len=10, n=4200, budget=1, fams=(), expect=dict(mode=1, lhash=False)),
    "h11scan": dict(len=11, n=127, budget=2, fams=(5, 8, 33), expect=dict(mode=2, seed=(0, 0), tier=0)),
    "h11b1": dict(len=11, n=128, budget=1, fams=(5, 8, 33), expect=dict(mode=2, seed=(2, 5), tier=5, stride=5, compact=1)),
    "h11b2": dict(len=11, n=128, budget=2, fams=(5, 8, 33), expect=dict(mode=2, seed=(3, 3), tier=5, stride=5, compact=1)),
    "h16": dict(len=16, n=None, budget=3, fams=_F,
                expect=dict(mode=2, seed=(4, 4), seed2=(3, 5), tier=8, stride=8, compact=1, defer=1)),
    "h20b2": dict(len=20, n=None, budget=2, fams=_F, expect=dict(mode=2, seed=(3, 6), tier=8, stride=10, compact=1, defer=0)),
    "h20b3": dict(len=20, n=None, budget=3, fams=_F,
                  expect=dict(mode=2, seed=(4, 5), seed2=(3, 6), tier=8, stride=10, compact=1, defer=1)),
    "h20b4": dict(len=20, n=None, budget=4, fams=_F,
                  expect=dict(mode=2, seed=(5, 4), seed2=(3, 6), seed3=(4, 5), tier=8, stride=10, compact=1, defer=1)),
    "h20b5": dict(len=20, n=None, budget=5, fams=_F,
                  expect=dict(mode=2, seed=(6, 3), seed2=(3, 6), seed3=(4, 5), tier=8, stride=10, compact=1, defer=1)),
    "h20b6": dict(len=20, n=None, budget=6, fams=_F, expect=dict(mode=2, seed=(0, 0), tier=0, defer=0)),
    "h26c": dict(len=26, n=512, budget=1, fams=(5, 8, 33, 65, 129), expect=dict(mode=2, seed=(2, 8), tier=8, stride=13, compact=1)),
    "h26w": dict(len=26, n=513, budget=1, fams=(5, 8, 33, 65, 129), expect=dict(mode=2, seed=(2, 8), tier=8, stride=13, compact=0)),
    "h32b1": dict(len=32, n=None, budget=1, fams=_F, expect=dict(mode=2, seed=(2, 8), tier=8, stride=16, compact=0, defer=0)),
    "h32b3": dict(len=32, n=None, budget=3, fams=_F, full_centres=2,
                  expect=dict(mode=2, seed=(4, 8), seed2=(3, 8), tier=8, stride=16, compact=0, defer=1)),
    "odd": dict(len=20, n=None, budget=3, fams=_F, odd=True,
                expect=dict(mode=2, seed=(4, 5), seed2=(3, 6), tier=0, n_odd=2, defer=0)),
    "two": dict(len=20, n=None, budget=3, fams=_F, kind="two",
                expect=dict(mode=2, seed=(4, 5), seed2=(3, 6), tier=8, stride=10, compact=1, defer=0)),
    "sample": dict(len=16, n=None, budget=3, fams=_F, kind="sample",
                   expect=dict(mode=2, seed=(4, 4), seed2=(3, 5), tier=8, stride=8, compact=1, defer=1)),
}
SPECIALISED = ("d10", "h20b3", "h20b4", "h26w", "two")


def _ascii(codes):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[codes]


def _text(codes):
    return _ascii(codes).tobytes().decode()


# ---- reference sets ---------------------------------------------------------------------------------------------
def build_refs(L, n, fams, seed, odd=False):
    """-> (refs as strings, info).  Order: the prefix families (each with its four near-pair partners last), the suffix
    family, four scattered near pairs, scattered references up to n, then (odd) one reference with an 'N' and one of
    L - 1 bases.  info: families [(first index, members with partners)], suffix (first, members), pairs [(a, b, d)]"""
    rng = np.random.default_rng(seed)
    refs, seen = [], set()
    pairs = []

    def add(code):
        key = code.tobytes()
        if key in seen:
            return False
        seen.add(key)
        refs.append(code.astype(np.uint8))
        return True

    def rand(k):
        return rng.integers(0, 4, k).astype(np.uint8)

    def partner_of(j, d, lo):
        """a new reference at distance d from reference j, differing at positions >= lo only"""
        while True:
            pos = rng.choice(np.arange(lo, L), d, replace=False)
            out = refs[j].copy()
            out[pos] = (out[pos] + rng.integers(1, 4, d)) % 4
            if add(out):
                pairs.append((j, len(refs) - 1, d))
                return

    families, prefixes = [], set()
    for size in fams:
        while True:
            prefix = rand(8)
            if prefix.tobytes() not in prefixes:
                prefixes.add(prefix.tobytes())
                break
        first = len(refs)
        while len(refs) - first < size:
            add(np.concatenate([prefix, rand(L - 8)]))
        for d in (1, 2, 3, 4):  # the partners keep the prefix: they sit in the family's bucket, behind everything else
            partner_of(first + d - 1, min(d, L - 8), 8)
        families.append((first, len(refs) - first))
    s0 = min(L // 2, 8)
    sfx = rand(L - s0)
    first = len(refs)
    while len(refs) - first < SUFFIX_SIZE:
        add(np.concatenate([rand(s0), sfx]))
    suffix = (first, SUFFIX_SIZE)
    scattered_first = len(refs)
    for d in (1, 2, 3, 4):
        while not add(rand(L)):
            pass
        partner_of(len(refs) - 1, d, 0)
    total = n if n is not None else len(refs) + SCATTERED
    assert len(refs) <= total, (len(refs), total)
    while len(refs) < total:
        add(rand(L))
    out = [_text(r) for r in refs]
    if odd:
        with_n = refs[scattered_first + 9].copy()
        out.append(_text(with_n)[:3] + "N" + _text(with_n)[4:])
        out.append(_text(rand(L - 1)))
    info = dict(families=families, suffix=suffix, pairs=pairs, scattered=scattered_first, n_plain=len(refs))
    return out, info


def index_blocks(L, budget, n, n_odd=0):
    """{index: [(first base, bases)]} as bc_plan::lower lays them out (the tests assert that it did)"""
    out = {}
    nb = budget + 1
    blen = min(8, L // nb)
    if L <= 10 or n < 128 or blen < 3:
        return out
    out["seed"] = [(b * blen, blen) for b in range(nb)]
    if nb > 3 and L // 3 >= 5:
        out["seed2"] = [(b * min(8, L // 3), min(8, L // 3)) for b in range(3)]
        if nb > 4 and L // 4 >= 5:
            out["seed3"] = [(b * min(8, L // 4), min(8, L // 4)) for b in range(4)]
    tb = min(8, L // 2)
    if budget >= 1 and tb >= 4 and n_odd == 0:
        out["tier"] = [(0, tb), (L // 2, tb)]
    return out


# ---- captures ---------------------------------------------------------------------------------------------------
def _subs(centre, d, positions=None):
    """every capture (base codes) that differs from `centre` at exactly d of `positions`"""
    L = len(centre)
    if d == 0:
        return centre[None].copy()
    positions = np.arange(L) if positions is None else np.asarray(positions)
    pos = np.array(list(itertools.combinations(positions.tolist(), d)), dtype=np.int64).reshape(-1, d)
    sub = np.array(list(itertools.product((1, 2, 3), repeat=d)), dtype=np.uint8)
    out = np.broadcast_to(centre, (len(pos), len(sub), L)).copy()
    rows = np.arange(len(pos))[:, None, None]
    cols = np.arange(len(sub))[None, :, None]
    out[rows, cols, pos[:, None, :]] = (centre[pos][:, None, :] + sub[None]) % 4
    return out.reshape(-1, L)


def _spoil(rng, centre, positions):
    out = centre.copy()
    positions = np.asarray(positions, dtype=np.int64)
    out[positions] = (out[positions] + rng.integers(1, 4, len(positions))) % 4
    return out


def _sampled_far(rng, centre, d, blocks):
    """captures at distance d > 3: for every index, every subset of min(d, blocks) of its blocks spoiled (one mismatch
    in each, the rest of the mismatches in the same blocks or on bases no block covers), twice; plus random placements"""
    L = len(centre)
    out = []
    for index in blocks.values():
        covered = set()
        for first, ln in index:
            covered.update(range(first, first + ln))
        free = [p for p in range(L) if p not in covered]
        for subset in itertools.combinations(range(len(index)), min(d, len(index))):
            for _ in range(2):
                pos = [int(rng.integers(index[b][0], index[b][0] + index[b][1])) for b in subset]
                pool = [p for b in subset for p in range(index[b][0], index[b][0] + index[b][1]) if p not in pos] + free
                if len(pool) < d - len(pos):
                    pool = [p for p in range(L) if p not in pos]
                pos += rng.choice(pool, d - len(pos), replace=False).tolist()
                out.append(_spoil(rng, centre, pos))
    for _ in range(8):
        out.append(_spoil(rng, centre, rng.choice(L, d, replace=False)))
    return np.array(out, dtype=np.uint8)


def _ties(rng, centre, partner, budget):
    """captures as far from `centre` as from `partner`, at every distance up to budget + 1 that the pair allows"""
    L = len(centre)
    diff = np.flatnonzero(centre != partner)
    same = np.flatnonzero(centre == partner)
    dp = len(diff)
    out = []
    for t in range(1, budget + 2):
        for a in range(dp // 2 + 1):      # a bases of the partner, b third letters, e mismatches with both
            b = dp - 2 * a
            e = t - a - b
            if e < 0 or e > len(same):
                continue
            for _ in range(12):
                cap = centre.copy()
                p = rng.permutation(diff)
                cap[p[:a]] = partner[p[:a]]
                for q in p[a:a + b]:
                    cap[q] = [x for x in range(4) if x != centre[q] and x != partner[q]][int(rng.integers(0, 2))]
                cap = _spoil(rng, cap, rng.choice(same, e, replace=False))
                out.append(cap)
    return np.array(out, dtype=np.uint8).reshape(-1, L)


def _with_n(rng, centre, full_double):
    """ASCII captures with 'N': every single and double placement with no and with one further mismatch (all of them
    for single 'N's and, where full_double, for double ones; four drawn ones otherwise), drawn 3-, 4- and 5-'N' captures
    and a few captures that hold a byte outside ACGTN"""
    L = len(centre)
    out = []
    for i in range(L):
        others = [p for p in range(L) if p != i]
        a = _ascii(np.concatenate([_subs(centre, 0), _subs(centre, 1, others)]))
        a[:, i] = ord("N")
        out.append(a)
    for i, j in itertools.combinations(range(L), 2):
        others = [p for p in range(L) if p != i and p != j]
        one = _subs(centre, 1, others)
        if not full_double:
            one = one[rng.choice(len(one), 4, replace=False)]
        a = _ascii(np.concatenate([_subs(centre, 0), one]))
        a[:, (i, j)] = ord("N")
        out.append(a)
    drawn = []
    for k in (3, 4, 5):
        for _ in range(40):
            p = rng.permutation(L)
            a = _ascii(_spoil(rng, centre, p[k:k + int(rng.integers(0, 3))]))
            a[p[:k]] = ord("N")
            drawn.append(a)
    for _ in range(12):
        p = rng.permutation(L)
        a = _ascii(_spoil(rng, centre, p[1:1 + int(rng.integers(0, 2))]))
        a[p[0]] = b"acgtnRYX."[int(rng.integers(0, 9))]
        drawn.append(a)
    out.append(np.array(drawn, dtype=np.uint8))
    return np.concatenate(out)


# places in a family's bucket at which the cooperative searches hand over: behind the 32 entries per segment of
# coarse_probe_x4's first round trip, behind the first 64 and the first 128 of wave_scan_blocks_wide
CENTRE_PLACES = (40, 70, 130)


def choose_centres(info, n_refs):
    """[(reference, its near partner or None)]: the first member of the first family (its partner at distance 1 sits
    behind the bucket's head), the distance-2 partner that ends the largest family (behind 256 entries there), members
    at CENTRE_PLACES of the smallest families that have such a place, the suffix family's member 36, both ends of
    scattered near pairs, and scattered references: at least eight"""
    partner = {}
    for a, b, _ in info["pairs"]:
        partner[a] = b
        partner[b] = a
    out = []
    if info["families"]:
        f0, _ = info["families"][0]
        fl, nl = info["families"][-1]
        out += [f0, fl + nl - 3]
        for place in CENTRE_PLACES:
            for first, members in info["families"]:
                if members - 4 > place and first + place not in out:
                    out.append(first + place)
                    break
    out.append(info["suffix"][0] + 36)
    sc = info["scattered"]
    out += [sc, sc + 5, sc + 9]  # distance-1 pair (first end), distance-3 pair (partner end), plain
    k = sc + 8
    while len(out) < 8:
        if k not in out:
            out.append(k)
        k += 1
    assert len(set(out)) == len(out) and max(out) < n_refs
    return [(c, partner.get(c)) for c in out]


def build_captures(refs, info, L, budget, seed, full_centres=8):
    """ASCII captures [m, L] around the centres.  Complete up to distance min(budget + 1, 3); the first `full_centres`
    centres carry the complete outermost shell and the complete double-'N' set, the others (configurations whose shell
    is too large to run for every centre) a drawn tenth of that shell"""
    rng = np.random.default_rng(seed)
    codes = {c: i for i, c in enumerate("ACGT")}
    code = lambda j: np.array([codes[c] for c in refs[j]], dtype=np.uint8)
    blocks = index_blocks(L, budget, len(refs), len(refs) - info["n_plain"])
    dmax = min(budget + 1, 3)
    plain, noisy = [], []
    for k, (c, partner) in enumerate(choose_centres(info, info["n_plain"])):
        centre = code(c)
        for d in range(dmax + 1):
            shell = _subs(centre, d)
            if k >= full_centres and d == dmax:
                shell = shell[rng.choice(len(shell), len(shell) // 10, replace=False)]
            plain.append(shell)
        for d in range(4, budget + 2):
            plain.append(_sampled_far(rng, centre, d, blocks))
        if partner is not None:
            plain.append(_ties(rng, centre, code(partner), budget))
        noisy.append(_with_n(rng, centre, k < min(full_centres, 2)))
    return np.concatenate([_ascii(np.concatenate(plain))] + noisy)


# ---- the brute force --------------------------------------------------------------------------------------------
def brute_fix_error(refs, captures, budget):
    """refs: strings; captures: uint8 [m, L] (ASCII).  -> (matched [m] bool, reference index [m] int64 (-1: none),
    smallest mismatch count [m] int64, tie [m] bool: more than one reference at that count)"""
    captures = np.ascontiguousarray(captures)
    m, L = captures.shape
    n = len(refs)
    R = np.zeros((n, L), dtype=np.uint8)  # 0: past the reference's end (zip stops at the shorter string)
    rlen = np.array([len(r) for r in refs])
    for j, r in enumerate(refs):
        R[j, :min(len(r), L)] = np.frombuffer(r.encode(), dtype=np.uint8)[:L]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    r_one = (R[:, :, None] == letters).reshape(n, 4 * L).astype(np.float32)
    r_cmp = ((R != ord("N")) & (R != 0)).astype(np.float32)
    matched = np.zeros(m, dtype=bool)
    idx = np.full(m, -1, dtype=np.int64)
    best = np.zeros(m, dtype=np.int64)
    tie = np.zeros(m, dtype=bool)
    step = max(1024, 16000000 // n)
    for i0 in range(0, m, step):
        cap = captures[i0:i0 + step]
        c_one = (cap[:, :, None] == letters).reshape(len(cap), 4 * L).astype(np.float32)
        c_cmp = (cap != ord("N")).astype(np.float32)
        # positions compared (neither side 'N', inside both strings) minus positions with the same letter
        D = (c_cmp @ r_cmp.T - c_one @ r_one.T).astype(np.uint8)
        dmin = D.min(axis=1)
        cnt = np.count_nonzero(D == dmin[:, None], axis=1)
        arg = D.argmin(axis=1)
        ok = (dmin <= budget) & (cnt == 1)
        sl = slice(i0, i0 + len(cap))
        matched[sl] = ok
        idx[sl] = np.where(ok, arg, -1)
        best[sl] = dmin.astype(np.int64)
        tie[sl] = cnt > 1
        # an exact member (the very string) wins whatever else is near
        zrow = np.flatnonzero(dmin == 0)
        zi, zj = np.nonzero(D[zrow] == 0)
        zi = zrow[zi]
        same =(rlen[zj] == L) & (cap[zi] == R[zj]).all(axis=1)
        for i, j in zip(zi[same][::-1], zj[same][::-1]):
            matched[i0 + i], idx[i0 + i], tie[i0 + i] = True, j, False
    return matched, idx, best, tie


def floors(brute, captures, budget):
    """{class: captures in it}, from the brute force alone"""
    matched, idx, best, tie = brute
    has_n = (captures == ord("N")).any(axis=1)
    out = {}
    for d in range(1, budget + 1):
        out["unique at %d" % d] = int((matched & (best == d) & ~has_n).sum())
        out["tied at %d" % d] = int((tie & (best == d) & ~has_n).sum())
    out["nearest at budget + 1"] = int((best == budget + 1).sum())
    out["with N, matched"] = int((has_n & matched).sum())
    out["with N, failed"] = int((has_n & ~matched).sum())
    return out


# ---- a configuration, ready to run ------------------------------------------------------------------------------
class Config:
    pass


@functools.lru_cache(maxsize=3)
def build(name):
    """the configuration's sets, captures, brute-force answers and its two read arrangements (built once, shared)"""
    spec = CONFIGS[name]
    c = Config()
    c.name, c.len, c.budget, c.kind = name, spec["len"], spec["budget"], spec.get("kind", "counted")
    c.expect = spec["expect"]
    seed = 1000 + sorted(CONFIGS).index(name)
    c.refs, c.info = build_refs(c.len, spec["n"], spec["fams"], seed, spec.get("odd", False))
    c.captures = build_captures(c.refs, c.info, c.len, c.budget, seed + 500, spec.get("full_centres", 8))
    c.brute = brute_fix_error(c.refs, c.captures, c.budget)
    rng = np.random.default_rng(seed + 900)
    m = len(c.captures)
    c.second = None
    if c.kind == "two":
        c.second = sorted({_text(r) for r in rng.integers(0, 4, (4 * SECOND_N, SECOND_LEN))})[:SECOND_N]
        c.scheme = C1 + "{%d}TGGA{%d}" % (c.len, SECOND_LEN) + C2
    else:
        c.scheme = C1 + ("[%d]" if c.kind == "sample" else "{%d}") % c.len + C2
    c.fail_code = 2 if c.kind == "sample" else 3
    kw = dict(max_constant=0)
    kw["max_sample" if c.kind == "sample" else "max_barcode"] = c.budget
    c.case = dict(scheme=c.scheme, kwargs=kw)
    if c.kind == "sample":
        c.case["samples"] = {r: r for r in c.refs}
    else:
        c.case["counted"] = [c.refs] + ([c.second] if c.second else [])
    # every plain reference as a capture of its own: the exact reads of the sparse arrangement
    c.n_plain = c.info["n_plain"]
    own = np.array([np.frombuffer(r.encode(), dtype=np.uint8) for r in c.refs[:c.n_plain]])
    own_brute = brute_fix_error(c.refs, own, c.budget)
    assert own_brute[0].all() and (own_brute[1] == np.arange(c.n_plain)).all()
    # packed: the neighbourhood reads one after the other; sparse: a drawn part of them, SPARSE_PATTERN[w] of them at
    # drawn lanes of wavefront w (64 consecutive reads), every other read an exact one
    sel = rng.permutation(m)[:SPARSE_READS]
    src, at = [], 0
    w = 0
    while at < len(sel):
        k = min(SPARSE_PATTERN[w % len(SPARSE_PATTERN)], len(sel) - at)
        wave = -1 - rng.integers(0, c.n_plain, 64)  # -1 - j: the exact read of reference j
        wave[rng.choice(64, k, replace=False)] = sel[at:at + k]
        src.append(wave)
        at += k
        w += 1
    src = np.concatenate(src)
    c.sources = {"packed": np.arange(m), "sparse": src}
    c.own, c.seed, c.arrangements = own, seed, {}
    return c


def arrangement(c, kind):
    """reads (uint8 [reads, stride]) and the brute force's per-read answer for them: outcome code and dense index"""
    if kind in c.arrangements:
        return c.arrangements[kind]
    src, own = c.sources[kind], c.own
    rng = np.random.default_rng(c.seed + len(kind))
    a = c.arrangements[kind] = Config()
    filler = src < 0
    caps = np.where(filler[:, None], own[np.where(filler, -1 - src, 0)], c.captures[np.where(filler, 0, src)])
    matched = np.where(filler, True, c.brute[0][np.where(filler, 0, src)])
    idx = np.where(filler, -1 - src, c.brute[1][np.where(filler, 0, src)])
    a.searching = ~filler
    const = lambda s: np.broadcast_to(np.frombuffer(s.encode(), dtype=np.uint8), (len(src), len(s)))
    parts = [const(C1), caps]
    if c.second:
        second = np.array([np.frombuffer(r.encode(), dtype=np.uint8) for r in c.second])
        pick = rng.integers(0, len(second), len(src))
        m2, i2, _, _ = brute_fix_error(c.second, second[pick], c.budget)
        assert m2.all()
        parts += [const("TGGA"), second[pick]]
        idx = idx * len(c.second) + i2
    parts.append(const(C2))
    used = sum(p.shape[1] for p in parts)
    if used < MIN_READ:
        parts.append(const(("CA" * MIN_READ)[:MIN_READ - used]))
    a.seq = np.ascontiguousarray(np.concatenate(parts, axis=1))
    a.stride = a.seq.shape[1]
    a.outcome = np.where(matched, 0, c.fail_code).astype(np.uint8)
    a.index = np.where(matched, idx, -1)
    return a


def oracle_run(c, a, threads=8):
    """the arrangement through the C oracle, in `threads` slices -> (per-read outcomes, counters, sorted rows)"""
    n = len(a.seq)
    cuts = [n * t // threads for t in range(threads + 1)]

    def one(t):
        o = oracle_lib.Oracle(c.case["scheme"], samples=c.case.get("samples"), counted=c.case.get("counted"), **c.case["kwargs"])
        part = a.seq[cuts[t]:cuts[t + 1]]
        outc = o.process_batch_outcomes(part.reshape(-1), None, a.stride, a.stride) if len(part) else np.zeros(0, np.uint8)
        return outc, o.counters, o.rows()

    oracle_lib.lib()  # (built before the threads start)
    with ThreadPoolExecutor(threads) as pool:
        res = list(pool.map(one, range(threads)))
    counters = {k: sum(r[1][k] for r in res) for k in oracle_lib.NAMES}
    rows = {}
    for r in res:
        for s, t, cnt in r[2]:
            rows[(s, t)] = rows.get((s, t), 0) + cnt
    return np.concatenate([r[0] for r in res]), counters, sorted((s, t, cnt) for (s, t), cnt in rows.items())


def expected_rows(c, a):
    """the rows the brute force's answers add up to, in the form of Engine.result_rows()"""
    keep = a.index[a.outcome == 0]
    values, counts = np.unique(keep, return_counts=True)
    out = []
    for v, cnt in zip(values.tolist(), counts.tolist()):
        if c.kind == "sample":
            out.append((c.refs[v], "", cnt))
        elif c.second:
            out.append(("barcode", c.refs[v // len(c.second)] + "," + c.second[v % len(c.second)], cnt))
        else:
            out.append(("barcode", c.refs[v], cnt))
    return sorted(out)


def check_layout(c, lay):
    """the configuration landed on the layer it is there for, and its crowded buckets are crowded"""
    e = c.expect
    assert lay["mode"] == e["mode"] and lay["len"] == c.len and lay["max_err"] == c.budget and lay["n_refs"] == len(c.refs), lay
    if "lhash" in e:
        assert (lay["lhash_nb"] > 0 and lay["lhash_complete"] == 1) == e["lhash"], lay
        return
    for key in ("seed", "seed2", "seed3"):
        assert (lay[key + "_nb"], lay[key + "_blen"]) == e.get(key, (0, 0)), (key, lay[key + "_nb"], lay[key + "_blen"])
    assert lay["tier_blen"] == e["tier"], lay["tier_blen"]
    if e["tier"]:
        assert (lay["tier_stride"], lay["tier_compact"]) == (e["stride"], e["compact"])
    assert lay["n_odd"] == e.get("n_odd", 0) and lay["n_idx"] == (c.n_plain if lay["seed_nb"] else 0)
    if "defer" in e:
        assert lay["defer_search"] == e["defer"]
    got = {}
    if lay["seed_nb"]:
        got["seed"] = [(b * lay["seed_blen"], lay["seed_blen"]) for b in range(lay["seed_nb"])]
    if lay["seed2_nb"]:
        got["seed2"] = [(b * lay["seed2_blen"], lay["seed2_blen"]) for b in range(lay["seed2_nb"])]
    if lay["seed3_nb"]:
        got["seed3"] = [(b * lay["seed3_blen"], lay["seed3_blen"]) for b in range(lay["seed3_nb"])]
    if lay["tier_blen"]:
        got["tier"] = [(0, lay["tier_blen"]), (lay["tier_stride"], lay["tier_blen"])]
    assert got == index_blocks(c.len, c.budget, len(c.refs), lay["n_odd"])  # what the far samples were aimed at
    # bucket lengths: each family in block 0, the suffix family in the last block, of every index
    for key, blocks in got.items():
        off = lay[key + "_off"].reshape(len(blocks), -1)
        for first, members in c.info["families"] + [c.info["suffix"]]:
            b = len(blocks) - 1 if (first, members) == c.info["suffix"] else 0
            v = block_value(c.refs[first], *blocks[b])
            assert off[b][v + 1] - off[b][v] >= members, (key, first, members, int(off[b][v + 1] - off[b][v]))


def block_value(ref, first, bases):
    """bucket of `ref` in a block: plane 1 (ASCII bit 1) in the low bits, plane 2 (ASCII bit 2) above it, base i at bit i"""
    v = 0
    for i in range(bases):
        ch = ord(ref[first + i])
        v |= ((ch >> 1) & 1) << i | ((ch >> 2) & 1) << (bases + i)
    return v
