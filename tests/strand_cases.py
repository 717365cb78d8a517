"""Helpers shared by the strand tests: rc() as the header defines it, mixed-orientation inputs, and the oracle
composition that states what `reverse` and `both` count (the reference has no such option)."""
import copy

import numpy as np

import parity

_PAIRS = b"ATCGMKRYVBHD"
_COMP = bytes.maketrans(_PAIRS + _PAIRS.lower(), b"TAGCKMYRBVDH" + b"TAGCKMYRBVDH".lower())
PAD_SEQ, PAD_QUAL = ord("N"), ord("!")


def rc_seq(b):
    """bytes -> reverse complement: the IUPAC pairs in either case, every other byte itself"""
    return b.translate(_COMP)[::-1]


def rc(seq, qual):
    """a read as (str, str): the sequence reverse-complemented over its own length, the quality line reversed over its
    own"""
    return rc_seq(seq.encode("latin-1")).decode("latin-1"), qual[::-1]


def mix(case, seed):
    """a copy of the case with a seeded half of its reads replaced by their rc"""
    c = copy.copy(case)
    rng = np.random.default_rng(7000 + seed)
    flip = rng.random(len(case["reads"])) < 0.5
    c["reads"] = [rc(s, q) if f else (s, q) for (s, q), f in zip(case["reads"], flip)]
    return c


def fixed_length(case):
    """a copy of the case whose reads all have the longest read's length: shorter ones get bases and qualities appended
    (cutting them instead would cut the scheme off the reads that hold it near their end)"""
    c = copy.copy(case)
    n = max(len(s) for s, _ in case["reads"])
    c["reads"] = [(s + ("ACGT" * n)[:n - len(s)], q + "I" * (n - len(q))) for s, q in case["reads"]]
    return c


def orientation_census(case):
    """how the reads of a mixed case split, from two probe oracles' verdicts on every read as it stands and reversed:
    dict(forward: past the constant region as they stand, reverse_only: only as rc, neither, either_way: past it in both
    orientations, matched_forward, matched_reverse_only)"""
    pf, pr = parity.oracle_for(case), parity.oracle_for(case)
    f = [pf.process(s, q) for s, q in case["reads"]]
    r = [pr.process(*rc(s, q)) for s, q in case["reads"]]
    cr = "constant_region"
    return dict(forward=sum(a != cr for a in f), reverse_only=sum(a == cr and b != cr for a, b in zip(f, r)),
                neither=sum(a == cr and b == cr for a, b in zip(f, r)), either_way=sum(a != cr and b != cr for a, b in zip(f, r)),
                matched_forward=sum(a == "matched" for a in f),
                matched_reverse_only=sum(a == cr and b == "matched" for a, b in zip(f, r)))


def substituted(case, mode):
    """-> (the reads the oracle is run on, which of them were replaced by their rc).  `both`: the reads a PROBE oracle
    instance calls constant_region"""
    reads = case["reads"]
    if mode == "forward":
        return list(reads), [False] * len(reads)
    if mode == "reverse":
        return [rc(s, q) for s, q in reads], [True] * len(reads)
    assert mode == "both"
    probe = parity.oracle_for(case)
    swap = [probe.process(s, q) == "constant_region" for s, q in reads]
    return [rc(s, q) if w else (s, q) for (s, q), w in zip(reads, swap)], swap


def expected(case, mode):
    """the oracle composition: oracle.process in read order on the substituted input.
    -> dict(outcomes [names], counters, rows, retried, matched_reverse, oracle, reads, swapped)"""
    reads, swap = substituted(case, mode)
    o = parity.oracle_for(case)
    out = [o.process(s, q) for s, q in reads]
    return dict(outcomes=out, counters=o.counters, rows=o.rows(), retried=sum(swap),
                matched_reverse=sum(1 for e, w in zip(out, swap) if w and e == "matched"), oracle=o, reads=reads, swapped=swap)


def check_engine(case, plan, eng, exp, outc=None, idx=None, fold_duplicates=False):
    """counters, rows and strand_reads of an engine against expected(); with a trace also every read's outcome and (for a
    matched read) index, through parity.decode_rows.  fold_duplicates: matched / duplicate are one class per read (which
    of two equal keys is the duplicate depends on scheduling)"""
    got = eng.counters()
    assert {k: got[k] for k in exp["counters"]} == exp["counters"], (got, exp["counters"])
    assert got["total_reads"] == len(case["reads"]) and got["unsupported_reads"] == 0, got
    assert eng.result_rows() == exp["rows"]
    if fold_duplicates:
        # of two sightings of one molecule either may be the BC_MATCHED one: only the reads that passed every test in
        # reverse bound the second number
        retried, matched_reverse = eng.strand_reads()
        passed = sum(1 for e, w in zip(exp["outcomes"], exp["swapped"]) if w and e in ("matched", "duplicates"))
        assert retried == exp["retried"] and 0 < matched_reverse <= passed, (retried, matched_reverse, passed)
    else:
        assert eng.strand_reads() == (exp["retried"], exp["matched_reverse"])
    if outc is None:
        return
    fold = (lambda v: 0 if v == parity.CODE["duplicates"] else v) if fold_duplicates else (lambda v: v)
    counts = {}
    for i, e in enumerate(exp["outcomes"]):
        assert fold(int(outc[i])) == fold(parity.CODE[e]), (i, e, int(outc[i]), case["reads"][i], exp["swapped"][i])
        if e == "matched" and not fold_duplicates:
            counts[int(idx[i])] = counts.get(int(idx[i]), 0) + 1
    if not fold_duplicates:
        discard = (not plan.sample_barcode) and len(plan.samples()) > 0
        assert parity.decode_rows(plan, counts, discard) == exp["rows"]
