"""Inputs of the tests that cross the seams between the match kernels (tests/test_gpu_kernel_seams.py, and the length
sweep of tests/test_lane_emulation.py).  A batch reaches the lane-per-read kernel in one of eight <NW,NWW> instantiations,
its scheme-specialised form, or the wave-per-read kernel, by two numbers only: the longest read the batch can hold
(`stride` with per-read lengths, `read_len` without) and the scheme's length L.  Everything here is a plain case dict in
the form of cases.build_case, or a batch: dict(reads, seq, qual, lens, stride, read_len, use_lens)."""
import numpy as np

import cases
import readgen

LONG_L = "[16]ACGTTGCA{32}GGATCCAT{32}TTGACAGT{24}CATGCATG"  # L = 136: <8,2> and <10,4> need a scheme this long
LONG_L_LEN = 136
NOSAMPLE_LEN = 34
DEL_LEN = 59

# maxlen -> the generic instantiation (or the wave-per-read kernel) that must run: both sides of every edge of NW
# (128/129, 256/257, 320/321) and of NWW (32/33, 64/65, 128/129 candidate offsets = maxlen - L + 1)
NOSAMPLE_EDGES = [(34, "<4,1>"), (65, "<4,1>"), (66, "<4,2>"), (97, "<4,2>"), (98, "<4,4>"), (128, "<4,4>"),
                  (129, "<8,4>"), (161, "<8,4>"), (162, "<8,8>"), (256, "<8,8>"), (257, "<10,10>"), (320, "<10,10>"),
                  (321, "long")]
LONG_L_EDGES = [(136, "<8,2>"), (199, "<8,2>"), (200, "<8,4>"), (256, "<8,4>"), (257, "<10,4>"), (263, "<10,4>"),
                (264, "<10,10>"), (320, "<10,10>"), (321, "long")]
# the specialised kernel serves instantiations up to <8,4>: its last eligible shapes, and the first that are not
JIT_SHAPES = [("nosample", 34, True), ("nosample", 66, True), ("nosample", 97, True), ("nosample", 98, True),
              ("nosample", 128, True), ("nosample", 129, True), ("nosample", 161, True), ("long_l", 256, True),
              ("nosample", 162, False), ("long_l", 257, False)]

_cache = {}


def expected_kernel(tag):
    return "long_match_kernel" if tag == "long" else "match_count_kernel" + tag


def lane_kernel(maxlen, L):
    """the kernel a batch of this shape must reach with the specialised kernel off, stated apart from the engine: 32
    bases per plane word in 4, 8 or 10 words; maxlen - L + 1 candidate offsets in 32-bit words, rounded up to the next
    instantiation; above 320 bases the wave-per-read kernel"""
    if maxlen > 320:
        return "long_match_kernel"
    nw = 4 if maxlen <= 128 else (8 if maxlen <= 256 else 10)
    words = -(-(maxlen - L + 1) // 32) if maxlen >= L else 1
    nww = next(w for w in {4: (1, 2, 4), 8: (2, 4, 8), 10: (4, 10)}[nw] if words <= w)
    return "match_count_kernel<%d,%d>" % (nw, nww)


def nosample_case():
    """NOSAMPLE_SCHEME (L = 34) with counted sets and the quality filter"""
    if "nosample" not in _cache:
        rng = np.random.default_rng(4101)
        _cache["nosample"] = dict(name="seam_nosample", scheme=cases.NOSAMPLE_SCHEME, samples=None,
                                  counted=[readgen.make_set(rng, 30, 9, 2), readgen.make_set(rng, 8, 4, 2)],
                                  kwargs=dict(min_quality=20.0))
    return dict(_cache["nosample"])


def long_l_case():
    """LONG_L: 4 samples, counted sets of 12, 9 and 7 references"""
    if "long_l" not in _cache:
        rng = np.random.default_rng(4102)
        s = readgen.make_set(rng, 4, 16, 4)
        _cache["long_l"] = dict(name="seam_long_l", scheme=LONG_L, samples={x: "S%d" % i for i, x in enumerate(s)},
                                counted=[readgen.make_set(rng, 12, 32, 6), readgen.make_set(rng, 9, 32, 6),
                                         readgen.make_set(rng, 7, 24, 5)],
                                kwargs=dict(min_quality=20.0))
    return dict(_cache["long_l"])


def del_case():
    """DEL_SCHEME (L = 59) as in cases.build_case("del_mismatch_quality"): the sets of the sweep's third scheme"""
    c = cases.build_case("del_mismatch_quality", seed=41, n=1)
    c.pop("reads")
    return c


SWEEP_CASES = {"nosample": nosample_case, "del": del_case, "long_l": long_l_case}
SWEEP_L = {"nosample": NOSAMPLE_LEN, "del": DEL_LEN, "long_l": LONG_L_LEN}


def sweep_lengths(L):
    """every length from L to 320 within one base of a multiple of 32, or within two of L + 32 k: both sides of every
    edge of the plane words (NW) and of the candidate-offset words (NWW)"""
    out = []
    for m in range(L, 321):
        near_word = min(m % 32, 32 - m % 32) <= 1
        near_offsets = min((m - L) % 32, 32 - (m - L) % 32) <= 2
        if near_word or near_offsets:
            out.append(m)
    return out


def make_batch(reads, stride=None, use_lens=False, read_len=None):
    seq, qual, lens = readgen.to_arrays(reads, stride=stride)
    stride = seq.shape[1]
    return dict(reads=reads, seq=np.ascontiguousarray(seq).reshape(-1), qual=np.ascontiguousarray(qual).reshape(-1),
                lens=lens if use_lens else None, stride=stride, read_len=stride if use_lens or read_len is None else read_len,
                use_lens=use_lens)


def shape_batch(which, maxlen, ragged, n=600, keep=True):
    """n reads of case `which` for one dispatch shape: fixed length (read_len = maxlen, no lengths) or ragged (lengths,
    stride = maxlen, the longest read being maxlen bases); keep=False: made anew and not kept (a sweep over many shapes)"""
    key = ("shape", which, maxlen, ragged, n)
    if key in _cache:
        return _cache[key]
    c = SWEEP_CASES[which]()
    rng = np.random.default_rng(7000 + 13 * maxlen + (1 if ragged else 0) + 1000 * sorted(SWEEP_CASES).index(which))
    reads = readgen.gen_reads(rng, c["scheme"], n, maxlen, list(c["samples"]) if c["samples"] else None, c["counted"],
                              p_sub=0.02, p_n=0.004, p_lowq=0.3, var_len=ragged)
    if ragged and max(len(s) for s, _ in reads) < maxlen:  # the stride is the longest line
        s, q = reads[0]
        reads[0] = (s + "A" * (maxlen - len(s)), q + "I" * (maxlen - len(q)))
    b = make_batch(reads, stride=maxlen, use_lens=ragged)
    if keep:
        _cache[key] = b
    return b


def _sets(rng, kind):
    if kind == "raw":
        return None, None, [readgen.make_set(rng, 12, 9, 2), readgen.make_set(rng, 5, 4, 2)]
    s = readgen.make_set(rng, 3, 8, 3)
    counted = [readgen.make_set(rng, 5, 8, 3) for _ in range(3)]
    return s, counted, counted


def small(kind="plain"):
    """SMALL ("plain": DEL_SCHEME, 3 samples x 5 x 5 x 5 references = 375 tuples, so that tuples repeat), SMALL_RANDOM
    ("random": the same sets on DEL_RANDOM_SCHEME, 40 % of the reads copies of earlier ones) or SMALL_RAW ("raw":
    NOSAMPLE_SCHEME without a counted file, captures drawn from pools of 12 and 5) -> the case dict, with c["batches"] =
    {P1..P5} of 1200 reads each:
      P1 100 bases fixed; P2 200 or fewer, ragged, with lengths; P3 300 fixed; P4 330 fixed (wave-per-read kernel);
      P5 P1's reads at stride 336 with lengths (a stride above 320 sends any reads to the wave-per-read kernel)"""
    key = ("small", kind)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(4200)  # the same sets for plain and random
    samples, counted, pool = _sets(rng, kind)
    scheme = {"plain": cases.DEL_SCHEME, "random": cases.DEL_RANDOM_SCHEME, "raw": cases.NOSAMPLE_SCHEME}[kind]
    c = dict(name="seam_small_" + kind, scheme=scheme, samples={x: "S%d" % i for i, x in enumerate(samples)} if samples else None,
             counted=counted, kwargs=dict(min_quality=20.0))
    dup = 0.4 if kind == "random" else 0.0
    batches = {}
    for seed, (name, rl, ragged) in enumerate([("P1", 100, False), ("P2", 200, True), ("P3", 300, False), ("P4", 330, False)], 1):
        r = np.random.default_rng(seed)
        reads = readgen.gen_reads(r, scheme, 1200, rl, samples, pool, p_sub=0.02, p_n=0.004, p_lowq=0.3, dup_frac=dup,
                                  var_len=ragged)
        batches[name] = make_batch(reads, use_lens=ragged)
    batches["P5"] = make_batch(batches["P1"]["reads"], stride=336, use_lens=True)
    c["batches"] = batches
    _cache[key] = c
    return c


ORDERS = [("P1", "P4", "P2"), ("P4", "P1", "P3"), ("P1", "P5")]
LONG_BATCHES = ("P4", "P5")


def same_reads_pool(n=600):
    """one pool of ragged DEL_SCHEME reads of 250 bases or fewer, submitted at six strides"""
    if "pool" not in _cache:
        c = del_case()
        rng = np.random.default_rng(4300)
        c["reads"] = readgen.gen_reads(rng, c["scheme"], n, 250, list(c["samples"]), c["counted"], p_sub=0.02, p_n=0.004,
                                       p_lowq=0.3, var_len=True)
        _cache["pool"] = c
    return _cache["pool"]


POOL_STRIDES = [(250, "<8,8>"), (256, "<8,8>"), (257, "<10,10>"), (320, "<10,10>"), (321, "long"), (336, "long")]


def fastq_records(c, parts, seed):
    """parts: [(records, shortest, longest)] -> reads of case `c` with lengths drawn from each part's range in turn"""
    rng = np.random.default_rng(seed)
    samples = list(c["samples"]) if c["samples"] else None
    reads = []
    for n, lo, hi in parts:
        for _ in range(n):
            rl = int(rng.integers(lo, hi + 1))
            reads += readgen.gen_reads(rng, c["scheme"], 1, rl, samples, c["counted"], p_sub=0.02, p_n=0.004, p_lowq=0.3)
    return reads


def fastq_text(reads, first=0):
    return "".join("@r%d\n%s\n+\n%s\n" % (first + i, s, q) for i, (s, q) in enumerate(reads)).encode()
