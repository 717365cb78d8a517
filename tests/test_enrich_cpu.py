"""ResultsEnrichment from index marginals (the form bc_engine_enrich hands out) against the reference's string path
(info.rs:840-904, restated in pyref_output.Writer.add_single / add_double), on the host: random (sample, tuple, count)
rows, the marginals summed with numpy, the maps compared key by key."""
import numpy as np
import pytest

import pyref_output


def _pkg():
    import ngs_barcode_count_amd as pkg
    return pkg


def marginals(rows, n_samples, sizes):
    """numpy marginal sums of (sample, tuple, count) rows, in Engine.enrichment's form"""
    G = len(sizes)
    singles = [np.zeros((n_samples, n), dtype=np.uint64) for n in sizes]
    doubles = {}
    if G >= 3:
        doubles = {(g, h): np.zeros((n_samples, sizes[g], sizes[h]), dtype=np.uint64)
                   for g in range(G) for h in range(g + 1, G)}
    if rows:
        s = np.array([r[0] for r in rows])
        t = np.array([r[1] for r in rows])
        c = np.array([r[2] for r in rows], dtype=np.uint64)
        for g in range(G):
            np.add.at(singles[g], (s, t[:, g]), c)
        for (g, h), a in doubles.items():
            np.add.at(a, (s, t[:, g], t[:, h]), c)
    return singles, doubles


def string_path(rows, sample_keys, ids):
    """what the reference builds from the same rows written as ID strings"""
    w = pyref_output.Writer({k: {} for k in sample_keys}, {}, [], len(ids), "p", False, True)
    for k in sample_keys:
        w.single[k], w.double[k] = {}, {}
    for s, t, c in rows:
        written = ",".join(ids[g][i] for g, i in enumerate(t))
        w.add_single(sample_keys[s], written, c)
        if len(ids) > 2:
            w.add_double(sample_keys[s], written, c)
    return w.single, w.double


def random_rows(rng, n_samples, sizes, n_rows, skip_sample=None):
    seen, rows = set(), []
    for _ in range(n_rows):
        s = int(rng.integers(n_samples))
        if s == skip_sample:
            continue
        t = tuple(int(rng.integers(n)) for n in sizes)
        if (s, t) in seen:  # (rows are the table's non-zero entries: one per tuple)
            continue
        seen.add((s, t))
        rows.append((s, t, int(rng.integers(1, 1 << 20))))
    return rows


@pytest.mark.parametrize("sizes", [(5, 7), (4, 6, 5), (3, 4, 2, 5), (9, 1, 8)])
@pytest.mark.parametrize("dup_ids", [False, True])
def test_marginals_equal_string_path(sizes, dup_ids):
    rng = np.random.default_rng(len(sizes) * 10 + dup_ids)
    sample_keys = ["AACC", "GGTT", "CATG"]
    ids = [["g%d_%d" % (g, i) for i in range(n)] for g, n in enumerate(sizes)]
    if dup_ids:  # two sequences of one group that share an ID: their counts add up
        for g in range(len(sizes)):
            if sizes[g] > 2:
                ids[g][2] = ids[g][0]
        ids[-1][-1] = ""  # an empty ID
    rows = random_rows(rng, 3, sizes, 60, skip_sample=1)  # sample 1 receives nothing
    singles, doubles = marginals(rows, 3, sizes)
    e = _pkg().ResultsEnrichment()
    e.add_sample_barcodes(sample_keys)
    e.add_marginals(sample_keys, ids, singles, doubles)
    exp_single, exp_double = string_path(rows, sample_keys, ids)
    assert e.single_hashmap == exp_single
    assert e.double_hashmap == exp_double
    assert e.single_hashmap["GGTT"] == {} and e.double_hashmap["GGTT"] == {}
    if len(sizes) == 4:
        assert len({k for k in e.double_hashmap["AACC"]}) > 0
        assert len(doubles) == 6
    if len(sizes) < 3:
        assert all(v == {} for v in e.double_hashmap.values())


def test_keys_exist_only_where_the_sum_is_not_zero():
    sizes = (3, 3, 3)
    ids = [["a", "b", "c"], ["d", "e", "f"], ["x", "x", "y"]]
    rows = [(0, (0, 1, 2), 4), (0, (2, 1, 0), 1)]
    singles, doubles = marginals(rows, 1, sizes)
    e = _pkg().ResultsEnrichment()
    e.add_sample_barcodes(["barcode"])
    e.add_marginals(["barcode"], ids, singles, doubles)
    assert e.single_hashmap["barcode"] == {"a,,": 4, "c,,": 1, ",e,": 5, ",,y": 4, ",,x": 1}
    assert e.double_hashmap["barcode"] == {"a,e,": 4, "c,e,": 1, "a,,y": 4, "c,,x": 1, ",e,y": 4, ",e,x": 1}
    assert (e.single_hashmap, e.double_hashmap) == string_path(rows, ["barcode"], ids)


def test_unknown_sample_adds_land_nowhere():
    """the reference adds a sample it has no map for into a temporary (info.rs:862)"""
    e = _pkg().ResultsEnrichment()
    e.add_sample_barcodes(["S1"])
    e.add_single("S2", "a,b", 3)
    e.add_double("S2", "a,b,c", 3)
    e.add_single("S1", "a,b", 3)
    assert e.single_hashmap == {"S1": {"a,": 3, ",b": 3}} and e.double_hashmap == {"S1": {}}
    singles, doubles = marginals([(1, (0, 0, 0), 2)], 2, (1, 1, 1))
    e.add_marginals(["S1", "S2"], [["a"], ["b"], ["c"]], singles, doubles)
    assert set(e.single_hashmap) == {"S1"} and e.single_hashmap["S1"] == {"a,": 3, ",b": 3}


class _FakePlan:
    def __init__(self, samples, sample_barcode, ids):
        self._samples, self.sample_barcode, self._ids = samples, sample_barcode, ids
        self.barcode_num = len(ids)

    def samples(self):
        return [(s, "id_" + s) for s in self._samples]

    def counted(self, g):
        return [("SEQ%d" % i, x) for i, x in enumerate(self._ids[g])]


class _FakeEngine:
    """what ResultsEnrichment.fill reads from an engine: its plan and its enrichment()"""

    def __init__(self, plan, rows, n_samples):
        self.plan = plan
        self._m = marginals(rows, n_samples, [len(x) for x in plan._ids])

    def enrichment(self):
        return self._m


@pytest.mark.parametrize("landed", [False, True])
def test_fill_keys_with_a_sample_file_but_no_sample_barcode(landed):
    """the reference's writers make maps for every key of Results: the sample file's sequences, and "barcode" only once
    a count lands there (a random-barcode run, info.rs:792-801)"""
    ids = [["a", "b"], ["c"], ["d", "e"]]
    plan = _FakePlan(["AAAA", "CCCC"], False, ids)
    rows = [(0, (1, 0, 1), 3)] if landed else []
    e = _pkg().ResultsEnrichment().fill(_FakeEngine(plan, rows, 1))
    keys = {"AAAA", "CCCC"} | ({"barcode"} if landed else set())
    assert set(e.single_hashmap) == keys and set(e.double_hashmap) == keys
    assert e.single_hashmap["AAAA"] == {} and e.single_hashmap["CCCC"] == {}
    if landed:
        exp = string_path(rows, ["barcode"], ids)
        assert e.single_hashmap["barcode"] == exp[0]["barcode"] and e.double_hashmap["barcode"] == exp[1]["barcode"]


def test_fill_keys_with_and_without_a_sample_barcode():
    ids = [["a", "b"], ["c", "d"]]
    e = _pkg().ResultsEnrichment().fill(_FakeEngine(_FakePlan([], False, ids), [], 1))
    assert e.single_hashmap == {"barcode": {}} and e.double_hashmap == {"barcode": {}}
    rows = [(1, (0, 1), 2)]
    e = _pkg().ResultsEnrichment().fill(_FakeEngine(_FakePlan(["AAAA", "CCCC", "GGGG"], True, ids), rows, 3))
    assert e.single_hashmap == {"AAAA": {}, "CCCC": {"a,": 2, ",d": 2}, "GGGG": {}}
