"""ngs-barcode-count_amd -- MI355X (gfx950) engine for the per-read match/count path of
Roco-scientist/NGS-Barcode-Count, behind the C ABI of include/barcode_count_hip.h.

Import name: `ngs_barcode_count_amd` (the shim module at the repo root maps it onto this
directory, whose name is not a Python identifier).

Two layers:
  * Plan / Engine / Synth -- thin ctypes wrappers of the C ABI;
  * SequenceFormat, BarcodeConversions, MaxSeqErrors, SequenceErrors, Results, SequenceParser --
    host-side mirror of the reference's own types for this path (src/info.rs, src/parse.rs), same
    names and argument meaning, so callers and tests read like the reference.
There is no CPU implementation in this package: without the HIP library everything raises.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import COUNTER_NAMES, SynthParams
from ._lib import BC_ENRICH_SINGLE as ENRICH_SINGLE, BC_ENRICH_DOUBLE as ENRICH_DOUBLE

__all__ = ["Plan", "Engine", "Comm", "Synth", "SequenceFormat", "BarcodeConversions", "MaxSeqErrors", "SequenceErrors",
           "Results", "ResultsEnrichment", "SequenceParser", "fix_error", "BarcodeCountError", "COUNTER_NAMES",
           "ENRICH_SINGLE", "ENRICH_DOUBLE"]


class BarcodeCountError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (status %d)" % (msg, code))
        self.code = code


def _check(lib, rc):
    if rc != 0:
        raise BarcodeCountError(rc, _lib.last_error(lib))


def _opt(v):
    return -1 if v is None else int(v)


class Plan:
    """Compiled scheme + known barcode sets + error budgets (bc_plan)."""

    def __init__(self, scheme_text, lib=None):
        self._lib = lib or _lib.load()
        b = scheme_text.encode()
        self._p = self._lib.bc_plan_create(b, len(b))
        if not self._p:
            raise BarcodeCountError(_lib.BC_ERR_INVALID, _lib.last_error(self._lib))

    def __del__(self):
        if getattr(self, "_p", None):
            self._lib.bc_plan_destroy(self._p)
            self._p = None

    # SequenceFormat fields (info.rs:176-187)
    format_string = property(lambda s: s._lib.bc_plan_format_string(s._p).decode())
    regions_string = property(lambda s: s._lib.bc_plan_regions_string(s._p).decode())
    regex_string = property(lambda s: s._lib.bc_plan_regex_string(s._p).decode())
    length = property(lambda s: s._lib.bc_plan_length(s._p))
    constant_region_length = property(lambda s: s._lib.bc_plan_constant_region_length(s._p))
    barcode_num = property(lambda s: s._lib.bc_plan_barcode_num(s._p))
    barcode_lengths = property(lambda s: [s._lib.bc_plan_barcode_length(s._p, i) for i in range(s.barcode_num)])
    random_barcode = property(lambda s: bool(s._lib.bc_plan_has_random(s._p)))
    sample_barcode = property(lambda s: bool(s._lib.bc_plan_has_sample(s._p)))

    @property
    def sample_length_option(self):
        v = self._lib.bc_plan_sample_length(self._p)
        return None if v < 0 else v

    def load_sample_csv(self, text):
        b = text.encode()
        _check(self._lib, self._lib.bc_plan_load_sample_csv(self._p, b, len(b)))

    def load_counted_csv(self, text):
        b = text.encode()
        _check(self._lib, self._lib.bc_plan_load_counted_csv(self._p, b, len(b)))

    def add_sample(self, seq, sample_id):
        _check(self._lib, self._lib.bc_plan_add_sample(self._p, seq.encode(), sample_id.encode()))

    def add_counted(self, barcode_index, seq, barcode_id):
        _check(self._lib, self._lib.bc_plan_add_counted(self._p, barcode_index, seq.encode(), barcode_id.encode()))

    def samples(self):
        """[(sequence, id)] in engine index order"""
        L, p = self._lib, self._p
        return [(L.bc_plan_sample_seq(p, i).decode(), L.bc_plan_sample_id(p, i).decode())
                for i in range(L.bc_plan_n_samples(p))]

    def counted(self, barcode_index):
        L, p = self._lib, self._p
        return [(L.bc_plan_counted_seq(p, barcode_index, i).decode(), L.bc_plan_counted_id(p, barcode_index, i).decode())
                for i in range(L.bc_plan_n_counted(p, barcode_index))]

    def set_max_errors(self, sample_errors=None, barcode_errors=None, constant_errors=None):
        _check(self._lib, self._lib.bc_plan_set_max_errors(self._p, _opt(sample_errors), _opt(barcode_errors),
                                                           _opt(constant_errors)))

    def set_min_quality(self, q):
        _check(self._lib, self._lib.bc_plan_set_min_quality(self._p, float(q)))

    def set_strand(self, strand):
        """which orientation of a read is counted: "forward" (default), "reverse" (every read as its reverse
        complement) or "both" (as it stands first; reversed when the constant region fails).  Read by Engine()."""
        if strand not in _lib.STRAND_NAMES:
            raise ValueError("strand must be one of %s, not %r" % (", ".join(_lib.STRAND_NAMES), strand))
        _check(self._lib, self._lib.bc_plan_set_strand(self._p, _lib.STRAND_NAMES.index(strand)))

    strand = property(lambda s: _lib.STRAND_NAMES[s._lib.bc_plan_strand(s._p)])

    max_constant_errors = property(lambda s: s._lib.bc_plan_max_constant_errors(s._p))
    max_sample_errors = property(lambda s: s._lib.bc_plan_max_sample_errors(s._p))
    max_barcode_errors = property(lambda s: [s._lib.bc_plan_max_barcode_errors(s._p, i)
                                             for i in range(s.barcode_num)])

    def quality_threshold(self, run_len):
        return self._lib.bc_plan_quality_threshold(self._p, run_len)

    @property
    def mode(self):
        """"dense" (counter table) or "sparse" (hash map of tuple keys: some barcode is kept raw)"""
        m = self._lib.bc_plan_mode(self._p)
        if m == 0:
            raise BarcodeCountError(_lib.BC_ERR_UNSUPPORTED, _lib.last_error(self._lib))
        return "dense" if m == 1 else "sparse"

    @property
    def table_entries(self):
        if self.mode == "sparse":
            return 0
        return self._lib.bc_plan_table_entries(self._p)


class Engine:
    """One run on one GPU (bc_engine).  `table` may be a caller-owned zeroed device buffer of
    plan.table_entries u32 (e.g. a torch tensor's data_ptr()) so it can be reduced with RCCL."""

    def __init__(self, plan, device=0, stream=None, table_ptr=None):
        self._lib = plan._lib
        self.plan = plan
        self._e = self._lib.bc_engine_create(plan._p, int(device), stream, table_ptr)
        if not self._e:
            raise BarcodeCountError(_lib.BC_ERR_HIP, _lib.last_error(self._lib))

    def close(self):
        if getattr(self, "_e", None):
            self._lib.bc_engine_destroy(self._e)
            self._e = None

    __del__ = close

    def submit_device(self, d_seq, d_qual, n_reads, stride, read_len, d_lens=None):
        _check(self._lib, self._lib.bc_engine_submit_device(self._e, d_seq, d_qual, d_lens, stride, read_len, n_reads))

    def submit_device_q(self, d_seq, d_qual, n_reads, stride, d_lens, d_qlens):
        """records whose quality line differs in length from the sequence line: both length arrays (u16, device)"""
        _check(self._lib, self._lib.bc_engine_submit_device_q(self._e, d_seq, d_qual, d_lens, d_qlens, stride, n_reads))

    def submit_host(self, seq, qual, stride, read_len, lens=None):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        n = seq.size // stride
        qp = None
        if qual is not None:
            qual = np.ascontiguousarray(qual, dtype=np.uint8)
            qp = qual.ctypes.data
        lp = None
        if lens is not None:
            lens = np.ascontiguousarray(lens, dtype=np.uint16)
            lp = lens.ctypes.data
        _check(self._lib, self._lib.bc_engine_submit_host(self._e, seq.ctypes.data, qp, lp, stride, read_len, n))

    def count_fastq(self, path, shard=0, n_shards=1):
        """input::read_fastq + the workers (input.rs:24-89, parse.rs:53-76): reads a .fastq / .fastq.gz
        file and counts it; returns the reference's "Total sequences" value.  A .bam file (unaligned BAM) is counted as
        the FASTQ text `samtools fastq` writes for it; its total is the number of records handed on."""
        n = C.c_uint64()
        if n_shards == 1:
            _check(self._lib, self._lib.bc_fastq_count(self._e, str(path).encode(), C.byref(n), None, None))
        else:  # this GPU's share of the file's records (bc_fastq_count_shard)
            _check(self._lib, self._lib.bc_fastq_count_shard(self._e, str(path).encode(), shard, n_shards, C.byref(n), None, None))
        return n.value

    def sync(self):
        _check(self._lib, self._lib.bc_engine_sync(self._e))

    def reset(self):
        _check(self._lib, self._lib.bc_engine_reset(self._e))

    def reset_results(self):
        """a fresh Results (table / bit map / keys); the outcome counters go on"""
        _check(self._lib, self._lib.bc_engine_reset_results(self._e))

    def counters(self):
        out = (C.c_uint64 * 8)()
        _check(self._lib, self._lib.bc_engine_counters(self._e, out))
        return dict(zip(COUNTER_NAMES, [int(x) for x in out]))

    table_ptr = property(lambda s: s._lib.bc_engine_table_ptr(s._e))
    counters_ptr = property(lambda s: s._lib.bc_engine_counters_ptr(s._e))
    table_entries = property(lambda s: s._lib.bc_engine_table_entries(s._e))

    def trace(self, d_outcome_u8, d_index_u64):
        """per-read outcome / dense index written by the next submits (tests); None disables"""
        _check(self._lib, self._lib.bc_engine_trace(self._e, d_outcome_u8, d_index_u64))

    def strand_reads(self):
        """(retried, matched_reverse): the reads handed to the reverse pass since the engine was created (all of them
        under "reverse", the forward constant-region failures under "both", 0 under "forward") and how many of those
        matched.  Waits for the engine's stream unless the strand is "forward"."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(self._lib, self._lib.bc_engine_strand_reads(self._e, C.byref(a), C.byref(b)))
        return a.value, b.value

    # random-barcode mode: the set of (tuple, random barcode) keys
    def key_count(self):
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_key_count(self._e, C.byref(n)))
        return n.value

    def export_keys(self, d_keys, capacity):
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_export_keys(self._e, d_keys, capacity, C.byref(n)))
        return n.value

    def import_keys(self, d_keys, n):
        new = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_import_keys(self._e, d_keys, n, C.byref(new)))
        return new.value

    def clear_keys(self):
        _check(self._lib, self._lib.bc_engine_clear_keys(self._e))

    def materialize_table(self):
        """random-barcode plans with a dense table: per-tuple distinct counts of the current key set -> the table"""
        _check(self._lib, self._lib.bc_engine_materialize_table(self._e))

    def export_counts(self, d_keys, d_counts, capacity):
        """(key, count) pairs of a raw-key plan's map -> device buffers; None buffers: only their number"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_export_counts(self._e, d_keys, d_counts, capacity, C.byref(n)))
        return n.value

    def import_counts(self, d_keys, d_counts, n):
        _check(self._lib, self._lib.bc_engine_import_counts(self._e, d_keys, d_counts, n))

    def timing(self, enable=True):
        _check(self._lib, self._lib.bc_engine_timing(self._e, 1 if enable else 0))

    def kernel_name(self):
        return self._lib.bc_engine_kernel_name(self._e).decode()

    def count_log_folds(self):
        """folds of a count log into the counters since the engine was created (0: every read counted atomically)"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_count_log_folds(self._e, C.byref(n)))
        return n.value

    def wide_lane_reads(self):
        """reads submitted to the lane-per-read kernel under a wide-key plan since the engine was created (BC_WIDE_LANE=1
        and an eligible plan; 0 otherwise: such reads then went to the wave-per-read kernel)"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_wide_lane_reads(self._e, C.byref(n)))
        return n.value

    def enrich_render_passes(self):
        """table passes made for the sums behind render_enriched() / render_enriched_merged() since the engine was created"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_enrich_render_passes(self._e, C.byref(n)))
        return n.value

    def gz_blocks_inflated(self):
        """BGZF blocks inflated on the device for this engine since it was created (0: every .gz went through zlib)"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_gz_blocks_inflated(self._e, C.byref(n)))
        return n.value

    def gz_segments_inflated(self):
        """segments of ordinary gzip streams inflated on the device for this engine since it was created (BC_GZ_DEVICE=all)"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_gz_segments_inflated(self._e, C.byref(n)))
        return n.value

    def sclk_mhz(self):
        """shader clock right now (0.3 ms probe kernel)"""
        v = C.c_double()
        _check(self._lib, self._lib.bc_engine_sclk_mhz(self._e, C.byref(v)))
        return v.value

    def kernel_ms(self):
        ms, n = C.c_double(), C.c_uint64()
        _check(self._lib, self._lib.bc_engine_kernel_ms(self._e, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_ms_each(self):
        """per-launch times (ms) of the match kernel since the last kernel_ms(), in launch order"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_kernel_ms_each(self._e, None, 0, C.byref(n)))
        out = (C.c_double * max(n.value, 1))()
        _check(self._lib, self._lib.bc_engine_kernel_ms_each(self._e, out, n.value, C.byref(n)))
        return [float(out[i]) for i in range(n.value)]

    def nonzero_entries(self):
        """rows finish() would produce now (dense plans, no random barcode): one sweep of the table"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_nonzero_entries(self._e, C.byref(n)))
        return n.value

    def finish_stream(self, on_rows):
        """bc_engine_finish_stream: on_rows(keys uint64 array, counts uint32 array) per chunk (copies of the chunk);
        returns the number of rows.  Host and device memory stay bounded whatever the table holds."""
        err = []

        def cb(kp, cp, n, _user):
            try:
                on_rows(np.ctypeslib.as_array(kp, shape=(n,)).copy(), np.ctypeslib.as_array(cp, shape=(n,)).copy())
                return 0
            except Exception as ex:  # never let an exception cross the C frames
                err.append(ex)
                return 1

        fn = _lib.ROWS_FN(cb)
        n = C.c_uint64()
        rc = self._lib.bc_engine_finish_stream(self._e, fn, None, C.byref(n))
        if err:
            raise err[0]
        _check(self._lib, rc)
        return n.value

    def _render(self, call, on_text):
        out, err = bytearray(), []

        def cb(tp, n, _user):
            try:
                chunk = C.string_at(tp, n)
                if on_text is None:
                    out.extend(chunk)
                else:
                    on_text(chunk)
                return 0
            except Exception as ex:  # never let an exception cross the C frames
                err.append(ex)
                return 1

        fn = _lib.TEXT_FN(cb)
        n = C.c_uint64()
        rc = call(fn, C.byref(n))
        if err:
            raise err[0]
        _check(self._lib, rc)
        return n.value if on_text is not None else bytes(out)

    def render_counts(self, sample=0, on_text=None):
        """bc_engine_render_counts: the lines of sample index `sample`'s counts file (no header), written on the device,
        in ascending dense-index order: b"id_0,..,id_{G-1},count\\n" per tuple that counts.  -> bytes; with on_text= every
        chunk (bytes, ends with a newline) goes to that callable as it leaves the device and the line count returns."""
        return self._render(lambda fn, n: self._lib.bc_engine_render_counts(self._e, int(sample), fn, None, n), on_text)

    def render_merged(self, samples, on_text=None):
        """bc_engine_render_merged: the merged file's lines (no header) for the sample indices `samples` as columns, in
        that order: one line per tuple that counts in any LISTED sample, zero counts written as 0."""
        cols = np.ascontiguousarray(list(samples), dtype=np.uint32)
        return self._render(lambda fn, n: self._lib.bc_engine_render_merged(
            self._e, cols.ctypes.data if cols.size else None, cols.size, fn, None, n), on_text)

    def render_raw_counts(self, sample=0, on_text=None):
        """bc_engine_render_raw_counts: the lines of sample index `sample`'s counts file (no header) of a raw-key plan,
        sorted and written on the device: b"f_0,..,f_{G-1},count\\n" per tuple the sample counts, a field being the ID of
        a known barcode or the bases of a raw capture; lines ascend by the tuple of per-barcode digits (set index, or the
        capture's base-5 code with its first base least significant).  Returns as render_counts does."""
        return self._render(lambda fn, n: self._lib.bc_engine_render_raw_counts(self._e, int(sample), fn, None, n), on_text)

    def render_raw_merged(self, samples, on_text=None):
        """bc_engine_render_raw_merged: the merged file's lines (no header) of a raw-key plan for the sample indices
        `samples` as columns, in that order: one line per tuple that counts in any LISTED sample, zero counts written as 0."""
        cols = np.ascontiguousarray(list(samples), dtype=np.uint32)
        return self._render(lambda fn, n: self._lib.bc_engine_render_raw_merged(
            self._e, cols.ctypes.data if cols.size else None, cols.size, fn, None, n), on_text)

    def raw_render_sorts(self):
        """sorts made for render_raw_counts() / render_raw_merged() since the engine was created: the renders of one state
        of the counts share one"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_raw_render_sorts(self._e, C.byref(n)))
        return n.value

    def raw_render_sort_ms(self):
        """device milliseconds of the last of those sorts (map export, re-key, sort)"""
        v = C.c_double()
        _check(self._lib, self._lib.bc_engine_raw_render_sort_ms(self._e, C.byref(v)))
        return v.value

    def render_wide_counts(self, sample=0, on_text=None):
        """bc_engine_render_wide_counts: render_raw_counts() for a plan with wide keys (key words > 1: captures above 27
        bases, or several that overflow one 64-bit key): the same lines in the same order, sorted and written on the
        device.  Returns as render_counts does."""
        return self._render(lambda fn, n: self._lib.bc_engine_render_wide_counts(self._e, int(sample), fn, None, n), on_text)

    def render_wide_merged(self, samples, on_text=None):
        """bc_engine_render_wide_merged: render_raw_merged() for a plan with wide keys."""
        cols = np.ascontiguousarray(list(samples), dtype=np.uint32)
        return self._render(lambda fn, n: self._lib.bc_engine_render_wide_merged(
            self._e, cols.ctypes.data if cols.size else None, cols.size, fn, None, n), on_text)

    def wide_render_sorts(self):
        """sorts made for render_wide_counts() / render_wide_merged() since the engine was created: the renders of one
        state of the counts share one"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_wide_render_sorts(self._e, C.byref(n)))
        return n.value

    def wide_render_sort_ms(self):
        """device milliseconds of the last of those sorts (map export, order keys, sort, gather)"""
        v = C.c_double()
        _check(self._lib, self._lib.bc_engine_wide_render_sort_ms(self._e, C.byref(v)))
        return v.value

    def render_enriched(self, kind, sample=0, on_text=None):
        """bc_engine_render_enriched: the lines of sample index `sample`'s Single (kind = ENRICH_SINGLE) or Double
        (ENRICH_DOUBLE) file (no header), written on the device in ascending key order: G comma-joined fields of which
        one (two) holds an ID, then the count, e.g. b",id,,count\\n".  IDs shared inside a set are one key.  Returns as
        render_counts does."""
        return self._render(lambda fn, n: self._lib.bc_engine_render_enriched(self._e, int(kind), int(sample), fn, None, n),
                            on_text)

    def render_enriched_merged(self, kind, samples, on_text=None):
        """bc_engine_render_enriched_merged: the merged Single / Double file's lines (no header) for the sample indices
        `samples` as columns, in that order: one line per key that counts in any LISTED sample."""
        cols = np.ascontiguousarray(list(samples), dtype=np.uint32)
        return self._render(lambda fn, n: self._lib.bc_engine_render_enriched_merged(
            self._e, int(kind), cols.ctypes.data if cols.size else None, cols.size, fn, None, n), on_text)

    def render_raw_enriched(self, kind, sample=0, on_text=None):
        """bc_engine_render_raw_enriched: render_enriched() for a raw-key plan: the lines of sample index `sample`'s Single
        (kind = ENRICH_SINGLE) or Double (ENRICH_DOUBLE) file (no header), summed, sorted and written on the device.  A
        field holds the ID of a known barcode or the bases of a raw capture, e.g. b",ACGTACGT,,7\\n"; Single lines ascend
        by (barcode, digit), Double lines by (pair, digit, digit), the digits being render_raw_counts()'s.  Returns as
        render_counts does."""
        return self._render(lambda fn, n: self._lib.bc_engine_render_raw_enriched(self._e, int(kind), int(sample), fn, None, n),
                            on_text)

    def render_raw_enriched_merged(self, kind, samples, on_text=None):
        """bc_engine_render_raw_enriched_merged: the merged Single / Double file's lines (no header) of a raw-key plan for
        the sample indices `samples` as columns, in that order: one line per key that counts in any LISTED sample."""
        cols = np.ascontiguousarray(list(samples), dtype=np.uint32)
        return self._render(lambda fn, n: self._lib.bc_engine_render_raw_enriched_merged(
            self._e, int(kind), cols.ctypes.data if cols.size else None, cols.size, fn, None, n), on_text)

    def raw_enrich_reduces(self):
        """kinds (Single, Double) built for render_raw_enriched() / render_raw_enriched_merged() since the engine was
        created: the renders of one state of the counts share one build per kind"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_raw_enrich_reduces(self._e, C.byref(n)))
        return n.value

    def raw_enrich_reduce_ms(self):
        """device milliseconds of the last of those builds (project, sort, reduce of every projection of one kind)"""
        v = C.c_double()
        _check(self._lib, self._lib.bc_engine_raw_enrich_reduce_ms(self._e, C.byref(v)))
        return v.value

    def enrichment(self, doubles=True):
        """bc_engine_enrich: single and pair counts of the counts finish() would hand out now, summed on the device ->
        (singles, doubles): singles = [uint64 array (S, N_g) per counted barcode g]; doubles = {(g, h): uint64 array
        (S, N_g, N_h)} for the pairs g < h, empty with fewer than 3 counted barcodes (or doubles=False).  S = samples
        (1 without a sample group).  The engine's table, counters and rows stay as they are."""
        ns, nd = C.c_uint64(), C.c_uint64()
        _check(self._lib, self._lib.bc_engine_enrich_entries(self._e, C.byref(ns), C.byref(nd)))
        sizes = [self._lib.bc_plan_n_counted(self.plan._p, g) for g in range(self.plan.barcode_num)]
        single = np.zeros(ns.value, dtype=np.uint64)
        double = np.zeros(nd.value if doubles else 0, dtype=np.uint64)
        _check(self._lib, self._lib.bc_engine_enrich(self._e, single.ctypes.data if single.size else None,
                                                     double.ctypes.data if double.size else None))
        S = ns.value // sum(sizes) if sum(sizes) else 0
        single = single.reshape(S, sum(sizes))
        singles, off = [], 0
        for n in sizes:
            singles.append(single[:, off:off + n])
            off += n
        pairs = {}
        if double.size:
            double = double.reshape(S, double.size // S)
            off = 0
            for g in range(len(sizes)):
                for h in range(g + 1, len(sizes)):
                    pairs[(g, h)] = double[:, off:off + sizes[g] * sizes[h]].reshape(S, sizes[g], sizes[h])
                    off += sizes[g] * sizes[h]
        return singles, pairs

    def reduce_all(self, comm, root=0):
        """bc_engine_reduce_all: the job's one exchange (collective over comm); -> the job's counters on the root,
        zeros elsewhere.  Afterwards the root's engine holds the job's table / key set / key map."""
        out = (C.c_uint64 * 8)()
        _check(self._lib, self._lib.bc_engine_reduce_all(self._e, comm._c if comm is not None else None, root, out))
        return dict(zip(COUNTER_NAMES, [int(x) for x in out]))

    def finish_all(self, comm, root=0):
        """bc_engine_finish_all = reduce_all + finish on the root; -> (counters, number of rows)"""
        out = (C.c_uint64 * 8)()
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_finish_all(self._e, comm._c if comm is not None else None, root, out, C.byref(n)))
        return dict(zip(COUNTER_NAMES, [int(x) for x in out])), n.value

    def finish(self):
        """bc_engine_finish: compacts the results into sparse rows; returns their number"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_finish(self._e, C.byref(n)))
        return n.value

    def rows(self):
        """-> (sample_idx[n], barcode_idx[n, barcode_num], count[n]) of the non-zero table entries"""
        n = C.c_uint64()
        _check(self._lib, self._lib.bc_engine_finish(self._e, C.byref(n)))
        n = n.value
        nb = max(self.plan.barcode_num, 1)
        s = np.zeros(n, dtype=np.uint32)
        b = np.zeros((n, nb), dtype=np.uint32)
        c = np.zeros(n, dtype=np.uint64)
        if n:
            _check(self._lib, self._lib.bc_engine_rows(self._e, 0, n, s.ctypes.data, b.ctypes.data, c.ctypes.data))
        return s, b[:, :self.plan.barcode_num], c

    def result_rows(self):
        """sorted [(sample key, "b1,b2,..", count)] with sequences as keys, like Results (info.rs:661-665)"""
        if self.plan.mode == "sparse":
            n = C.c_uint64()
            _check(self._lib, self._lib.bc_engine_finish(self._e, C.byref(n)))
            sb, tb, cnt = C.create_string_buffer(64), C.create_string_buffer(1024), C.c_uint64()
            out = []
            for i in range(n.value):
                _check(self._lib, self._lib.bc_engine_row_text(self._e, i, sb, 64, tb, 1024, C.byref(cnt)))
                out.append((sb.value.decode(), tb.value.decode(), int(cnt.value)))
            return sorted(out)
        s, b, c = self.rows()
        samples = [x for x, _ in self.plan.samples()] if self.plan.sample_barcode else ["barcode"]
        sets = [[x for x, _ in self.plan.counted(i)] for i in range(self.plan.barcode_num)]
        out = []
        for i in range(len(c)):
            out.append((samples[s[i]], ",".join(sets[j][b[i, j]] for j in range(len(sets))), int(c[i])))
        return sorted(out)


class Comm:
    """The communicator of a multi-GPU job (bc_comm): one rank per GPU, ONE exchange at the job's end.
    Comm.rccl(id, rank, world, device): RCCL over xGMI -- rank 0 makes `id` with Comm.unique_id() and hands the bytes to
    the others (a file, a pipe, torch.distributed ...).  Comm.host(dir, rank, world): message files in a directory every
    rank can write to (any processes of one machine, several ranks on one GPU included)."""

    def __init__(self, handle, lib):
        self._c, self._lib = handle, lib

    @staticmethod
    def unique_id(lib=None):
        lib = lib or _lib.load()
        buf = C.create_string_buffer(_lib.BC_COMM_ID_BYTES)
        _check(lib, lib.bc_comm_unique_id(buf))
        return buf.raw

    @classmethod
    def rccl(cls, unique_id, rank, world, device, lib=None):
        lib = lib or _lib.load()
        assert len(unique_id) == _lib.BC_COMM_ID_BYTES
        h = lib.bc_comm_create(C.create_string_buffer(bytes(unique_id), _lib.BC_COMM_ID_BYTES), rank, world, int(device))
        if not h:
            raise BarcodeCountError(_lib.BC_ERR_COMM, _lib.last_error(lib))
        return cls(h, lib)

    @classmethod
    def host(cls, directory, rank, world, lib=None):
        lib = lib or _lib.load()
        h = lib.bc_comm_create_host(str(directory).encode(), rank, world)
        if not h:
            raise BarcodeCountError(_lib.BC_ERR_COMM, _lib.last_error(lib))
        return cls(h, lib)

    rank = property(lambda s: s._lib.bc_comm_rank(s._c))
    world = property(lambda s: s._lib.bc_comm_world(s._c))

    def barrier(self):
        _check(self._lib, self._lib.bc_comm_barrier(self._c))

    def sum_u64(self, values, root=0):
        """element-wise sum of a list of ints onto the root (the other ranks get their own values back)"""
        arr = (C.c_uint64 * len(values))(*values)
        _check(self._lib, self._lib.bc_comm_sum_u64(self._c, arr, len(values), root))
        return [int(x) for x in arr]

    def close(self):
        if getattr(self, "_c", None):
            self._lib.bc_comm_destroy(self._c)
            self._c = None

    __del__ = close


class Synth:
    """Counter-based synthetic read generator; identical on host and device."""

    def __init__(self, plan, seed, read_len=100, p_sub=0.0, p_n=0.0, p_lowq=0.0, phred=(30, 40), lowq=(2, 15),
                 n_molecules=0, zipf=False, geo_total=0):
        self._lib = plan._lib
        self.plan = plan
        f = lambda p: min(int(round(p * 4294967296.0)), 4294967295)
        self.params = SynthParams(seed, read_len, f(p_sub), f(p_n), f(p_lowq), phred[0], phred[1], lowq[0], lowq[1],
                                  n_molecules, 1 if zipf else 0, 0, geo_total)
        self._s = self._lib.bc_synth_create(plan._p, C.byref(self.params))
        if not self._s:
            raise BarcodeCountError(_lib.BC_ERR_INVALID, _lib.last_error(self._lib))

    def __del__(self):
        if getattr(self, "_s", None):
            self._lib.bc_synth_destroy(self._s)
            self._s = None

    def generate_host(self, first, n, stride=None):
        stride = stride or self.params.read_len
        seq = np.empty(n * stride, dtype=np.uint8)
        qual = np.empty(n * stride, dtype=np.uint8)
        _check(self._lib, self._lib.bc_synth_generate_host(self._s, first, n, seq.ctypes.data, qual.ctypes.data, stride))
        return seq, qual

    def generate_device(self, device, stream, first, n, d_seq, d_qual, stride=None):
        stride = stride or self.params.read_len
        _check(self._lib, self._lib.bc_synth_generate_device(self._s, device, stream, first, n, d_seq, d_qual, stride))


def bam_scan(path, lib=None):
    """the header of a BAM file, on the host: (references in its dictionary, inflated offset of the first record,
    inflated bytes)"""
    lib = lib or _lib.load()
    n_ref, first, size = C.c_uint32(), C.c_uint64(), C.c_uint64()
    _check(lib, lib.bc_bam_scan(str(path).encode(), C.byref(n_ref), C.byref(first), C.byref(size)))
    return n_ref.value, first.value, size.value


def orient_device(d_seq, d_qual, stride, read_len, n_out, d_seq_out, d_qual_out, d_lens=None, d_qlens=None, d_index=None,
                  d_lens_out=None, d_qlens_out=None, device=0, stream=None, lib=None):
    """bc_strand_orient_device: output read j = the reverse complement of read d_index[j] (None: read j) of a batch on
    the device, in the batch's own form.  Device pointers; only enqueues on `stream`."""
    lib = lib or _lib.load()
    _check(lib, lib.bc_strand_orient_device(int(device), stream, d_seq, d_qual, d_lens, d_qlens, stride, read_len, d_index,
                                            n_out, d_seq_out, d_qual_out, d_lens_out, d_qlens_out))


def make_set(seed, n, k, min_dist=1, lib=None):
    lib = lib or _lib.load()
    buf = C.create_string_buffer(n * (k + 1))
    rc = lib.bc_synth_make_set(seed, n, k, min_dist, buf)
    _check(lib, rc)
    raw = buf.raw
    return [raw[i * (k + 1):i * (k + 1) + k].decode() for i in range(n)]


def probe_atomic_rate(device, table_ptr, entries, n_atomics, lib=None):
    """random no-return atomic adds of 0 per second over a u32 table on this device (box diagnostic)"""
    lib = lib or _lib.load()
    v = C.c_double()
    _check(lib, lib.bc_probe_atomic_rate(int(device), table_ptr, entries, n_atomics, C.byref(v)))
    return v.value


def precompile(plan, stride=100, read_len=None, lens=False, cache_dir=None):
    """Builds the scheme-specialised match kernel of a plan for one batch shape ahead of time (no GPU needed) into
    the kernel cache (default: jit_cache/ next to the library), so that engines of this plan find it ready.
    stride / read_len as they will be passed to submit_*; lens = per-read lengths will be passed."""
    lib = plan._lib
    _check(lib, lib.bc_plan_precompile(plan._p, stride, stride if read_len is None else read_len, 1 if lens else 0,
                                       cache_dir.encode() if cache_dir else None))


def fix_error(mismatch_seq, possible_seqs, mismatches, device=0, lib=None):
    """fix_error (parse.rs:553-593) on the GPU: the unique nearest candidate or None."""
    lib = lib or _lib.load()
    possible_seqs = list(possible_seqs)
    arr = (C.c_char_p * max(len(possible_seqs), 1))(*[s.encode() for s in possible_seqs])
    r = lib.bc_fix_error(mismatch_seq.encode(), arr, len(possible_seqs), mismatches, device)
    if r < -1:
        raise BarcodeCountError(int(r) + 1, _lib.last_error(lib))
    return None if r < 0 else possible_seqs[r]


# ------------------------------------------------------------------------------------------------
# host-side mirror of the reference's types for this path
# ------------------------------------------------------------------------------------------------
class SequenceFormat:
    """info.rs:176-310"""

    def __init__(self, plan):
        self.plan = plan
        for f in ("format_string", "regions_string", "length", "constant_region_length", "barcode_num",
                  "barcode_lengths", "sample_length_option", "random_barcode", "sample_barcode"):
            setattr(self, f, getattr(plan, f))

    @classmethod
    def parse_format_file(cls, format_path):
        with open(format_path) as fh:
            return cls(Plan(fh.read()))

    @classmethod
    def from_text(cls, text):
        return cls(Plan(text))

    def __str__(self):  # Display, info.rs:313-335
        key, seen = "", set()
        names = {"S": "\nS: Sample barcode", "B": "\nB: Counted barcode", "C": "\nC: Constant region",
                 "R": "\nR: Random barcode"}
        for ch in self.regions_string:
            if ch not in seen:
                seen.add(ch)
                key += names.get(ch, "")
        return "-FORMAT-\n%s\n%s%s" % (self.format_string, self.regions_string, key)


class BarcodeConversions:
    """info.rs:338-457; the sets live in the plan of the SequenceFormat they belong to"""

    def __init__(self, sequence_format):
        self.plan = sequence_format.plan

    def sample_barcode_file_conversion(self, barcode_path):
        with open(barcode_path) as fh:
            self.plan.load_sample_csv(fh.read())

    def barcode_file_conversion(self, barcode_path, barcode_num=None):
        with open(barcode_path) as fh:
            self.plan.load_counted_csv(fh.read())

    samples_barcode_hash = property(lambda s: dict(s.plan.samples()))
    sample_seqs = property(lambda s: {x for x, _ in s.plan.samples()})
    counted_barcodes_hash = property(lambda s: [dict(s.plan.counted(i)) for i in range(s.plan.barcode_num)])
    counted_barcode_seqs = property(lambda s: [{x for x, _ in s.plan.counted(i)} for i in range(s.plan.barcode_num)])


class MaxSeqErrors:
    """info.rs:461-616"""

    def __init__(self, sample_errors_option, sample_barcode_size_option, barcode_errors_option, barcode_sizes,
                 constant_errors_option, constant_region_size, min_quality, lib=None):
        lib = lib or _lib.load()
        n = len(barcode_sizes)
        sizes = (C.c_uint16 * max(n, 1))(*barcode_sizes)
        out = (C.c_uint16 * (2 + max(n, 1)))()
        lib.bc_max_seq_errors(_opt(sample_errors_option), _opt(sample_barcode_size_option), _opt(barcode_errors_option),
                              sizes, n, _opt(constant_errors_option), constant_region_size, out)
        self._c, self._s, self._b = out[0], out[1], [out[2 + i] for i in range(n)]
        self.options = (sample_errors_option, barcode_errors_option, constant_errors_option)
        self.min_quality = min_quality

    def max_constant_errors(self):
        return self._c

    def max_sample_errors(self):
        return self._s

    def max_barcode_errors(self):
        return list(self._b)


class SequenceErrors:
    """info.rs:16-172; filled from the engine's device counters"""
    FIELDS = ["matched", "constant_region", "sample_barcode", "barcode", "duplicates", "low_quality"]

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, 0)

    def update(self, counters):
        for f in self.FIELDS:
            setattr(self, f, counters[f] & 0xFFFFFFFF)  # AtomicU32 (info.rs:17-22)

    def __str__(self):  # Display, info.rs:141-172
        g = lambda v: "{:,}".format(v)
        return ("Correctly matched sequences: %s\nConstant region mismatches:  %s\nSample barcode mismatches:   %s\n"
                "Counted barcode mismatches:  %s\nDuplicates:                  %s\nLow quality barcodes:        %s" %
                (g(self.matched), g(self.constant_region), g(self.sample_barcode), g(self.barcode), g(self.duplicates),
                 g(self.low_quality)))


class Results:
    """info.rs:669-808: results_hashmap[sample][\"b1,b2,..\"] = count"""

    def __init__(self, samples_barcode_hash, random_barcode, sample_barcode):
        self.results_hashmap = {}
        if samples_barcode_hash:
            for s in samples_barcode_hash:
                self.results_hashmap[s] = {}
        elif not sample_barcode:
            self.results_hashmap["barcode"] = {}

    def fill(self, rows):
        for sample, tup, count in rows:
            self.results_hashmap.setdefault(sample, {})[tup] = count


class ResultsEnrichment:
    """info.rs:811-904: single_hashmap / double_hashmap[sample key]["id1,,"] = count.  add_single / add_double build them
    from rows as the reference does; fill() builds them from the engine's device-side marginals (Engine.enrichment)."""

    def __init__(self):
        self.single_hashmap = {}
        self.double_hashmap = {}

    def add_sample_barcodes(self, samples_barcodes):
        for s in samples_barcodes:
            self.single_hashmap[s] = {}
            self.double_hashmap[s] = {}

    def add_single(self, sample_id, barcode_string, count):  # info.rs:840-866
        parts = barcode_string.split(",")
        m = self.single_hashmap.get(sample_id, {})  # (an unknown sample: the add lands in a temporary)
        for i in range(len(parts)):
            key = ",".join(parts[x] if x == i else "" for x in range(len(parts)))
            m[key] = m.get(key, 0) + count

    def add_double(self, sample_id, barcode_string, count):  # info.rs:869-904
        parts = barcode_string.split(",")
        n = len(parts)
        m = self.double_hashmap.get(sample_id, {})
        for a in range(n - 1):
            for b in range(a + 1, n):
                key = ",".join(parts[x] if x in (a, b) else "" for x in range(n))
                m[key] = m.get(key, 0) + count

    def add_marginals(self, sample_keys, ids, singles, doubles):
        """the maps from index marginals: sample_keys[s] = the key of sample s, ids[g][i] = the ID of sequence i of
        counted set g, singles / doubles as Engine.enrichment returns them.  Sequences that share an ID add up, and a key
        exists only where its sum is not zero (the reference makes one only when a row adds to it)."""
        G = len(ids)
        for s, key in enumerate(sample_keys):
            m = self.single_hashmap.get(key)
            if m is not None:
                for g in range(G):
                    row = singles[g][s]
                    for i in np.flatnonzero(row):
                        k = "," * g + ids[g][i] + "," * (G - 1 - g)
                        m[k] = m.get(k, 0) + int(row[i])
            m = self.double_hashmap.get(key)
            if m is not None:
                for (g, h), a in doubles.items():
                    a = a[s]
                    for i, j in zip(*np.nonzero(a)):
                        k = "," * g + ids[g][i] + "," * (h - g) + ids[h][j] + "," * (G - 1 - h)
                        m[k] = m.get(k, 0) + int(a[i, j])

    def fill(self, engine):
        """the maps of a dense plan's run from bc_engine_enrich, with the sample keys the reference's writers give them
        (add_sample_barcodes over the Results keys, output.rs:74-97): every sample of the sample file, else "barcode"
        when the scheme has no sample barcode -- and "barcode" also once a count lands there (a random-barcode run with a
        sample file but no sample barcode, info.rs:792-801).  Every such key gets its maps, empty or not."""
        plan = engine.plan
        samples = [x for x, _ in plan.samples()]
        results_keys = samples if samples else ([] if plan.sample_barcode else ["barcode"])
        table_keys = samples if plan.sample_barcode else ["barcode"]  # the key of each sample index of the table
        singles, doubles = engine.enrichment()
        for s, k in enumerate(table_keys):
            if k not in results_keys and singles and singles[0][s].any():
                results_keys = results_keys + [k]
        self.add_sample_barcodes([k for k in results_keys if k not in self.single_hashmap])
        ids = [[i for _, i in plan.counted(g)] for g in range(plan.barcode_num)]
        self.add_marginals(table_keys, ids, singles, doubles)
        return self


class SequenceParser:
    """parse.rs:15-163.  The worker pool of main.rs:93-120 becomes one engine per GPU; the queue of
    packed records (SharedMutData.seq) becomes batches of sequence / quality lines."""

    def __init__(self, results, sequence_errors, sequence_format, max_errors, min_quality_score, device=0):
        self.results = results
        self.sequence_errors = sequence_errors
        self.plan = sequence_format.plan
        so, bo, co = max_errors.options
        self.plan.set_max_errors(so, bo, co)
        self.plan.set_min_quality(min_quality_score)
        self.engine = Engine(self.plan, device)

    def parse(self, seq, qual, stride, read_len, lens=None):
        """one batch of reads from host arrays; call finish() after the last batch"""
        self.engine.submit_host(seq, qual, stride, read_len, lens)

    def finish(self):
        self.sequence_errors.update(self.engine.counters())
        self.results.fill(self.engine.result_rows())
