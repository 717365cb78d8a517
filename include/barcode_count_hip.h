/*
 * barcode_count_hip.h -- C ABI of the MI355X (gfx950) barcode match/count engine.
 *
 * Drop-in boundary for ONE path of Roco-scientist/NGS-Barcode-Count (crate
 * barcode-count v0.11.1): the per-read match/count loop of src/parse.rs
 * (SequenceParser::parse, parse.rs:53-76, and everything it calls) together
 * with Results::add_count (info.rs:735-808) and the six SequenceErrors
 * counters (info.rs:16-139).  The reference exposes no FFI of its own; these
 * entry points are what a Rust `extern "C"` block in the reference's
 * src/main.rs would bind in place of the rayon worker fan-out
 * (main.rs:93-120) -- see INTEGRATION.md for that binding.
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * All functions return BC_OK (0) or a negative status; bc_last_error() gives
 * the message of the calling thread's last failure.  Nothing here falls back
 * to a CPU implementation: an engine cannot be created without a HIP device.
 */
#ifndef BARCODE_COUNT_HIP_H
#define BARCODE_COUNT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BC_OK 0
#define BC_ERR_INVALID (-1)     /* the reference would return Err / panic on this input */
#define BC_ERR_UNSUPPORTED (-2) /* valid for the reference, not handled by this engine (message says what) */
#define BC_ERR_HIP (-3)         /* HIP runtime failure */
#define BC_ERR_NOMEM (-4)
#define BC_ERR_STATE (-5)       /* call order violated */
#define BC_ERR_COMM (-6)        /* the exchange between the ranks of a multi-GPU job failed (a peer is gone, I/O) */

/* outcome counters: SequenceErrors (info.rs:16-23) in Display order (info.rs:141-172),
 * then two engine-side extras */
enum {
  BC_MATCHED = 0,
  BC_CONSTANT_REGION = 1,
  BC_SAMPLE_BARCODE = 2,
  BC_BARCODE = 3,
  BC_DUPLICATES = 4,
  BC_LOW_QUALITY = 5,
  BC_TOTAL_READS = 6, /* reads submitted (input.rs:128-130 total_reads, minus the gz off-by-one) */
  BC_UNSUPPORTED_READS = 7, /* reads the engine cannot score exactly (non-ASCII bytes); always 0 for FASTQ */
  BC_NCOUNTERS = 8
};

typedef struct bc_plan bc_plan;     /* compiled scheme + known barcode sets + error budgets (host) */
typedef struct bc_engine bc_engine; /* one run on one GPU: device tables, stream, results */
typedef struct bc_synth bc_synth;   /* counter-based synthetic read generator */

const char *bc_version(void);
const char *bc_last_error(void);

/* ---- static run description ------------------------------------------------------------ */

/* SequenceFormat::parse_format_file (info.rs:215-310); `text` = content of the scheme file. */
bc_plan *bc_plan_create(const char *scheme_text, size_t len);
void bc_plan_destroy(bc_plan *p);
/* SequenceFormat fields (info.rs:176-187) */
const char *bc_plan_format_string(const bc_plan *p);
const char *bc_plan_regions_string(const bc_plan *p);
const char *bc_plan_regex_string(const bc_plan *p);
uint32_t bc_plan_length(const bc_plan *p);
uint32_t bc_plan_constant_region_length(const bc_plan *p);
uint32_t bc_plan_barcode_num(const bc_plan *p);
uint32_t bc_plan_barcode_length(const bc_plan *p, uint32_t i);
int32_t bc_plan_sample_length(const bc_plan *p); /* -1 = None */
int bc_plan_has_random(const bc_plan *p);
int bc_plan_has_sample(const bc_plan *p);

/* BarcodeConversions::sample_barcode_file_conversion + get_sample_seqs (info.rs:364-381, 435-441) */
int bc_plan_load_sample_csv(bc_plan *p, const char *csv_text, size_t len);
/* BarcodeConversions::barcode_file_conversion + get_barcode_seqs (info.rs:390-433, 444-456) */
int bc_plan_load_counted_csv(bc_plan *p, const char *csv_text, size_t len);
/* what the loaders insert, one entry at a time (a later duplicate sequence replaces the ID) */
int bc_plan_add_sample(bc_plan *p, const char *seq, const char *id);
int bc_plan_add_counted(bc_plan *p, uint32_t barcode_index, const char *seq, const char *id);
/* known sets in engine index order (index = position in first-insertion order) */
uint32_t bc_plan_n_samples(const bc_plan *p);
const char *bc_plan_sample_seq(const bc_plan *p, uint32_t i);
const char *bc_plan_sample_id(const bc_plan *p, uint32_t i);
uint32_t bc_plan_n_counted(const bc_plan *p, uint32_t barcode_index);
const char *bc_plan_counted_seq(const bc_plan *p, uint32_t barcode_index, uint32_t i);
const char *bc_plan_counted_id(const bc_plan *p, uint32_t barcode_index, uint32_t i);

/* MaxSeqErrors::new (info.rs:490-543); -1 = None (use 20 % of the length) */
int bc_plan_set_max_errors(bc_plan *p, int sample_errors, int barcode_errors, int constant_errors);
uint32_t bc_plan_max_constant_errors(const bc_plan *p);          /* info.rs:565 */
uint32_t bc_plan_max_sample_errors(const bc_plan *p);            /* info.rs:589 */
uint32_t bc_plan_max_barcode_errors(const bc_plan *p, uint32_t i); /* info.rs:613 */
/* free-standing form for the reference's doctest values: out[0]=constant, out[1]=sample, out[2..]=barcodes */
void bc_max_seq_errors(int sample_errors, int sample_size, int barcode_errors, const uint16_t *barcode_sizes,
                       uint32_t n_barcodes, int constant_errors, uint16_t constant_region_size, uint16_t *out);
/* --min-quality (arguments.rs:111-118); 0 = filter off (parse.rs:98) */
int bc_plan_set_min_quality(bc_plan *p, float min_quality);
/* integer score-sum threshold equivalent to the f32 mean test of parse.rs:352-355 for a run of n
 * bases: low quality <=> sum(scores) < T_n */
uint32_t bc_plan_quality_threshold(const bc_plan *p, uint32_t run_len);

/* Which orientation of a read is counted (the reference has no such option; MAGeCK's --reverse-complement is one).
 * rc(read): the sequence line reversed over its own length, every byte through the complement table -- the IUPAC pairs
 * A-T C-G M-K R-Y V-B H-D in either case; W S N w s n and every other byte (>= 0x80 included) map to themselves -- and
 * the quality line reversed over ITS own length (the two can differ, bc_engine_submit_device_q).  It is what the BAM
 * path hands on for a record flagged 0x10 and what `samtools fastq` writes for it.
 *   BC_STRAND_FORWARD (default): reads are counted as they stand.
 *   BC_STRAND_REVERSE: every read is counted as rc(read); nothing else changes.
 *   BC_STRAND_BOTH: a read is judged as it stands first.  Any outcome but BC_CONSTANT_REGION is its outcome -- forward
 *     wins, even where rc(read) would match too; a BC_CONSTANT_REGION read's outcome is that of rc(read), whatever that
 *     is (BC_CONSTANT_REGION again is possible).
 * Every read adds one to BC_TOTAL_READS and one to exactly one other counter; bc_engine_counters never shows a read
 * twice.  Both orientations count into one Results: a random-barcode key seen forward makes the same molecule seen in
 * reverse a duplicate.  For unaligned BAM from a basecaller (no 0x10 flags), non-directional amplicon preps, or an R2
 * file.  BC_ERR_INVALID for another value.  Read when an engine is created: a later change does not reach that engine. */
#define BC_STRAND_FORWARD 0
#define BC_STRAND_REVERSE 1
#define BC_STRAND_BOTH 2
int bc_plan_set_strand(bc_plan *p, int strand);
int bc_plan_strand(const bc_plan *p);

/* ---- engine ---------------------------------------------------------------------------- */

/* Number of u32 entries of the dense per-(sample, barcode tuple) counter table the plan needs
 * (product of the set sizes); 0 when the plan cannot use a dense table. */
uint64_t bc_plan_table_entries(const bc_plan *p);

/* Replaces SequenceParser::new (parse.rs:28-52) for all workers of one device.  `hip_stream`
 * (a hipStream_t) may be NULL: the engine then owns a stream.  `table_mem` may point to
 * caller-owned device memory of bc_plan_table_entries()*4 bytes (zeroed by the caller), so the
 * caller can reduce it across devices with RCCL; NULL lets the engine allocate it. */
bc_engine *bc_engine_create(const bc_plan *p, int device_id, void *hip_stream, void *table_mem);
void bc_engine_destroy(bc_engine *e);

/* One batch of reads = the records the reference's workers pop from SharedMutData.seq
 * (parse.rs:78-86), already split into the sequence line and the quality line.
 * Layout: read i occupies bytes [i*stride, i*stride+len_i) of `seq` and of `qual`
 * (ASCII, as in the FASTQ); len_i = lens[i] or read_len when lens is NULL.  qual may be NULL
 * only when the quality filter is off.  Both buffers must be 16-byte aligned.
 * _device: pointers are device memory; the call only enqueues work on the engine's stream -- under BC_STRAND_FORWARD and
 * BC_STRAND_REVERSE.  Under BC_STRAND_BOTH it no longer "only enqueues": per chunk of BC_STRAND_CHUNK reads (default
 * 2^24, a multiple of 256) the host waits once for the first pass, to learn how many reads go to the second; the
 * caller's buffers are still read after the call returns (the last chunk's second pass), as before.
 * The engine's scratch for the reversed reads grows on demand to one chunk -- per read 2 * stride + 4 bytes, and with
 * BC_STRAND_BOTH 13 more (the list, the outcome byte, the index the traced kernels write) -- and is freed with it.
 * _host: pointers are host memory; the engine stages them through pinned buffers with
 * hipMemcpyAsync on a side stream and returns when the host buffers may be reused. */
int bc_engine_submit_device(bc_engine *e, const void *d_seq, const void *d_qual, const void *d_lens, uint32_t stride,
                            uint32_t read_len, uint64_t n_reads);
/* The same for records whose quality line is not as long as their sequence line (trimmed or damaged files): the
 * reference zips the scores with the regions (parse.rs:340-345), so what counts is the quality line's own length.
 * d_lens / d_qlens: u16 per read, both required; the first min(qlen, stride) quality bytes are stored at the stride. */
int bc_engine_submit_device_q(bc_engine *e, const void *d_seq, const void *d_qual, const void *d_lens, const void *d_qlens,
                              uint32_t stride, uint64_t n_reads);
/* the engine's stream (a hipStream_t) and device, for callers that produce batches on the device themselves */
void *bc_engine_hip_stream(bc_engine *e);
int bc_engine_device(const bc_engine *e);
int bc_engine_submit_host(bc_engine *e, const void *seq, const void *qual, const uint16_t *lens, uint32_t stride,
                          uint32_t read_len, uint64_t n_reads);
int bc_engine_sync(bc_engine *e);
/* zero the table and the counters (a fresh Results::new, info.rs:678) */
int bc_engine_reset(bc_engine *e);
/* the same without the outcome counters: a fresh Results (table, bit map, key set / map) for the next sample of a run
 * whose SequenceErrors go on counting.  Large engine-owned tables are reset by the blocks that were touched (they are
 * almost all zeros after a job: first occurrences live in the bit map), not by a 16 GB memset. */
int bc_engine_reset_results(bc_engine *e);

/* SequenceErrors values (u64; the reference wraps at 2^32, info.rs:17-22) */
int bc_engine_counters(bc_engine *e, uint64_t out[BC_NCOUNTERS]);
/* device pointers, for cross-device reduction by the caller (RCCL sum over u32 / u64).  The table holds plain u32
 * counts when this returns and again after every later bc_engine_sync (large tables count on two levels in between,
 * bc_kernel.h: taking the pointer makes every sync fold them, as for a caller-owned table). */
void *bc_engine_table_ptr(bc_engine *e);
void *bc_engine_counters_ptr(bc_engine *e);
uint64_t bc_engine_table_entries(const bc_engine *e);

/* Compacts the non-zero table entries on the device; rows are then readable in any order.
 * A row = (sample index, barcode index per counted barcode, count): the (sample, tuple, count)
 * triples Results holds (info.rs:661-665), with indices into the plan's known sets.
 * Device memory is bounded whatever the table holds: the table is compacted range by range through two staging
 * buffers of BC_FINISH_CHUNK_ROWS rows (default 2^22; 12 bytes per row on the device and pinned).  bc_engine_finish
 * keeps all rows on the host (12 bytes per row; BC_ERR_NOMEM when that does not fit). */
int bc_engine_finish(bc_engine *e, uint64_t *n_rows);
int bc_engine_rows(bc_engine *e, uint64_t first, uint64_t n, uint32_t *sample_idx, uint32_t *barcode_idx,
                   uint64_t *count);
/* The same compaction with the rows handed to `fn` chunk by chunk as they leave the device (nothing is kept: host
 * memory is bounded too).  A chunk is n (key, count) pairs valid during the call; key = the dense table index
 * (bc_engine_decode_index turns it into set indices) or, for plans that keep raw captures, the tuple key.  fn returns 0
 * to go on; anything else stops the compaction (BC_ERR_STATE). */
typedef int (*bc_rows_fn)(const uint64_t *key, const uint32_t *count, uint64_t n, void *user);
int bc_engine_finish_stream(bc_engine *e, bc_rows_fn fn, void *user, uint64_t *n_rows);
int bc_engine_decode_index(const bc_engine *e, uint64_t dense_index, uint32_t *sample_idx, uint32_t *barcode_idx);
/* number of rows bc_engine_finish would produce now (dense plans without a random barcode): one sweep of the table,
 * nothing is moved */
int bc_engine_nonzero_entries(bc_engine *e, uint64_t *n);

/* Single and double barcode enrichment (`--enrich`, ResultsEnrichment of info.rs:811-904) of a dense plan, computed on
 * the device as index sums of the counts bc_engine_finish would hand out now: one pass over the table (and the bit map
 * of two-level counting), random-barcode plans materialized first as bc_engine_finish does, the root's summed table
 * after bc_engine_finish_all.  The table, the counters and the rows stay as they are; the call may come before or after
 * bc_engine_finish, and more than once.
 * Layout, with G = the number of counted barcodes, N_g = the size of known set g (engine index order),
 * S = table_entries / (N_0 * .. * N_{G-1}) (the plan's sample count with a sample group, else 1), s = sample index and
 * i_g = index into set g:
 *   singles: single_counts[s * SUM + off_g + i_g], SUM = N_0 + .. + N_{G-1}, off_g = N_0 + .. + N_{g-1};
 *   pairs in the order add_double produces them (info.rs:869-904): (0,1), (0,2), .., (0,G-1), (1,2), .., (G-2,G-1);
 *   doubles: double_counts[s * P + poff_(g,h) + i_g * N_h + i_h], P = sum over pairs of N_g * N_h, poff_(g,h) = that
 *   sum over the pairs before (g,h).
 * All counts are u64 (marginals of u32 entries pass 2^32).  Doubles exist only for G >= 3 (the reference writes Double
 * files only then, output.rs:176, 349): double_entries = 0 below.  A key of the reference's maps exists where its sum
 * is not zero.  Device scratch: S * (SUM + P) * 8 bytes (BC_ERR_NOMEM when that cannot be allocated).
 * Plans that keep raw captures (bc_plan_mode 2) have no index form: BC_ERR_UNSUPPORTED. */
/* sizes of bc_engine_enrich's outputs, in u64 entries: S * SUM and S * P */
int bc_engine_enrich_entries(const bc_engine *e, uint64_t *single_entries, uint64_t *double_entries);
/* host pointers of those sizes; double_counts may be NULL (pairs are then skipped) */
int bc_engine_enrich(bc_engine *e, uint64_t *single_counts, uint64_t *double_counts);

/* The counts files of a dense plan as CSV text, written on the device from the counts bc_engine_finish would hand out
 * now: the same preamble as bc_engine_enrich (submits waited for, a random-barcode plan materialized, the bit map of
 * two-level counting read as it stands, the root's summed table after bc_engine_finish_all).  The table, the counters and
 * the rows stay as they are; the calls may come before or after bc_engine_finish, and more than once.
 * Layout, with G = the number of counted barcodes, T = N_0 * .. * N_{G-1} tuples per sample, id_g = the ID
 * (bc_plan_counted_id) of the tuple's index into set g, copied byte for byte:
 *   bc_engine_render_counts: for sample index s (0 for a plan without a sample group) one line per tuple whose count is
 *     not zero:  id_0,id_1,..,id_{G-1},count\n
 *   bc_engine_render_merged: for the ordered list sample_idx[0 .. n_samples) (a sample may come twice; any order) one
 *     line per tuple for which some LISTED sample counts:  id_0,..,id_{G-1},c_0,c_1,..\n  with c_k the count of sample
 *     sample_idx[k], 0 written as "0".
 * Order: ascending tuple index t = sum_g i_g * prod_{k>g} N_k (the dense index within the sample's slice; the last
 * counted barcode varies fastest), so the text is the same on every run.  No header line.
 * The text reaches `fn` in chunks of at most BC_RENDER_CHUNK_BYTES (default 64 MiB; never less than the longest
 * possible line) through two staging buffers, the device writing one while fn reads the other; device memory is those
 * two buffers + 12 bytes per 1024 tuples (BC_ERR_NOMEM when that cannot be allocated; the engine stays usable).
 * Plans that keep raw captures (bc_plan_mode 2) have no index form: BC_ERR_UNSUPPORTED. */
/* a chunk of text, valid during the call; always ends with '\n'; return 0 to go on, else the render stops (BC_ERR_STATE) */
typedef int (*bc_text_fn)(const char *text, size_t n, void *user);
/* n_rows (may be NULL): the number of lines */
int bc_engine_render_counts(bc_engine *e, uint32_t sample_idx, bc_text_fn fn, void *user, uint64_t *n_rows);
int bc_engine_render_merged(bc_engine *e, const uint32_t *sample_idx, uint32_t n_samples, bc_text_fn fn, void *user,
                            uint64_t *n_rows);

/* The Single and Double enrichment files of a dense plan as CSV text, written on the device from the sums
 * bc_engine_enrich computes (same notation: G, N_g, SUM, P, off_g, poff), with the preamble, the chunking and the callback
 * contract of bc_engine_render_counts / _merged (BC_RENDER_CHUNK_BYTES, two staging buffers, `fn` != 0 -> BC_ERR_STATE
 * with the engine still usable, BC_ERR_NOMEM likewise; the table, the counters and the rows stay as they are; no header).
 * A key is an index k into one sample's slice of the sums; lines come in ascending k:
 *   BC_ENRICH_SINGLE: k in [0, SUM) = off_g + i_g;  BC_ENRICH_DOUBLE: k in [0, P) = poff_(g,h) + i_g * N_h + i_h (none
 *   for G < 3: zero lines, BC_OK).
 * A line has G fields joined by commas, as add_single / add_double build the key (info.rs:840-904): field g (and h)
 * holds the ID, copied byte for byte, every other field is empty; then the count(s), u64 in decimal.  G = 3, g = 1:
 *   ,id,,count\n
 *   bc_engine_render_enriched: one line per key whose sum for sample_idx is not zero.
 *   bc_engine_render_enriched_merged: one line per key whose sum is not zero for some LISTED sample, one count per
 *     listed sample (any order, a sample may come twice), 0 written as "0".
 * Entries of one known set whose IDs are byte-equal are ONE key (the reference's maps are keyed by text): their sums are
 * folded, on the device, into the entry with the smallest index, and only that entry has a line.  Text that coincides
 * across DIFFERENT groups or pairs -- possible only when some ID is empty -- is NOT merged: write such plans from
 * bc_engine_enrich on the host.
 * The sums are computed once (one pass over the table) and kept on the device, S * (SUM + P) * 8 bytes, until
 * something changes what bc_engine_finish would hand out: a submit, a reset, a key or count import, bc_engine_clear_keys,
 * bc_engine_materialize_table, the exchange of bc_engine_finish_all.  A table the caller owns or has taken the pointer
 * of (bc_engine_table_ptr) may change unseen: its sums are computed anew for every call.  bc_engine_enrich is not
 * affected: it returns the raw, unfolded sums from scratch of its own.
 * Plans that keep raw captures: BC_ERR_UNSUPPORTED; another kind, or a sample index out of range: BC_ERR_INVALID. */
#define BC_ENRICH_SINGLE 1
#define BC_ENRICH_DOUBLE 2
/* How many times the engine has computed those sums (one pass over the table each) since it was created: the renders of
 * one state of the counts make one pass between them; every render of a table the caller can write makes its own.
 * Read-only: does not wait for the device. */
int bc_engine_enrich_render_passes(const bc_engine *e, uint64_t *n);
int bc_engine_render_enriched(bc_engine *e, int kind, uint32_t sample_idx, bc_text_fn fn, void *user, uint64_t *n_rows);
int bc_engine_render_enriched_merged(bc_engine *e, int kind, const uint32_t *sample_idx, uint32_t n_samples, bc_text_fn fn,
                                     void *user, uint64_t *n_rows);

/* The counts files of a raw-key plan (bc_plan_mode 2: some counted barcode has no conversion file, so its capture is
 * the key) as CSV text, written on the device from the counts bc_engine_finish would hand out now: the submits waited
 * for, a random-barcode plan's key set aggregated into per-tuple distinct counts, the root's merged map after
 * bc_engine_finish_all.  The map, the counters and the rows stay as they are; the calls may come before or after
 * bc_engine_finish, and more than once.
 * Layout, with G = the number of counted barcodes; field f_g = the ID (bc_plan_counted_id), copied byte for byte, when
 * barcode g has a known set, else the capture's bases as they were read (A, C, T, G, N):
 *   bc_engine_render_raw_counts: for sample index s (0 for a plan without a sample group) one line per tuple the sample
 *     counts:  f_0,f_1,..,f_{G-1},count\n
 *   bc_engine_render_raw_merged: for the ordered list sample_idx[0 .. n_samples) (a sample may come twice; any order)
 *     one line per tuple for which some LISTED sample counts:  f_0,..,f_{G-1},c_0,c_1,..\n  with c_k the count of sample
 *     sample_idx[k], 0 written as "0".
 * Order: lines ascend by the tuple (d_0, .., d_{G-1}) compared barcode by barcode, Barcode_1 first; d_g is the index
 * into the set for a known barcode and, for a raw one, the number  sum_k c_k * 5^k  over its bases with A, C, T, G, N =
 * 0 .. 4 and k the base's position from 0 (so captures compare from their LAST base backwards).  The order is made by a
 * radix sort on the device (24.5 bytes per row while it runs), and the text is the same on every run.  No header line.
 * The sorted rows stay on the device, 12 bytes per key the map may hold, until something changes what bc_engine_finish
 * would hand out (a submit, a reset, a key or count import, bc_engine_clear_keys, the exchange of bc_engine_finish_all):
 * the renders of one state of the counts share one sort.
 * Chunking, BC_RENDER_CHUNK_BYTES, the callback contract (`fn` != 0 -> BC_ERR_STATE, the engine still usable) and
 * BC_ERR_NOMEM are those of bc_engine_render_counts.
 * BC_ERR_UNSUPPORTED: a dense plan (use bc_engine_render_counts / _merged); a plan with wide keys
 * (bc_engine_key_words() > 1: bc_engine_render_wide_counts / _merged below render those; the message still names the
 * host path) or whose SAMPLE barcode is kept raw (its sample keys are captures, not indices, info.rs:742-757) -- write
 * those from bc_engine_finish + bc_engine_row_text on the host.  BC_ERR_INVALID: a sample index out of range, a null
 * callback, a null list with n_samples != 0. */
int bc_engine_render_raw_counts(bc_engine *e, uint32_t sample_idx, bc_text_fn fn, void *user, uint64_t *n_rows);
int bc_engine_render_raw_merged(bc_engine *e, const uint32_t *sample_idx, uint32_t n_samples, bc_text_fn fn, void *user,
                                uint64_t *n_rows);
/* How many sorts the engine has made for those renders since it was created.  Read-only: does not wait for the device. */
int bc_engine_raw_render_sorts(const bc_engine *e, uint64_t *n);
/* Device time of the last of them (export of the map, re-key, sort), in milliseconds, from HIP events; 0 before any. */
int bc_engine_raw_render_sort_ms(const bc_engine *e, double *ms);

/* The counts files of a wide-key plan (bc_engine_key_words() > 1: some counted barcode without a conversion file is longer
 * than 27 bases, or the captures overflow one 64-bit key together -- README.md "Barcode-seq") as CSV text, written on the
 * device.  Lines, layout, order and counts are those of bc_engine_render_raw_counts / _merged above, word for word: the
 * digit of a raw capture is still  sum_k c_k * 5^k  (it no longer fits a word, the order is the same: captures compare
 * from their LAST base backwards, A < C < T < G < N), so a scheme's files keep their order when a capture grows from 27
 * to 28 bases.  For a random-barcode plan the count of a tuple is the number of its distinct random barcodes.
 * The order is made on the device: the map is exported as bc_engine_finish exports it, every key is given an order key
 * of K <= bc_engine_key_words() - 1 u64, the order keys are sorted word by word (a stable radix sort per word), and keys
 * and counts are gathered into that order.  W = bc_engine_key_words(): at most (W + K) * 8 + 28.5 bytes per row while it
 * runs, W * 8 + 4 bytes per row kept on the device afterwards, until something changes what bc_engine_finish would hand
 * out: the renders of one state of the counts share one sort.
 * Calls before or after bc_engine_finish, and more than once; on the root after bc_engine_finish_all they render the
 * job's merged map.  Chunking, BC_RENDER_CHUNK_BYTES, the callback contract (`fn` != 0 -> BC_ERR_STATE, the engine still
 * usable) and BC_ERR_NOMEM are those of bc_engine_render_counts.
 * BC_ERR_UNSUPPORTED: a dense plan (use bc_engine_render_counts / _merged); a raw-key plan with one-word keys (use
 * bc_engine_render_raw_counts / _merged); a plan whose SAMPLE barcode is kept raw (write it from bc_engine_finish +
 * bc_engine_row_text on the host); 2^32 - 2048 rows or more.  BC_ERR_INVALID: a sample index out of range, a null
 * callback, a null list with n_samples != 0. */
int bc_engine_render_wide_counts(bc_engine *e, uint32_t sample_idx, bc_text_fn fn, void *user, uint64_t *n_rows);
int bc_engine_render_wide_merged(bc_engine *e, const uint32_t *sample_idx, uint32_t n_samples, bc_text_fn fn, void *user,
                                 uint64_t *n_rows);
/* How many sorts the engine has made for those renders since it was created.  Read-only: does not wait for the device. */
int bc_engine_wide_render_sorts(const bc_engine *e, uint64_t *n);
/* Device time of the last of them (export of the map, order keys, sort, gather), in milliseconds, from HIP events; 0
 * before any. */
int bc_engine_wide_render_sort_ms(const bc_engine *e, double *ms);

/* The Single and Double enrichment files of a raw-key plan (bc_plan_mode 2, one-word keys) as CSV text, written on the
 * device: what bc_engine_render_enriched / _merged are to a dense plan.  `kind` is BC_ENRICH_SINGLE or BC_ENRICH_DOUBLE.
 * The sums are made from the sorted rows of bc_engine_render_raw_counts (the same sort is shared; nothing else is exported
 * from the map): per counted barcode g (Single) or pair g < h (Double, in add_double's order (0,1), (0,2), .., (1,2), ..)
 * every row is projected to the key  d_g * S + s  or  (d_g * R_h + d_h) * S + s  (d: the digit bc_engine_render_raw_counts
 * orders by -- the set index of a known barcode, sum_k c_k * 5^k of a raw one; R_h: barcode h's radix; s: the sample index
 * of S), the projected keys are sorted over their own bit length and every run of equal keys is reduced to its u64 sum,
 * all on the device.  Entries of one known set whose IDs are byte-equal are ONE key, as in the dense call: their digit is
 * the smallest index with that ID.  Text that coincides across DIFFERENT barcodes or pairs -- possible only when some ID is
 * empty -- is NOT merged.
 * A line has G fields joined by commas, as add_single / add_double build the key (info.rs:840-904): field g (and h) holds
 * the ID of a known barcode, copied byte for byte, or the bases of a raw capture as they were read; every other field is
 * empty; then the sum(s), u64 in decimal.  Three raw barcodes of 8 bases:
 *   ,ACGTACGT,,7\n           Single of barcode 2          ACGTACGT,,TTGCAAGC,3\n   Double of barcodes 1 and 3
 *   bc_engine_render_raw_enriched: one line per key that sample_idx counts.
 *   bc_engine_render_raw_enriched_merged: one line per key whose sum is not zero for some LISTED sample, one sum per listed
 *     sample (any order, a sample may come twice), 0 written as "0".
 * Order: Single lines ascend by (g, d_g), Double lines by (pair, d_g, d_h); the text is the same on every run.  No header.
 * BC_ENRICH_DOUBLE with fewer than three counted barcodes, and an engine nothing was submitted to: no line, BC_OK.
 * Each kind is built once per state of the counts, at its first render, and kept on the device -- 16 bytes per (key,
 * sample) that counts, plus the segment starts -- until the sorted rows are retired (a submit, a reset, a key or count
 * import, bc_engine_clear_keys, the exchange of bc_engine_finish_all).  While a kind is built: 32.5 bytes per row
 * beside the sorted rows (one set of buffers that every projection uses in turn), released before the render.  On the root after bc_engine_finish_all the calls render the job's
 * merged map.
 * Chunking, BC_RENDER_CHUNK_BYTES, the callback contract (`fn` != 0 -> BC_ERR_STATE, the engine still usable) and
 * BC_ERR_NOMEM (everything taken is released) are those of bc_engine_render_raw_counts.
 * BC_ERR_UNSUPPORTED: a dense plan (use bc_engine_render_enriched / _merged); a plan with wide keys
 * (bc_engine_key_words() > 1) or whose SAMPLE barcode is kept raw -- build those files from bc_engine_finish +
 * bc_engine_row_text on the host.  BC_ERR_INVALID: another kind, a sample index out of range, a null callback, a null
 * list with n_samples != 0. */
int bc_engine_render_raw_enriched(bc_engine *e, int kind, uint32_t sample_idx, bc_text_fn fn, void *user, uint64_t *n_rows);
int bc_engine_render_raw_enriched_merged(bc_engine *e, int kind, const uint32_t *sample_idx, uint32_t n_samples,
                                         bc_text_fn fn, void *user, uint64_t *n_rows);
/* How many kinds the engine has built for those renders since it was created (+1 for the Single set, +1 for the Double
 * set, per state of the counts).  Read-only: does not wait for the device. */
int bc_engine_raw_enrich_reduces(const bc_engine *e, uint64_t *n);
/* Device time of the last build (every projection of one kind: project, sort, reduce, join), in milliseconds, from HIP
 * events; 0 before any. */
int bc_engine_raw_enrich_reduce_ms(const bc_engine *e, double *ms);

/* Row i as the reference's Results holds it (info.rs:661-665): the sample key (a sample barcode
 * sequence, or "barcode" without a sample group) and the counted barcodes "b1,b2,.." as sequences.
 * Works for every plan, including those that keep raw captures (no sample / counted-barcode
 * file: README.md "Barcode-seq"), whose rows have no index form. */
int bc_engine_row_text(bc_engine *e, uint64_t row, char *sample, size_t sample_cap, char *tuple, size_t tuple_cap,
                       uint64_t *count);
/* 0: the engine cannot run the plan (bc_last_error says why); 1: dense counter table;
 * 2: hash map of tuple keys (some barcode is kept raw because no conversion file names it) */
int bc_plan_mode(const bc_plan *p);

/* Random-barcode schemes (PCR-duplicate collapse, Results::add_count info.rs:770-802): the engine
 * keeps the set of distinct (sample, barcode tuple, random barcode) keys in a device hash set; a
 * read whose key is already present counts as BC_DUPLICATES (parse.rs:65-69) and the count of a
 * tuple is the number of its distinct random barcodes (output.rs:265-270; bc_engine_finish turns
 * the set into the dense table).  A key is tuple_index * 5^len + base-5 code of the random barcode
 * (A,C,T,G,N = 0..4).  Across GPUs a sum of tables would be wrong: export the
 * keys, exchange them so that every key has one owner, import, then reduce.  Device pointers. */
/* Plans whose captures kept raw (no conversion file) or whose random barcode do not fit that 64-bit key -- more than 27
 * bases, or several captures that overflow it together -- count under WIDE keys of bc_engine_key_words() u64 each (word
 * 0 a fingerprint of the rest, then the captures as bit planes; csrc/bc_long.h): everywhere below a key is then that
 * many consecutive u64, and a buffer of n keys holds n * bc_engine_key_words() of them.  Such plans run on the
 * wave-per-read kernel and hand their rows out as text (bc_engine_row_text). */
uint32_t bc_engine_key_words(const bc_engine *e);
int bc_engine_key_count(bc_engine *e, uint64_t *n);
int bc_engine_export_keys(bc_engine *e, void *d_keys, uint64_t capacity, uint64_t *n);
int bc_engine_import_keys(bc_engine *e, const void *d_keys, uint64_t n, uint64_t *n_new);
int bc_engine_clear_keys(bc_engine *e);
/* Dense table + random barcode, several GPUs: after the key exchange every rank turns ITS (owned) keys into per-tuple
 * distinct counts in its table with bc_engine_materialize_table; the tables are then summed onto the root
 * (distributed.reduce_table), whose bc_engine_finish compacts the summed table as it stands.  (On one GPU
 * bc_engine_finish materializes by itself.)  Any later submit / import / clear invalidates the materialized table. */
int bc_engine_materialize_table(bc_engine *e);
/* Plans that keep raw captures and have NO random barcode count in a (key -> count) map.  Across GPUs
 * the maps are merged by sending every (key, count) pair to the key's owner (or all of them to the
 * root), where bc_engine_import_counts adds them in.  export with NULL buffers only counts the pairs.
 * Device pointers: keys u64, counts u32. */
int bc_engine_export_counts(bc_engine *e, void *d_keys, void *d_counts, uint64_t capacity, uint64_t *n);
int bc_engine_import_counts(bc_engine *e, const void *d_keys, const void *d_counts, uint64_t n);

/* Dense counts for the wire.  out[i] = table[i] where that fits a byte, else 0 with (i, table[i]) appended to the
 * overflow list; *n_ovf = entries the list needs (call again with a larger one if it exceeds ovf_capacity).  The
 * receiver adds the bytes up and then the list entries -- exact for any counts, a quarter of the bytes when counts
 * are small (ngs-barcode-count_amd/distributed.py reduce_table).  Device pointers; runs on hip_stream and waits. */
int bc_table_pack_u8(const void *d_table_u32, uint64_t n, void *d_out_u8, void *d_ovf_idx_u64, void *d_ovf_val_u32,
                     uint64_t ovf_capacity, uint64_t *n_ovf, int device_id, void *hip_stream);

/* ... and the receiving side of the exchange: out[i] = sum of the n_rows byte slices rows[r * n + i], i < n
 * (n a multiple of 4). */
int bc_table_sum_u8(const void *d_rows_u8, uint32_t n_rows, uint64_t n, void *d_out_u32, int device_id, void *hip_stream);

/* ---- several GPUs: one process (or thread) per GPU, one exchange at the end of the job ----------
 * The reference is one process whose workers share one Results map (main.rs:93-120).  Across GPUs every rank counts
 * its own shard of the reads into its own engine -- no communication on the data path -- and the job ends with ONE
 * collective call on every rank, after which the root's engine holds the job's result:
 *   - dense table, no random barcode: the u32 tables are summed onto the root (all-to-all of byte-packed slices, local
 *     sums, slices to the root: one xGMI link per peer, never a ring);
 *   - random barcode: the (tuple, random) keys first go to one owner rank each, where duplicates across ranks collapse
 *     (a sum of set sizes would be wrong, output.rs:265-270); the owners' per-tuple distinct counts then add up;
 *   - captures kept raw: every rank's (key, count) pairs / keys go to the root's map.
 * A communicator is either RCCL over xGMI (bc_comm_create: ncclSend / ncclRecv on the engine's stream; rank 0 makes the
 * id with bc_comm_unique_id and hands its BC_COMM_ID_BYTES bytes to the other ranks by whatever means the caller has --
 * a file, a pipe, MPI) or message files in a directory all ranks can write to (bc_comm_create_host: works between any
 * processes of one machine, several ranks on ONE GPU included; device buffers are staged through host memory).
 * counters (may be NULL): the job's outcome counters on the root, zeros elsewhere.  The tables of the other ranks are
 * left in an unspecified state.  Tables must be 16-byte aligned (engine-owned ones are). */
typedef struct bc_comm bc_comm;
#define BC_COMM_ID_BYTES 128
int bc_comm_unique_id(void *id_out);
bc_comm *bc_comm_create(const void *id, int rank, int world, int device_id);
bc_comm *bc_comm_create_host(const char *dir, int rank, int world);
void bc_comm_destroy(bc_comm *c);
int bc_comm_rank(const bc_comm *c);
int bc_comm_world(const bc_comm *c);
int bc_comm_barrier(bc_comm *c);
/* element-wise sum of n u64 onto the root (e.g. the shards' "Total sequences"); the other ranks' values stay */
int bc_comm_sum_u64(bc_comm *c, uint64_t *vals, int n, int root);
/* the exchange alone: afterwards the root's table / key set / key map is the job's */
int bc_engine_reduce_all(bc_engine *e, bc_comm *c, int root, uint64_t counters[BC_NCOUNTERS]);
/* ... followed by bc_engine_finish on the root (rows readable there; *n_rows = 0 on the other ranks).  c = NULL or a
 * communicator of one rank: the same as bc_engine_counters + bc_engine_finish. */
int bc_engine_finish_all(bc_engine *e, bc_comm *c, int root, uint64_t counters[BC_NCOUNTERS], uint64_t *n_rows);
/* the plan an engine was created from */
const bc_plan *bc_engine_plan(const bc_engine *e);

/* Debug / parity-test hook: the next submits also write, for read i of the submit, its outcome
 * (BC_* counter index; BC_MATCHED = passed every test) to d_outcome_u8[i] and its dense table index
 * to d_index_u64[i].  Both device pointers; NULL switches tracing off.  Under BC_STRAND_REVERSE / _BOTH read i receives
 * its FINAL outcome and index at its own position i, whichever orientation decided it. */
int bc_engine_trace(bc_engine *e, void *d_outcome_u8, void *d_index_u64);
/* The reads handed to the reverse pass since the engine was created -- all of them under BC_STRAND_REVERSE, the forward
 * constant-region failures under BC_STRAND_BOTH, 0 under BC_STRAND_FORWARD -- and how many of those ended BC_MATCHED.
 * (Under a random-barcode plan either sighting of a molecule may be the BC_MATCHED one, so the second number depends on
 * the order the device counted them in; the counters and rows do not.)  Neither is zeroed by a reset.  Either pointer may be NULL.  Waits for the engine's stream (the two numbers are kept on
 * the device), except under BC_STRAND_FORWARD. */
int bc_engine_strand_reads(const bc_engine *e, uint64_t *retried, uint64_t *matched_reverse);

/* HIP-event timing of the match/count kernel on the engine's stream (for the roofline) */
int bc_engine_timing(bc_engine *e, int enable);
int bc_engine_kernel_ms(bc_engine *e, double *total_ms, uint64_t *launches);   /* sum since the last call; resets */
/* the same launches one by one, in launch order (up to `capacity` of them; *launches = how many there are); does not
 * reset: call it before bc_engine_kernel_ms */
int bc_engine_kernel_ms_each(bc_engine *e, double *ms_out, uint64_t capacity, uint64_t *launches);
/* Which kernel the last submit launched: "match_count_kernel<NW,NWW>" (the generic one, any plan) or
 * "bc_jit_match_count<NW,NWW>" (the one specialised to this plan's scheme); "" before the first submit. */
const char *bc_engine_kernel_name(bc_engine *e);
/* How many times the engine has folded a count log into its counters since it was created (log-mode counting: dense
 * plans with a bit map, BC_COUNT_LOG); 0 when every submit counted with per-read atomics.  One fold per chunk of at
 * most BC_COUNT_LOG_CHUNK reads of a log-mode submit.  Read-only: does not wait for the device. */
int bc_engine_count_log_folds(const bc_engine *e, uint64_t *n);
/* Reads submitted to the lane-per-read kernel under a wide-key plan since the engine was created.  A wide-key plan (a
 * raw capture or a random barcode above 27 bases, or captures that overflow the 64-bit key together) runs on that
 * kernel when BC_WIDE_LANE=1 was set at bc_engine_create and the plan is within the kernel's widths (groups, known
 * barcodes and random barcode of at most 32 bases, a format of at most 320, at most 31 constant errors); batches
 * above 320 bases go to the wave-per-read kernel as ever and are not counted here.  0 with the switch off (the
 * default) or an ineligible plan.  The counts are the same either way.  Read-only: does not wait for the device. */
int bc_engine_wide_lane_reads(const bc_engine *e, uint64_t *n);
/* Shader clock right now (MHz), measured by a 0.3 ms probe kernel on the engine's stream against the
 * 100 MHz reference counter.  Call it straight after the work of interest: the clock sags under power
 * and thermal limits, and the match kernel's time follows it. */
int bc_engine_sclk_mhz(bc_engine *e, double *mhz);

/* Box diagnostic for benchmarks: issues ~n_atomics no-return atomic adds of +1 at random entries of a u32 table, then
 * the same adds of -1 at the same entries (the table ends as it was, but is transiently different: the caller must be
 * idle on it), and reports the sustained rate of the first pass -- what the memory system of THIS device gives the match
 * kernel's counting alone (it differs between boxes by tens of percent).  Runs on the NULL stream and waits for the
 * device; it is not ordered against work on a non-blocking stream, so sync the engine first. */
int bc_probe_atomic_rate(int device_id, void *d_table_u32, uint64_t entries, uint64_t n_atomics, double *atomics_per_s);

/* Scheme-specialised kernels.  Next to the generic kernel (any plan, plan read from memory) an engine
 * can run one compiled for its plan's scheme (offsets, shift programs, thresholds and set sizes as
 * immediates; ~15-25 % faster).  The code object is looked up by content hash in jit_cache/ next to
 * the library and in $BC_JIT_CACHE: a hit is used from the first submit on.  On a miss the engine
 * keeps counting with the generic kernel and, once 2^20 reads have been submitted, compiles the
 * specialised one on a worker thread (ROCm's hipcc as a child process, else hiprtc in-process), stores
 * it in the cache and switches over at the next submit after it is ready.  Results are identical
 * either way.  If no compiler is available the engine says so once on stderr.
 * Environment: BC_JIT=0 (never) | 1 (default) | force (compile synchronously at the first submit) |
 * cached (cache hits only).
 * A specialised kernel is also specific to the batch shape: the stride and, for fixed-length batches, the read
 * length are compile-time constants of it (one kernel per shape; a FASTQ file has one or a few).
 * bc_plan_precompile builds the kernel of one shape ahead of time without touching a GPU: stride / read_len as
 * they will be passed to bc_engine_submit_* (reads of up to 256 bases; longer ones stay on the generic kernel),
 * with_lens = per-read lengths will be passed (read_len is then ignored), cache_dir NULL = next to the library. */
int bc_plan_precompile(const bc_plan *p, uint32_t stride, uint32_t read_len, int with_lens, const char *cache_dir);

/* fix_error (parse.rs:553-593) on the device: nearest unique candidate under Hamming distance
 * with 'N' wildcards, common-prefix compare.  Returns the candidate index, -1 for None,
 * or < -1 on error (BC_ERR_* - 1). */
int64_t bc_fix_error(const char *mismatch_seq, const char *const *possible_seqs, uint64_t n, uint16_t mismatches,
                     int device_id);

/* ---- FASTQ ingest (replaces input::read_fastq, input.rs:24-149) --------------- */

/* (A *.bam file is accepted as well: see "unaligned BAM" below.)
 * Reads a whole *.fastq / *.fastq.gz file, frames it into 4-line records exactly as
 * FastqLineReader does (input.rs:115-148), and submits the sequence / quality lines to the engine in
 * batches through bc_engine_submit_host (pinned buffers, copies overlapped with the kernel).
 * *total_reads receives the reference's "Total sequences" value, including its quirks: a trailing
 * partial record is counted but never processed, and a .gz input counts one read more
 * (input.rs:69-73, 128-130).  progress (may be NULL) is called with the running total about every
 * million reads.  Errors the reference raises come back as BC_ERR_INVALID with its message:
 * wrong extension (input.rs:36-39), unreadable file, first record not FASTQ (parse.rs:377-394). */
typedef void (*bc_progress_fn)(uint64_t total_reads, void *user);
int bc_fastq_count(bc_engine *e, const char *fastq_path, uint64_t *total_reads, bc_progress_fn progress, void *user);
/* One shard of n_shards (one per GPU of a job): the records that start inside this shard's share of the file's bytes.
 * Shard boundaries are moved to the next record start ('@' line whose second-next line begins with '+'), so the shards
 * tile the file's records exactly and their totals add up to bc_fastq_count's -- for a file whose lines come in fours;
 * one that does not is refused (BC_ERR_INVALID: the reference frames from the file's first line, a shard cannot).  The
 * first-record check is the first shard's, the trailing partial record the last shard's.  A BGZF file (see below) is
 * sharded like a plain one, by its INFLATED bytes: every shard reads and inflates only the blocks that cover its
 * records, and the end-of-stream quirks of a .gz input are the last shard's.  Any other .gz stream cannot be entered in
 * the middle: shard 0 reads all of it, the others nothing. */
int bc_fastq_count_shard(bc_engine *e, const char *fastq_path, uint32_t shard, uint32_t n_shards, uint64_t *total_reads,
                         bc_progress_fn progress, void *user);
/* where a shard that nominally begins at byte `offset` of a plain FASTQ file really begins: the first record start at
 * or after it (the file's size when there is none).  Host logic only: no engine, no GPU. */
int bc_fastq_record_start(const char *fastq_path, uint64_t offset, uint64_t *start);

/* ---- BGZF: blocked gzip, inflated on the device ------------------------------------------------- */

/* A *.fastq.gz file that is BGZF through and through (what bgzip and the htslib tools write: a chain of gzip members
 * of at most 64 KiB of text each, every header giving its member's length) is not read through zlib: the compressed
 * bytes go to the device, one wavefront inflates one block (all of RFC 1951, CRC32 and ISIZE checked there), and the
 * framing kernels go on from the inflated text.  Every other .gz file keeps the single zlib stream.  Counts are the same
 * either way.  Environment: BC_GZ_DEVICE=1 (default) | 0 (every .gz through zlib); BC_INGEST_VERBOSE=1: one line on
 * stderr per bc_fastq_count* call (path taken, shard, blocks inflated, records counted). */

/* Walks the member headers of a file (host only, no GPU).  BC_OK: the file is BGZF -- every member is deflate with
 * FEXTRA and a 'BC' subfield of length 2, the chain offset += BSIZE + 1 tiles the file to its last byte, every ISIZE is
 * at most 65536 (empty members, such as the 28-byte EOF marker, are ordinary blocks; the marker may be missing).
 * BC_ERR_UNSUPPORTED: it is not, and bc_last_error says where the chain broke.  BC_ERR_INVALID: unreadable. */
int bc_bgzf_scan(const char *path, uint64_t *n_blocks, uint64_t *inflated_bytes);
/* bc_fastq_record_start for a BGZF file: `inflated_offset` and *start count inflated bytes.  Inflates only the blocks
 * around the offset, with zlib on the host.  BC_ERR_UNSUPPORTED when the file is not BGZF. */
int bc_fastq_gz_record_start(const char *path, uint64_t inflated_offset, uint64_t *start);

/* one block of an inflate table */
typedef struct bc_bgzf_block {
  uint64_t src_off;  /* where the block's deflate stream (the member without header and trailer) starts in d_src */
  uint64_t dst_off;  /* where its text goes in d_dst */
  uint32_t src_len;  /* bytes of the deflate stream */
  uint32_t isize;    /* ISIZE of the trailer: bytes of text */
  uint32_t crc32;    /* CRC32 of the trailer */
} bc_bgzf_block;

/* per-block results of bc_bgzf_inflate_device */
#define BC_INFLATE_OK 0
#define BC_INFLATE_BAD_BLOCK_TYPE 1   /* BTYPE 3, or a stored block whose LEN / NLEN disagree */
#define BC_INFLATE_BAD_CODE_LENGTHS 2
#define BC_INFLATE_BAD_SYMBOL 3       /* invalid symbol, or a distance that reaches before the block's own text */
#define BC_INFLATE_INPUT_OVERRUN 4
#define BC_INFLATE_OUTPUT_OVERRUN 5
#define BC_INFLATE_ISIZE_MISMATCH 6
#define BC_INFLATE_CRC_MISMATCH 7

/* Inflates n_blocks BGZF blocks that lie in device memory: d_src[0, src_bytes) holds the compressed bytes, `blocks`
 * (host memory) says where each block's deflate stream is and where its text goes in d_dst[0, dst_bytes).  status
 * (host memory, n_blocks words) receives BC_INFLATE_OK or what was wrong with the block; a bad block never reads
 * outside its own stream nor writes outside its own [dst_off, dst_off + isize).  Runs on hip_stream (NULL: the default
 * stream) and waits for it.  BC_OK even when blocks are bad (the status says so); BC_ERR_INVALID only for a table that
 * contradicts src_bytes / dst_bytes (or a block above 65536 bytes either way). */
int bc_bgzf_inflate_device(int device_id, void *hip_stream, const void *d_src, uint64_t src_bytes,
                           const bc_bgzf_block *blocks, uint64_t n_blocks, void *d_dst, uint64_t dst_bytes,
                           uint32_t *status);
/* BGZF blocks inflated on the device for this engine since it was created (by bc_fastq_count*).  Read-only: does not
 * wait for the device. */
int bc_engine_gz_blocks_inflated(const bc_engine *e, uint64_t *n);

/* ---- ordinary gzip: one long deflate stream, inflated on the device in segments ------------------ */

/* What gzip, pigz and a sequencer's converter write is one deflate stream per member, with no index: there is no way
 * into its middle but to search for block headers.  A SPAN of such a stream -- compressed bytes, a start bit that is a
 * known block boundary, the 32 KiB of text before it -- is inflated in five stages: a wavefront per partition of
 * part_bytes compressed bytes finds the first offset at which a dynamic block header passes the decoder's checks; a
 * wavefront per candidate decodes without storing until it lands on a later candidate; the host follows those links
 * from the start bit (segments on the path are real, every other candidate is false); a wavefront per segment decodes
 * again with markers for the bytes before its start; the markers are resolved segment by segment, then all at once.
 * Opt-in for bc_fastq_count*: BC_GZ_DEVICE=all sends a .gz file that is not BGZF this way (BC_GZ_SPAN_BYTES and
 * BC_GZ_PART_BYTES size the spans and partitions); counts are the same either way. */

#define BC_GUNZIP_OK 0
#define BC_GUNZIP_OUTPUT_FULL 1  /* the text does not fit: text_bytes / end_bit give the last block boundary that does */
#define BC_GUNZIP_BAD_STREAM 2   /* not a deflate stream: `detail` is a BC_INFLATE_* word */

typedef struct bc_gunzip_result {
  uint32_t status;      /* BC_GUNZIP_* */
  uint32_t detail;
  uint64_t text_bytes;  /* bytes of text written to d_text (BC_GUNZIP_OUTPUT_FULL: that would fit; none are written) */
  uint64_t end_bit;     /* the block boundary the text ends at, in bits of d_src; == start_bit: no whole block */
  uint32_t member_end;  /* 1: that boundary is the end of the member's last block (the trailer follows, byte aligned) */
  uint32_t segments;    /* verified segments */
  uint32_t rejected;    /* candidates the chain walked past without landing on them (false block headers) */
  uint32_t crc32;       /* CRC-32 of the text written */
} bc_gunzip_result;

/* Inflates the whole blocks of d_src[0, src_bytes) (device memory, under 256 MiB) from bit start_bit on into
 * d_text[0, text_capacity).  d_history: the 32768 bytes of text before start_bit (device memory), or NULL at a member's
 * start.  part_bytes: a multiple of 8, at least 64; 0 = 32768.  The span ends at the member's end, at the last block
 * boundary its bytes hold, or (BC_GUNZIP_OUTPUT_FULL) where the text stops fitting: then nothing is written and the
 * caller comes back with the span cut at end_bit.  Runs on hip_stream and waits for it.  BC_OK whatever the stream is
 * like (the result says); a damaged stream never reads or writes outside the buffers. */
int bc_gunzip_span_device(int device_id, void *hip_stream, const void *d_src, uint64_t src_bytes, uint64_t start_bit,
                          const void *d_history, void *d_text, uint64_t text_capacity, uint32_t part_bytes,
                          bc_gunzip_result *result);
/* segments inflated that way for this engine since it was created (by bc_fastq_count*) */
int bc_engine_gz_segments_inflated(const bc_engine *e, uint64_t *n);

/* ---- unaligned BAM: BGZF blocks inflated and BAM records framed on the device -------------------- */

/* bc_fastq_count* accept a *.bam file and count it as they would count the plain FASTQ file that `samtools fastq` with
 * default options writes for it: the packed sequence through "=ACMGRSVTWYHKDBN", each quality byte q as
 * min(q, 93) + 33 (a record without qualities, first byte 0xFF: all '"'), an empty sequence and quality line for
 * l_seq == 0; a record flagged 0x10 is handed on reverse-complemented with its qualities reversed; records flagged
 * 0x100 or 0x800 (secondary, supplementary) are skipped and not counted.  Every other record is one read, and
 * *total_reads is their number: none of the .gz quirks apply.  Names, CIGAR, aux fields and the header are skipped.
 * The file always goes the device way (BC_GZ_DEVICE is about .gz names; BC_INGEST_VERBOSE names the path
 * bam-device): the BGZF blocks are inflated as above, and the records -- binary, length-prefixed, so that a record's
 * start is known only from the record before it -- are found in parallel: every offset that could start a record by
 * its fixed 36 bytes is a candidate, every candidate knows its successor, and jump pointers mark the one chain that
 * starts at the first unframed byte.  BC_ERR_INVALID: not BGZF, bad magic, a header that runs past the file, a damaged
 * block, a record chain that breaks (what follows a record is no record header, or bytes are left after the last whole
 * record).  BC_ERR_UNSUPPORTED: l_seq above 65535, a record longer than 4 MiB.
 * Several shards: shard 0 reads the whole file, the others nothing, as with an ordinary gzip stream.  Record-aligned
 * BAM shards are not built. */

/* The header of a BAM file (host only, no GPU): *n_ref the number of reference sequences in its dictionary,
 * *first_record_offset where, in the inflated stream, the first record starts, *inflated_bytes the stream's length.
 * BC_ERR_INVALID: unreadable, not BGZF, bad magic, or a header that runs past the end of the file. */
int bc_bam_scan(const char *path, uint32_t *n_ref, uint64_t *first_record_offset, uint64_t *inflated_bytes);

#define BC_BAM_OK 0
#define BC_BAM_BROKEN_CHAIN 1  /* what follows a whole record of the chain (or lies at `start`) is no record header */
#define BC_BAM_CAPACITY 2      /* more candidates than `capacity`: nothing is framed */
#define BC_BAM_TOO_LONG 3      /* as BROKEN_CHAIN, but the header there would do were its record not above 4 MiB */

typedef struct bc_bam_frame_result {
  uint32_t status;        /* BC_BAM_* */
  uint32_t reserved;
  uint64_t n_records;     /* whole records of the chain from `start`, written to the three arrays in order */
  uint64_t n_candidates;  /* offsets in [start, len - 36] that pass the header filter */
  uint64_t end_pos;       /* just past the chain's last whole record (`start` when there is none) */
} bc_bam_frame_result;

/* The record framing on its own: d_text[0, len) (device memory, 16-byte aligned, under 2 GiB) holds BAM records, the
 * first of them at `start`; n_ref is the dictionary's size.  d_rec_at / d_rec_len / d_rec_flag (device memory,
 * `capacity` words each) receive every whole record's offset, l_seq and flag -- secondary and supplementary ones too.
 * The chain ends where fewer than 36 bytes follow a record or a record runs past len.  Never reads outside the text,
 * whatever it holds.  Runs on hip_stream (NULL: the default stream) and waits for it.  BC_OK whatever the text is like
 * (the result says). */
int bc_bam_frame_device(int device_id, void *hip_stream, const void *d_text, uint64_t len, uint64_t start, uint32_t n_ref,
                        uint32_t *d_rec_at, uint32_t *d_rec_len, uint32_t *d_rec_flag, uint64_t capacity,
                        bc_bam_frame_result *result);

/* ---- reverse complement of a batch on the device ------------------------------------------------- */

/* The kernel behind BC_STRAND_REVERSE / _BOTH on its own: output read j = rc(read d_index[j]) of the batch (d_index: u32,
 * device memory, may repeat, skip and reorder; NULL = reads 0 .. n_out in order), rc as bc_plan_set_strand defines it.
 * The batch has the layout bc_engine_submit_device[_q] takes (d_qual, d_lens, d_qlens may be NULL; without d_lens every
 * read is read_len long; without d_qlens a quality line is as long as its sequence line), and the output has the same
 * form at the same stride: d_seq_out (and d_qual_out, d_lens_out, d_qlens_out for every input given) hold n_out reads.
 * Bytes [len, stride) of an output line are padding as the BAM path pads: 'N' in a sequence line, '!' in a quality line;
 * nothing outside the n_out * stride bytes is written.  Sequence and quality buffers 16-byte aligned; not in place.
 * Every d_index[j] must name a read of the batch: the call cannot check that.  Only enqueues on hip_stream (NULL: the
 * default stream) and does not wait. */
int bc_strand_orient_device(int device_id, void *hip_stream, const void *d_seq, const void *d_qual, const void *d_lens,
                            const void *d_qlens, uint32_t stride, uint32_t read_len, const uint32_t *d_index, uint64_t n_out,
                            void *d_seq_out, void *d_qual_out, void *d_lens_out, void *d_qlens_out);

/* ---- synthetic workloads (bench + full-size parity) -------------------------------------- */

typedef struct bc_synth_params {
  uint64_t seed;
  uint32_t read_len;     /* R; construct start uniform in [0, R-L-1] */
  uint32_t p_sub;        /* per-base substitution probability * 2^32 */
  uint32_t p_n;          /* per-base 'N' probability * 2^32 */
  uint32_t p_lowq;       /* probability * 2^32 that one barcode of a read gets low qualities */
  uint8_t phred_lo, phred_hi;   /* default Phred range, inclusive */
  uint8_t lowq_lo, lowq_hi;     /* low-quality Phred range, inclusive */
  uint64_t n_molecules;  /* 0: every read is its own molecule; else reads are draws from this many
                            molecules (PCR duplicates) */
  uint32_t zipf;         /* 1: counted-barcode indices follow a Zipf-like law with exponent 1 (P(rank k) ~ 1/k; the
                            hot-spot variant of SURVEY.md 8(d)) instead of the uniform one */
  uint32_t reserved;
  uint64_t geo_total;    /* > 0: PCR copies per molecule geometric with mean 2, scattered over this many reads (the
                            job's total) by a fixed permutation; n_molecules is then ignored */
} bc_synth_params;

bc_synth *bc_synth_create(const bc_plan *p, const bc_synth_params *params);
void bc_synth_destroy(bc_synth *s);
int bc_synth_generate_host(bc_synth *s, uint64_t first_read, uint64_t n_reads, void *seq, void *qual, uint32_t stride);
int bc_synth_generate_device(bc_synth *s, int device_id, void *hip_stream, uint64_t first_read, uint64_t n_reads,
                             void *d_seq, void *d_qual, uint32_t stride);
/* deterministic reference set: n distinct k-mers, pairwise Hamming distance >= min_dist;
 * out receives n*(k+1) bytes (NUL-terminated strings) */
int bc_synth_make_set(uint64_t seed, uint32_t n, uint32_t k, uint32_t min_dist, char *out);

#ifdef __cplusplus
}
#endif
#endif
