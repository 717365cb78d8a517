// bc_cli_output.hpp -- what `barcode-count` does once the reads are counted: the run's state, the display blocks, the
// rows rebuilt from the engine, the writers of the counts files and the stats file (bc_cli_output.cpp).
#pragma once

#include <stdint.h>
#include <time.h>

#include <map>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../../include/barcode_count_hip.h"
#include "bc_cli_writers.hpp"

struct Args {  // arguments.rs:6-20; filled by parse_args (barcode_count_main.cpp)
  std::string fastq, format, output_dir = "./", prefix;
  bool has_samples = false, has_counted = false;
  std::string sample_barcodes, counted_barcodes;
  int threads = 0;
  bool merge_output = false, enrich = false;
  int barcodes_errors = -1, sample_errors = -1, constant_errors = -1;
  float min_quality = 0.0f;
  int device = 0;
  int strand = BC_STRAND_FORWARD;  // --strand forward | reverse | both (bc_plan_set_strand)
  // several GPUs
  int gpus = 1;
  std::vector<int> devices;        // --devices a,b,..: the HIP device of each rank (default 0 .. gpus-1)
  std::string comm = "rccl";       // --comm rccl | host
  int rank = -1, world = 1;        // (set by the launcher for its rank processes)
  std::string comm_dir;
};

struct Run {
  Args args;
  bc_plan* plan = nullptr;
  bc_engine* engine = nullptr;
  uint32_t barcode_num = 0;
  uint64_t reverse_matched = 0;  // --strand reverse | both: the job's reads that matched as their reverse complement
  std::vector<std::pair<std::string, std::string>> samples;               // (sequence, id) in index order
  std::vector<std::vector<std::pair<std::string, std::string>>> counted;  // per barcode position
  // Results (info.rs:661-665) rebuilt from the engine's rows: sample key -> (tuple of sequences -> count)
  std::vector<std::string> sample_keys;
  struct Row {
    std::string code;     // "b1,b2,.." as sequences (the key Results holds)
    std::string written;  // the same converted to IDs when a counted-barcode file was given (output.rs:282-287)
    uint64_t count;
  };
  std::unordered_map<std::string, std::vector<Row>> results;
  std::unordered_map<std::string, std::unordered_map<std::string, uint64_t>> results_map;  // for the merged file
  std::vector<std::unordered_map<std::string, std::string>> counted_map;                  // sequence -> ID
  // WriteFiles state (output.rs:33-46)
  std::unordered_map<std::string, std::map<std::string, uint64_t>> single_hash, double_hash;
  std::unordered_set<std::string> compounds_written;
  std::vector<std::string> output_files;
  std::vector<uint64_t> output_counts;
  uint64_t merged_count = 0;
  std::string merge_text;
  // Which writer the full-counts files and the Single / Double files get (choose_writers).  Any counts writer but Rows
  // leaves no row on the host; the DenseText and RawText enrichment writers leave single_hash / double_hash empty.
  Writers writers;
  std::unordered_map<std::string, uint32_t> sample_index;  // sample key -> the engine's sample index (device writers)
};

[[noreturn]] void die(const char* fmt, ...);
std::string commas(uint64_t v);  // num-format Locale::en
double now_ms();
std::string elapsed_text(double ms_total);

std::string format_display(const Run& r);
std::string max_errors_display(const Run& r);
std::string errors_display(const uint64_t counters[BC_NCOUNTERS]);
// "" for --strand forward (stdout and the stats file stay byte for byte what they were), else one further line
std::string strand_display(const Run& r);

// Results as the writers see it: samples, counted, sample_keys, counted_map and sample_index from the plan
void describe_results(Run& r);
// the plan, the engine and the environment's four switches as the facts choose_writers decides on
WriterFacts gather_facts(const Run& r);
// CountsWriter::Rows: the engine's n_rows rows as host strings (results, results_map; may append to sample_keys)
void rebuild_rows(Run& r, uint64_t n_rows);
// EnrichWriter::Marginals: single_hash / double_hash from the device's marginal sums; false: the device has no room
// for them (or no enrichment for the plan), and the rows have to build the maps
bool fill_enrichment(Run& r);
// BC_WRITERS_VERBOSE / BC_ENRICH_VERBOSE: which writers the run got, on stderr
void report_writers(const Run& r);
// every counts file of the run: the full family, then with -e the Single and Double families
void write_counts_files(Run& r);
// BC_ENRICH_VERBOSE: how many keys the host's Single / Double maps hold after the files are written
void report_enrichment_maps(const Run& r);
void write_stats_file(const Run& r, time_t start, double start_ms, const uint64_t counters[BC_NCOUNTERS], uint64_t total_reads);
