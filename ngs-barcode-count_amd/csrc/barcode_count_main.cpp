// barcode_count_main.cpp -- the `barcode-count` command line, on top of the C ABI only.
//
// Drop-in for the reference binary: same flags and defaults
// (arguments.rs:27-124), same stdout blocks (main.rs:19-25, 65, 124-164; info.rs:141-172, 313-335,
// 618-659), same output files, headers and stats file (output.rs:74-576; info.rs:811-904).  The
// reader thread and the worker pool of main.rs:69-121 are replaced by bc_fastq_count + the gfx950
// engine.  Row order inside the CSVs is unspecified in the reference (HashMap iteration); here rows
// come out in the engine's index order.  `--threads` is accepted and ignored (no CPU workers exist).
//
// `--gpus N` (no counterpart in the reference, which is one process): the process started by the user never touches
// a GPU; it starts N rank processes of this same program, one per GPU, and passes rank 0's output through.  Every
// rank counts its share of the FASTQ file's records (bc_fastq_count_shard) and the job ends with the one exchange of
// bc_engine_finish_all -- RCCL over xGMI between the GPUs (rank 0's unique id travels through a file in a private
// temporary directory), or, with `--comm host`, message files in that directory (several ranks on one GPU).
//
// What happens once the reads are counted -- which writer each file gets, the rows, the files -- is bc_cli_output.cpp.
#include <errno.h>
#include <fcntl.h>
#include <spawn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <dirent.h>
#include <signal.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bc_cli_output.hpp"

extern char** environ;

namespace {

void usage() {
  printf(
      "NGS-Barcode-Count (MI355X engine)\nCounts barcodes located in sequencing data\n\nUSAGE:\n"
      "    barcode-count [FLAGS] [OPTIONS] --fastq <fastq> --sequence-format <format_file>\n\nFLAGS:\n"
      "    -e, --enrich          Create output files of enrichment for single and double synthons/barcodes\n"
      "    -m, --merge-output    Merge sample output counts into a single file.  Not necessary when there is only one sample\n"
      "    -h, --help            Prints help information\n\nOPTIONS:\n"
      "    -c, --counted-barcodes <barcode_file>      Counted barcodes file\n"
      "    -o, --output-dir <dir>                     Directory to output the counts to [default: ./]\n"
      "    -f, --fastq <fastq>                        FastQ file\n"
      "    -q, --sequence-format <format_file>        Sequence format file\n"
      "        --max-errors-counted-barcode <n>       Maximimum number of sequence errors allowed within each counted barcode. Defaults to 20%% of the total.\n"
      "        --max-errors-constant <n>              Maximimum number of sequence errors allowed within constant region. Defaults to 20%% of the total.\n"
      "        --max-errors-sample <n>                Maximimum number of sequence errors allowed within sample barcode. Defaults to 20%% of the total.\n"
      "        --min-quality <min>                    Minimum average read quality score per barcode [default: 0]\n"
      "    -p, --prefix <prefix>                      File prefix name.  THe output will end with '_<sample_name>_counts.csv'\n"
      "    -s, --sample-barcodes <sample_file>        Sample barcodes file\n"
      "    -t, --threads <threads>                    Number of threads (ignored: the GPU engine has no CPU workers)\n"
      "        --strand <forward|reverse|both>        Which orientation of a read is counted: as it stands, as its reverse complement,\n"
      "                                               or as it stands first and reversed when the constant region mismatches (unaligned BAM\n"
      "                                               from a basecaller, non-directional preps, an R2 file).  reverse and both print one\n"
      "                                               further line, 'Reverse strand matches:' [default: forward]\n"
      "        --device <id>                          HIP device to run on [default: 0]\n"
      "        --gpus <n>                             Run on n GPUs: one process per GPU, reads sharded, one exchange at the end [default: 1]\n"
      "        --devices <a,b,..>                     The HIP device of each of the n ranks [default: 0,1,..]\n"
      "        --comm <rccl|host>                     How the ranks exchange their results: RCCL over xGMI, or files in a temporary directory [default: rccl]\n");
}

int parse_u16(const char* what, const char* v) {
  char* end;
  const long x = strtol(v, &end, 10);
  if (*v == 0 || *end != 0 || x < 0 || x > 65535) die("Unable to convert %s to an integer", what);
  return (int)x;
}

Args parse_args(int argc, char** argv) {
  Args a;
  {
    char today[32];
    time_t t = time(nullptr);
    strftime(today, sizeof today, "%Y-%m-%d", localtime(&t));  // arguments.rs:25
    a.prefix = today;
  }
  bool have_fastq = false, have_format = false;
  for (int i = 1; i < argc; ++i) {
    std::string k = argv[i];
    std::string v;
    auto eq = k.find('=');
    bool inline_val = false;
    if (k.rfind("--", 0) == 0 && eq != std::string::npos) {
      v = k.substr(eq + 1);
      k = k.substr(0, eq);
      inline_val = true;
    }
    auto val = [&]() -> std::string {
      if (inline_val) return v;
      if (i + 1 >= argc) die("The argument '%s' requires a value", k.c_str());
      return argv[++i];
    };
    if (k == "-h" || k == "--help") {
      usage();
      exit(0);
    } else if (k == "-f" || k == "--fastq") {
      a.fastq = val();
      have_fastq = true;
    } else if (k == "-q" || k == "--sequence-format") {
      a.format = val();
      have_format = true;
    } else if (k == "-s" || k == "--sample-barcodes") {
      a.sample_barcodes = val();
      a.has_samples = true;
    } else if (k == "-c" || k == "--counted-barcodes") {
      a.counted_barcodes = val();
      a.has_counted = true;
    } else if (k == "-t" || k == "--threads") {
      a.threads = parse_u16("threads", val().c_str());
    } else if (k == "-o" || k == "--output-dir") {
      a.output_dir = val();
    } else if (k == "-p" || k == "--prefix") {
      a.prefix = val();
    } else if (k == "-m" || k == "--merge-output") {
      a.merge_output = true;
    } else if (k == "-e" || k == "--enrich") {
      a.enrich = true;
    } else if (k == "--max-errors-counted-barcode") {
      a.barcodes_errors = parse_u16("maximum barcode errors", val().c_str());
    } else if (k == "--max-errors-sample") {
      a.sample_errors = parse_u16("maximum sample errors", val().c_str());
    } else if (k == "--max-errors-constant") {
      a.constant_errors = parse_u16("maximum constant errors", val().c_str());
    } else if (k == "--min-quality") {
      const std::string s = val();
      char* end;
      a.min_quality = strtof(s.c_str(), &end);
      if (s.empty() || *end != 0) die("Unable to convert min score to a float");
    } else if (k == "--strand") {
      const std::string s = val();
      if (s != "forward" && s != "reverse" && s != "both") die("--strand must be forward, reverse or both");
      a.strand = s == "forward" ? BC_STRAND_FORWARD : (s == "reverse" ? BC_STRAND_REVERSE : BC_STRAND_BOTH);
    } else if (k == "--device") {
      a.device = parse_u16("device", val().c_str());
    } else if (k == "--gpus") {
      a.gpus = parse_u16("gpus", val().c_str());
      if (a.gpus < 1 || a.gpus > 64) die("--gpus must be between 1 and 64");
    } else if (k == "--devices") {
      const std::string list = val();
      size_t at = 0;
      while (at <= list.size()) {
        const size_t c = list.find(',', at);
        a.devices.push_back(parse_u16("device", list.substr(at, c == std::string::npos ? std::string::npos : c - at).c_str()));
        if (c == std::string::npos) break;
        at = c + 1;
      }
    } else if (k == "--comm") {
      a.comm = val();
      if (a.comm != "rccl" && a.comm != "host") die("--comm must be rccl or host");
    } else if (k == "--bc-rank") {  // (the three below are how the launcher tells a rank process who it is)
      a.rank = parse_u16("rank", val().c_str());
    } else if (k == "--bc-world") {
      a.world = parse_u16("world", val().c_str());
    } else if (k == "--bc-comm-dir") {
      a.comm_dir = val();
    } else {
      die("Found argument '%s' which wasn't expected, or isn't valid in this context", k.c_str());
    }
  }
  if (!have_fastq || !have_format) die("The following required arguments were not provided: --fastq <fastq> --sequence-format <format_file>");
  if (!a.devices.empty() && (int)a.devices.size() != a.gpus) die("--devices names %zu devices for --gpus %d", a.devices.size(), a.gpus);
  return a;
}

std::string read_file(const std::string& path, const char* ctx) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) die("%s %s", ctx, path.c_str());
  std::string s;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
  fclose(f);
  return s;
}

void progress(uint64_t total, void*) {  // input.rs:151-159 (printed every 10,000 reads there)
  printf("Total sequences:             %s\r", commas(total).c_str());
  fflush(stdout);
}

// --gpus N: starts the N rank processes and waits for them.  Nothing here touches a GPU (no HIP call, and the engine
// library is not even asked for a device), and nothing is exec'ed by a process that has: the ranks are fresh children.
int launch_ranks(const Args& a, int argc, char** argv) {
  const char* base = getenv("TMPDIR");
  std::string dir = std::string(access("/dev/shm", W_OK) == 0 ? "/dev/shm" : (base && *base ? base : "/tmp")) + "/barcode-count-XXXXXX";
  if (!mkdtemp(&dir[0])) die("cannot create a temporary directory for the ranks: %s", strerror(errno));
  char self[4096];
  const ssize_t sl = readlink("/proc/self/exe", self, sizeof self - 1);
  if (sl <= 0) die("cannot find this program's own path");
  self[sl] = 0;
  std::vector<pid_t> pids;
  for (int r = 0; r < a.gpus; ++r) {
    std::vector<std::string> args(argv, argv + argc);
    args[0] = self;
    const int dev = a.devices.empty() ? r : a.devices[(size_t)r];
    for (const char* extra : {"--bc-rank", "", "--bc-world", "", "--bc-comm-dir", "", "--device", ""}) args.push_back(extra);
    args[args.size() - 7] = std::to_string(r);
    args[args.size() - 5] = std::to_string(a.gpus);
    args[args.size() - 3] = dir;
    args[args.size() - 1] = std::to_string(dev);
    std::vector<char*> av;
    for (auto& s : args) av.push_back(&s[0]);
    av.push_back(nullptr);
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    if (r != 0) posix_spawn_file_actions_addopen(&fa, 1, "/dev/null", O_WRONLY, 0);  // one voice on stdout: rank 0's
    pid_t pid = 0;
    const int rc = posix_spawn(&pid, self, &fa, nullptr, av.data(), environ);
    posix_spawn_file_actions_destroy(&fa);
    if (rc != 0) {
      for (pid_t p : pids) kill(p, SIGTERM);
      die("cannot start rank %d: %s", r, strerror(rc));
    }
    pids.push_back(pid);
  }
  int worst = 0;
  for (size_t r = 0; r < pids.size(); ++r) {
    int status = 0;
    while (waitpid(pids[r], &status, 0) < 0 && errno == EINTR) {
    }
    const int code = WIFEXITED(status) ? WEXITSTATUS(status) : 128 + (WIFSIGNALED(status) ? WTERMSIG(status) : 0);
    if (code != 0) {
      fprintf(stderr, "Error: rank %zu ended with status %d\n", r, code);
      if (worst == 0)  // its peers may be waiting for it in the exchange: do not leave them waiting
        for (size_t q = r + 1; q < pids.size(); ++q) kill(pids[q], SIGTERM);
    }
    worst = std::max(worst, code);
  }
  // whatever is left of the ranks' messages, and the directory
  const std::string cmd_dir = dir;
  if (DIR* d = opendir(cmd_dir.c_str())) {
    while (struct dirent* e = readdir(d))
      if (e->d_name[0] != '.') unlink((cmd_dir + "/" + e->d_name).c_str());
    closedir(d);
  }
  rmdir(cmd_dir.c_str());
  return worst;
}

// a rank's communicator: RCCL (the unique id goes from rank 0 to the others through a file) or message files
bc_comm* make_comm(const Args& a) {
  if (a.comm == "host") {
    bc_comm* c = bc_comm_create_host(a.comm_dir.c_str(), a.rank, a.world);
    if (!c) die("%s", bc_last_error());
    return c;
  }
  unsigned char id[BC_COMM_ID_BYTES];
  const std::string path = a.comm_dir + "/rccl_id";
  if (a.rank == 0) {
    if (bc_comm_unique_id(id)) die("%s", bc_last_error());
    const std::string tmp = path + ".part";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f || fwrite(id, 1, sizeof id, f) != sizeof id || fclose(f) != 0 || rename(tmp.c_str(), path.c_str()) != 0)
      die("cannot write %s", path.c_str());
  } else {
    const double t0 = now_ms();
    for (;;) {
      FILE* f = fopen(path.c_str(), "rb");
      if (f) {
        const size_t n = fread(id, 1, sizeof id, f);
        fclose(f);
        if (n == sizeof id) break;
      }
      if (now_ms() - t0 > 300e3) die("rank 0 did not publish the communicator id");
      usleep(2000);
    }
  }
  bc_comm* c = bc_comm_create(id, a.rank, a.world, a.device);
  if (!c) die("%s", bc_last_error());
  return c;
}


// the plan from the scheme and the two barcode files, the two info blocks on stdout, the engine
void set_up_plan(Run& r) {
  const std::string scheme = read_file(r.args.format, "Failed to open");
  r.plan = bc_plan_create(scheme.data(), scheme.size());
  if (!r.plan) die("%s", bc_last_error());
  r.barcode_num = bc_plan_barcode_num(r.plan);
  printf("%s\n\n", format_display(r).c_str());  // main.rs:19

  if (r.args.enrich && r.barcode_num < 2) {  // main.rs:22-25
    fprintf(stderr, "Fewer than 2 counted barcodes.  Too few for barcode enrichment.  Argument flag is ignored\n");
    r.args.enrich = false;
  }
  if (r.args.has_samples) {
    const std::string t = read_file(r.args.sample_barcodes, "Failed to open");
    if (bc_plan_load_sample_csv(r.plan, t.data(), t.size())) die("%s", bc_last_error());
  }
  if (r.args.has_counted) {
    const std::string t = read_file(r.args.counted_barcodes, "Failed to read");
    if (bc_plan_load_counted_csv(r.plan, t.data(), t.size())) die("%s", bc_last_error());
  }
  bc_plan_set_max_errors(r.plan, r.args.sample_errors, r.args.barcodes_errors, r.args.constant_errors);
  bc_plan_set_min_quality(r.plan, r.args.min_quality);
  if (bc_plan_set_strand(r.plan, r.args.strand)) die("%s", bc_last_error());
  printf("%s\n\n", max_errors_display(r).c_str());  // main.rs:65

  r.engine = bc_engine_create(r.plan, r.args.device, nullptr, nullptr);
  if (!r.engine) die("%s", bc_last_error());
}

// Counts the file's reads: the whole file in one process, or this rank's share of the records and then the job's one
// exchange, after which the root holds the job's counters and its n_rows rows and goes on to write the job's files.
void count_reads(Run& r, bool multi, bool root, uint64_t* total_reads, uint64_t counters[BC_NCOUNTERS], uint64_t* n_rows) {
  if (r.args.fastq.size() >= 8 && r.args.fastq.compare(r.args.fastq.size() - 8, 8, "fastq.gz") == 0) {
    // input.rs:60-61
    printf("If this program stops reading before the expected number of sequencing reads, unzip the gzipped fastq and rerun.\n\n");
  }
  if (!multi) {
    if (bc_fastq_count(r.engine, r.args.fastq.c_str(), total_reads, progress, nullptr)) die("Read Fastq error: %s", bc_last_error());
    if (bc_engine_counters(r.engine, counters)) die("%s", bc_last_error());
    if (bc_engine_strand_reads(r.engine, nullptr, &r.reverse_matched)) die("%s", bc_last_error());
    return;
  }
  bc_comm* comm = make_comm(r.args);
  if (bc_fastq_count_shard(r.engine, r.args.fastq.c_str(), (uint32_t)r.args.rank, (uint32_t)r.args.world, total_reads,
                           root ? progress : nullptr, nullptr))
    die("Read Fastq error: %s", bc_last_error());
  if (bc_comm_sum_u64(comm, total_reads, 1, 0)) die("%s", bc_last_error());
  if (r.args.strand != BC_STRAND_FORWARD) {  // (a collective of its own, so that a forward job exchanges what it always did)
    if (bc_engine_strand_reads(r.engine, nullptr, &r.reverse_matched)) die("%s", bc_last_error());
    if (bc_comm_sum_u64(comm, &r.reverse_matched, 1, 0)) die("%s", bc_last_error());
  }
  if (bc_engine_finish_all(r.engine, comm, 0, counters, n_rows)) die("%s", bc_last_error());
  if (bc_comm_barrier(comm)) die("%s", bc_last_error());  // nobody leaves while a peer still reads its messages
  bc_comm_destroy(comm);
}

}  // namespace

int main(int argc, char** argv) {
  const double start_ms = now_ms();
  const time_t start = time(nullptr);
  Run r;
  r.args = parse_args(argc, argv);
  if (r.args.gpus > 1 && r.args.rank < 0) return launch_ranks(r.args, argc, argv);
  const bool multi = r.args.rank >= 0 && r.args.world > 1;
  const bool root = !multi || r.args.rank == 0;

  set_up_plan(r);
  uint64_t total_reads = 0, n_rows = 0;
  uint64_t counters[BC_NCOUNTERS];
  count_reads(r, multi, root, &total_reads, counters, &n_rows);
  if (root) {
    printf("Total sequences:             %s\r\n", commas((uint32_t)total_reads).c_str());  // input.rs:85-87
    printf("%s%s\n\n", errors_display(counters).c_str(), strand_display(r).c_str());  // main.rs:124
    printf("Compute time: %s\n\n", elapsed_text(now_ms() - start_ms).c_str());              // main.rs:127-135

    printf("-WRITING COUNTS-\n");
    describe_results(r);
    Writers& w = r.writers;
    w = choose_writers(gather_facts(r));
    // Marginals is the one choice that can fail at run time.  With the counts files on the device it is tried before
    // anything else (the sample keys are final); with them on the rows, after the rows are rebuilt (a row may add a key).
    if (w.counts == CountsWriter::DenseText && w.enrich == EnrichWriter::Marginals && !fill_enrichment(r))
      w = {CountsWriter::Rows, EnrichWriter::RowAdds};
    if (w.counts == CountsWriter::Rows) {
      if (!multi && bc_engine_finish(r.engine, &n_rows)) die("%s", bc_last_error());
      rebuild_rows(r, n_rows);
      if (w.enrich == EnrichWriter::Marginals && !fill_enrichment(r)) w.enrich = EnrichWriter::RowAdds;
    }
    report_writers(r);
    write_counts_files(r);
    report_enrichment_maps(r);
    write_stats_file(r, start, start_ms, counters, total_reads);
    printf("\nTotal time: %s\n", elapsed_text(now_ms() - start_ms).c_str());  // main.rs:156-164
  }
  bc_engine_destroy(r.engine);
  bc_plan_destroy(r.plan);
  return 0;
}
