// bc_cli_output.cpp -- the output side of `barcode-count`: display blocks, the rows rebuilt from the engine, the counts
// files and the stats file (output.rs:74-576; info.rs:141-172, 313-335, 618-659, 811-904).  Which writer a file gets is
// decided once (bc_cli_writers.hpp) and kept in Run::writers; everything here compares against those two enums.
#include "bc_cli_output.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include <algorithm>
#include <set>

[[noreturn]] void die(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "Error: ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  exit(1);
}

// num-format Locale::en
std::string commas(uint64_t v) {
  std::string s = std::to_string(v), out;
  for (size_t i = 0; i < s.size(); ++i) {
    if (i && (s.size() - i) % 3 == 0) out.push_back(',');
    out.push_back(s[i]);
  }
  return out;
}

double now_ms() {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  return tv.tv_sec * 1000.0 + tv.tv_usec / 1000.0;
}

std::string elapsed_text(double ms_total) {  // main.rs:128-134, output.rs:579-588
  const long long ms = (long long)ms_total;
  const long long secs = ms / 1000;
  char buf[128];
  snprintf(buf, sizeof buf, "%lld hours, %lld minutes, %lld.%03lld seconds", secs / 3600, (secs / 60) % 60, secs % 60,
           ms - secs * 1000);
  return buf;
}

namespace {

// f32 Display: shortest decimal that round-trips, no trailing ".0"
std::string f32_display(float v) {
  char buf[64];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof buf, "%.*g", prec, (double)v);
    if (strtof(buf, nullptr) == v) break;
  }
  std::string s = buf;
  if (s.find('e') != std::string::npos) {  // Rust never uses exponents for Display
    snprintf(buf, sizeof buf, "%f", (double)v);
    s = buf;
    while (s.find('.') != std::string::npos && (s.back() == '0' || s.back() == '.')) {
      const bool dot = s.back() == '.';
      s.pop_back();
      if (dot) break;
    }
  }
  return s;
}

std::string vec_debug(const std::vector<uint32_t>& v) {  // Rust {:?} of a Vec<u16>
  std::string s = "[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
  return s + "]";
}

bool has_sample_group(const Run& r) { return bc_plan_has_sample(r.plan) != 0; }

}  // namespace

std::string format_display(const Run& r) {  // info.rs:313-335
  const std::string regions = bc_plan_regions_string(r.plan);
  std::string key;
  std::set<char> seen;
  for (char c : regions) {
    if (!seen.insert(c).second) continue;
    if (c == 'S') key += "\nS: Sample barcode";
    if (c == 'B') key += "\nB: Counted barcode";
    if (c == 'C') key += "\nC: Constant region";
    if (c == 'R') key += "\nR: Random barcode";
  }
  return std::string("-FORMAT-\n") + bc_plan_format_string(r.plan) + "\n" + regions + key;
}

std::string max_errors_display(const Run& r) {  // info.rs:618-659
  std::vector<uint32_t> sizes, errs;
  for (uint32_t i = 0; i < r.barcode_num; ++i) {
    sizes.push_back(bc_plan_barcode_length(r.plan, i));
    errs.push_back(bc_plan_max_barcode_errors(r.plan, i));
  }
  std::string size_info, err_info;
  if (sizes.size() > 1) {
    size_info = "Barcode sizes: " + vec_debug(sizes);
    err_info = "Maximum mismatches allowed per barcode sequence: " + vec_debug(errs);
  } else if (sizes.size() == 1) {
    size_info = "Barcode size: " + std::to_string(sizes[0]);
    err_info = "Maximum mismatches allowed per barcode sequence: " + std::to_string(errs[0]);
  }
  const int32_t sl = bc_plan_sample_length(r.plan);
  const std::string dash = "--------------------------------------------------------------\n";
  return "-BARCODE INFO-\nConstant region size: " + std::to_string(bc_plan_constant_region_length(r.plan)) +
         "\nMaximum mismatches allowed per sequence: " + std::to_string(bc_plan_max_constant_errors(r.plan)) + "\n" + dash +
         "Sample barcode size: " + std::to_string(sl < 0 ? 0 : sl) +
         "\nMaximum mismatches allowed per sequence: " + std::to_string(bc_plan_max_sample_errors(r.plan)) + "\n" + dash +
         size_info + "\n" + err_info + "\n" + dash +
         "Minimum allowed average read quality score per barcode: " + f32_display(r.args.min_quality) + "\n";
}

std::string errors_display(const uint64_t c[BC_NCOUNTERS]) {  // info.rs:141-172 (AtomicU32: wraps at 2^32)
  auto g = [&](int k) { return commas((uint32_t)c[k]); };
  return "Correctly matched sequences: " + g(BC_MATCHED) + "\nConstant region mismatches:  " + g(BC_CONSTANT_REGION) +
         "\nSample barcode mismatches:   " + g(BC_SAMPLE_BARCODE) + "\nCounted barcode mismatches:  " + g(BC_BARCODE) +
         "\nDuplicates:                  " + g(BC_DUPLICATES) + "\nLow quality barcodes:        " + g(BC_LOW_QUALITY);
}

std::string strand_display(const Run& r) {
  if (r.args.strand == BC_STRAND_FORWARD) return "";
  return "\nReverse strand matches:      " + commas(r.reverse_matched);
}

// ---- what the writers decide on ---------------------------------------------------------------------------------------

// every sample key that exists before a row is seen (info.rs:698-719), the known sets, and the engine's index of each key
void describe_results(Run& r) {
  for (uint32_t i = 0; i < bc_plan_n_samples(r.plan); ++i) r.samples.emplace_back(bc_plan_sample_seq(r.plan, i), bc_plan_sample_id(r.plan, i));
  r.counted.resize(r.args.has_counted ? r.barcode_num : 0);
  for (uint32_t b = 0; b < r.counted.size(); ++b)
    for (uint32_t i = 0; i < bc_plan_n_counted(r.plan, b); ++i)
      r.counted[b].emplace_back(bc_plan_counted_seq(r.plan, b, i), bc_plan_counted_id(r.plan, b, i));
  for (const auto& s : r.samples) r.sample_keys.push_back(s.first);
  if (r.samples.empty() && !has_sample_group(r)) r.sample_keys.push_back("barcode");
  r.counted_map.resize(r.counted.size());
  for (size_t b = 0; b < r.counted.size(); ++b)
    for (const auto& kv : r.counted[b]) r.counted_map[b][kv.first] = kv.second;
  if (has_sample_group(r))
    for (uint32_t i = 0; i < r.samples.size(); ++i) r.sample_index[r.samples[i].first] = i;
  else
    r.sample_index["barcode"] = 0;
}

WriterFacts gather_facts(const Run& r) {
  WriterFacts f;
  f.dense = bc_plan_mode(r.plan) == 1;
  f.raw = bc_plan_mode(r.plan) == 2;
  f.enrich = r.args.enrich;
  f.counted_named_all = r.counted.size() == r.barcode_num;
  f.counted_whole = f.plain_ids = f.no_empty_id = true;
  for (const auto& set : r.counted) {
    f.counted_whole = f.counted_whole && !set.empty();
    for (const auto& kv : set) {
      // (an ID with a comma in it would split into other columns on the string path of enrichment)
      f.plain_ids = f.plain_ids && kv.second.find(',') == std::string::npos;
      f.no_empty_id = f.no_empty_id && !kv.second.empty();
    }
  }
  f.sample_group = has_sample_group(r);
  f.sample_ids = !r.samples.empty();
  f.wide = bc_engine_key_words(r.engine) > 1;
  uint64_t n_single = 0, n_double = 0;
  f.enrich_entries_ok = bc_engine_enrich_entries(r.engine, &n_single, &n_double) == BC_OK;
  auto env_is = [](const char* name, const char* value) {
    const char* v = getenv(name);
    return v && strcmp(v, value) == 0;
  };
  f.dense_text_off = env_is("BC_DEVICE_WRITERS", "0");
  f.dense_enrich_text_off = env_is("BC_DEVICE_ENRICH_WRITERS", "0");
  f.raw_text_on = env_is("BC_DEVICE_RAW_WRITERS", "1");
  f.raw_enrich_text_on = env_is("BC_DEVICE_RAW_ENRICH_WRITERS", "1");
  return f;
}

void report_writers(const Run& r) {
  if (getenv("BC_WRITERS_VERBOSE"))
    for (const auto& line : writer_reports(r.writers, bc_plan_mode(r.plan) == 2)) fprintf(stderr, "%s\n", line.c_str());
  if (r.writers.enrich != EnrichWriter::None && getenv("BC_ENRICH_VERBOSE"))
    fprintf(stderr, "%s\n", enrichment_report(r.writers).c_str());
}

void report_enrichment_maps(const Run& r) {  // (the device path of the Single / Double files builds none)
  if (r.writers.enrich == EnrichWriter::None || !getenv("BC_ENRICH_VERBOSE")) return;
  size_t keys = 0;
  for (const auto* maps : {&r.single_hash, &r.double_hash})
    for (const auto& kv : *maps) keys += kv.second.size();
  fprintf(stderr, "[barcode-count] enrichment maps: %zu keys on the host\n", keys);
}

// ---- the rows on the host ---------------------------------------------------------------------------------------------

namespace {

std::vector<std::string> split_commas(const std::string& s) {
  std::vector<std::string> out;
  size_t a = 0;
  for (size_t i = 0; i <= s.size(); ++i) {
    if (i == s.size() || s[i] == ',') {
      out.emplace_back(s, a, i - a);
      a = i + 1;
    }
  }
  return out;
}

std::string convert_code(const Run& r, const std::string& code) {  // output.rs:591-599
  const auto parts = split_commas(code);
  std::string out;
  for (size_t b = 0; b < parts.size(); ++b) {
    std::string id = parts[b];
    if (b < r.counted_map.size()) {
      auto it = r.counted_map[b].find(parts[b]);
      if (it != r.counted_map[b].end()) id = it->second;
    }
    out += (b ? "," : "") + id;
  }
  return out;
}

void add_row(Run& r, const std::string& key, const std::string& code, const std::string& written, uint64_t cnt) {
  // keys that only exist once a read lands on them: raw sample barcodes (info.rs:742-757) and the
  // "barcode" entry of a random-barcode run with a sample file but no sample group (info.rs:792-801)
  auto it = r.results.find(key);
  if (it == r.results.end()) {
    if (std::find(r.sample_keys.begin(), r.sample_keys.end(), key) == r.sample_keys.end()) r.sample_keys.push_back(key);
    it = r.results.emplace(key, std::vector<Run::Row>()).first;
  }
  it->second.push_back({code, written, cnt});
  if (r.args.merge_output) r.results_map[key][code] = cnt;
}

// dense plan: rows come as indices into the known sets; the sequence / ID strings are looked up
void rebuild_dense_rows(Run& r, uint64_t n_rows) {
  const bool sample_group = has_sample_group(r);
  const uint32_t nb = r.barcode_num ? r.barcode_num : 1;
  const uint64_t block = 1u << 20;
  std::vector<uint32_t> sidx(block), bidx(block * nb);
  std::vector<uint64_t> cnt(block);
  for (uint64_t first = 0; first < n_rows; first += block) {
    const uint64_t n = std::min(block, n_rows - first);
    if (bc_engine_rows(r.engine, first, n, sidx.data(), bidx.data(), cnt.data())) die("%s", bc_last_error());
    for (uint64_t i = 0; i < n; ++i) {
      std::string code, written;
      for (uint32_t b = 0; b < r.barcode_num; ++b) {
        const auto& kv = r.counted[b][bidx[i * nb + b]];
        if (b) {
          code.push_back(',');
          written.push_back(',');
        }
        code += kv.first;
        written += kv.second;
      }
      add_row(r, sample_group ? r.samples[sidx[i]].first : std::string("barcode"), code, written, cnt[i]);
    }
  }
}

}  // namespace

void rebuild_rows(Run& r, uint64_t n_rows) {
  if (bc_plan_mode(r.plan) == 1) return rebuild_dense_rows(r, n_rows);
  for (uint64_t i = 0; i < n_rows; ++i) {
    char sample[64], tuple[2048];
    uint64_t cnt = 0;
    if (bc_engine_row_text(r.engine, i, sample, sizeof sample, tuple, sizeof tuple, &cnt)) die("%s", bc_last_error());
    add_row(r, sample, tuple, r.counted.empty() ? std::string(tuple) : convert_code(r, tuple), cnt);
  }
}

// ---- Single / Double sums on the host -----------------------------------------------------------------------------------

namespace {

void add_single(Run& r, const std::string& sample, const std::string& barcode_string, uint64_t count) {  // info.rs:840-866
  const auto parts = split_commas(barcode_string);
  for (size_t index = 0; index < parts.size(); ++index) {
    std::string s;
    for (size_t x = 0; x < parts.size(); ++x) {
      if (x == index) s += parts[index];
      if (x != parts.size() - 1) s.push_back(',');
    }
    auto it = r.single_hash.find(sample);
    if (it != r.single_hash.end()) it->second[s] += count;  // else: the add lands in a temporary (info.rs:862)
  }
}

void add_double(Run& r, const std::string& sample, const std::string& barcode_string, uint64_t count) {  // info.rs:869-904
  const auto parts = split_commas(barcode_string);
  const size_t n = parts.size();
  for (size_t first = 0; first + 1 < n; ++first) {
    for (size_t add = 1; add < n - first; ++add) {
      std::string s;
      for (size_t col = 0; col < n; ++col) {
        if (col == first)
          s += parts[first];
        else if (col == first + add)
          s += parts[first + add];
        if (col != n - 1) s.push_back(',');
      }
      auto it = r.double_hash.find(sample);
      if (it != r.double_hash.end()) it->second[s] += count;
    }
  }
}

void add_sorted(std::map<std::string, uint64_t>& m, std::vector<std::pair<std::string, uint64_t>>& kv) {
  std::sort(kv.begin(), kv.end());
  for (size_t i = 0; i < kv.size();) {
    uint64_t sum = 0;
    size_t j = i;
    for (; j < kv.size() && kv[j].first == kv[i].first; ++j) sum += kv[j].second;
    m.emplace_hint(m.end(), std::move(kv[i].first), sum);  // (ascending keys into an empty map: constant time each)
    i = j;
  }
  kv.clear();
}

}  // namespace

// Dense plans: the whole of single_hash / double_hash at once from the device's marginal sums of the table
// (bc_engine_enrich), in place of add_single / add_double on every row.  Keys are built as add_single / add_double
// build them from a row's IDs; sequences of one group that share an ID add up; a key exists where its sum is not zero
// (the string path makes one when a row, count >= 1, adds to it).  Maps of samples the writers do not know stay out,
// as the string path's adds land in a temporary for them (info.rs:862).  Reads sample_keys: with the rows on the host it
// runs after rebuild_rows, which may append to them.
bool fill_enrichment(Run& r) {
  const bool sample_group = has_sample_group(r);
  const uint32_t G = r.barcode_num;
  uint64_t n_single = 0, n_double = 0;
  if (bc_engine_enrich_entries(r.engine, &n_single, &n_double) != BC_OK) return false;
  std::vector<uint64_t> single(n_single), dbl(n_double);
  const int rc = bc_engine_enrich(r.engine, single.data(), n_double ? dbl.data() : nullptr);
  if (rc == BC_ERR_NOMEM) return false;  // (no room for the device scratch: the rows build the maps as before)
  if (rc != BC_OK) die("%s", bc_last_error());
  std::vector<uint64_t> off(G + 1, 0);
  for (uint32_t g = 0; g < G; ++g) off[g + 1] = off[g] + r.counted[g].size();
  const uint64_t sum_n = off[G], S = sum_n ? n_single / sum_n : 0, P = S ? n_double / S : 0;
  auto commas_n = [](size_t n) { return std::string(n, ','); };
  std::vector<std::pair<std::string, uint64_t>> kv;
  for (uint64_t s = 0; s < S; ++s) {
    const std::string key = sample_group ? r.samples[s].first : std::string("barcode");
    if (std::find(r.sample_keys.begin(), r.sample_keys.end(), key) == r.sample_keys.end()) continue;
    const uint64_t* srow = single.data() + s * sum_n;
    for (uint32_t g = 0; g < G; ++g)
      for (size_t i = 0; i < r.counted[g].size(); ++i)
        if (const uint64_t v = srow[off[g] + i]) kv.emplace_back(commas_n(g) + r.counted[g][i].second + commas_n(G - 1 - g), v);
    if (!kv.empty()) add_sorted(r.single_hash[key], kv);
    if (!P) continue;
    const uint64_t* drow = dbl.data() + s * P;
    for (uint32_t g = 0; g + 1 < G; ++g)  // pairs in add_double's order: (0,1), (0,2), .., (1,2), ..
      for (uint32_t h = g + 1; h < G; ++h) {
        const size_t nh = r.counted[h].size();
        for (size_t i = 0; i < r.counted[g].size(); ++i)
          for (size_t j = 0; j < nh; ++j)
            if (const uint64_t v = drow[i * nh + j])
              kv.emplace_back(commas_n(g) + r.counted[g][i].second + commas_n(h - g) + r.counted[h][j].second +
                                  commas_n(G - 1 - h), v);
        drow += r.counted[g].size() * nh;
      }
    if (!kv.empty()) add_sorted(r.double_hash[key], kv);
  }
  return true;
}

// ---- the counts files -------------------------------------------------------------------------------------------------

namespace {

enum Enriched { kSingle, kDouble, kFull };  // a family of files; kSingle / kDouble index kEnrichKind

const int kEnrichKind[] = {BC_ENRICH_SINGLE, BC_ENRICH_DOUBLE};

std::string sample_name(const Run& r, const std::string& key) {  // output.rs:136-143
  if (r.samples.empty()) return key;
  for (const auto& s : r.samples)
    if (s.first == key) return s.second;
  return "barcode";
}

std::string create_header(const Run& r) {  // output.rs:184-196
  if (r.barcode_num > 1) {
    std::string h = "Barcode_1";
    for (uint32_t n = 1; n < r.barcode_num; ++n) h += ",Barcode_" + std::to_string(n + 1);
    return h;
  }
  return "Barcode";
}

// add_counts_string (output.rs:199-361): a sample's rows appended to `text`, new compounds to the merged text
uint64_t add_counts_string(Run& r, const std::string& sample, const std::vector<std::string>& samples, Enriched type,
                           std::string& text) {
  std::vector<Run::Row> enriched_rows;
  static const decltype(r.single_hash) none;
  const auto& holder = type == kSingle ? r.single_hash : (type == kDouble ? r.double_hash : none);
  if (type != kFull)
    for (const auto& kv : holder.at(sample)) enriched_rows.push_back({kv.first, kv.first, kv.second});
  const std::vector<Run::Row>& rows = type == kFull ? r.results[sample] : enriched_rows;
  uint64_t barcode_num = 0;
  for (const auto& row : rows) {
    const std::string& code = row.code;
    const uint64_t count = row.count;
    ++barcode_num;
    if (barcode_num % 50000 == 0) {
      printf("Barcodes counted: %s\r", commas(barcode_num).c_str());
      fflush(stdout);
    }
    const std::string& written = row.written;
    if (r.args.merge_output) {
      if (r.compounds_written.insert(code).second) {
        r.merged_count++;
        std::string merged_row = written;
        for (const auto& sb : samples) {
          uint64_t c = 0;
          if (type == kFull) {
            auto ms = r.results_map.find(sb);
            if (ms != r.results_map.end()) {
              auto it = ms->second.find(code);
              if (it != ms->second.end()) c = it->second;
            }
          } else {
            auto it = holder.at(sb).find(code);
            if (it != holder.at(sb).end()) c = it->second;
          }
          merged_row += "," + std::to_string(c);
        }
        r.merge_text += merged_row + "\n";
      }
    }
    text += written + "," + std::to_string(count) + "\n";
    if (type == kFull && r.writers.enrich == EnrichWriter::RowAdds) {
      add_single(r, sample, written, count);
      if (r.barcode_num > 2) add_double(r, sample, written, count);
    }
  }
  printf("Barcodes counted: %s\r\n", commas(barcode_num).c_str());
  return barcode_num;
}

std::string out_path(const Run& r, const std::string& name) {
  std::string path = r.args.output_dir;
  if (!path.empty() && path.back() != '/') path.push_back('/');
  return path + name;
}

void write_file(const Run& r, const std::string& name, const std::string& text) {
  const std::string path = out_path(r, name);
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) die("cannot create %s", path.c_str());
  fwrite(text.data(), 1, text.size(), f);
  fclose(f);
}

// The device's renderers, one file of one sample and the merged file of a list of samples, by writer.  The writers that
// go through host strings have none.
struct CountsRender {
  int (*single)(bc_engine*, uint32_t, bc_text_fn, void*, uint64_t*);
  int (*merged)(bc_engine*, const uint32_t*, uint32_t, bc_text_fn, void*, uint64_t*);
};
const CountsRender kCountsRender[] = {
    /* Rows      */ {nullptr, nullptr},
    /* DenseText */ {bc_engine_render_counts, bc_engine_render_merged},
    /* RawText   */ {bc_engine_render_raw_counts, bc_engine_render_raw_merged},
    /* WideText  */ {bc_engine_render_wide_counts, bc_engine_render_wide_merged},
};
struct EnrichRender {  // (the second argument is the kind, BC_ENRICH_SINGLE / BC_ENRICH_DOUBLE)
  int (*single)(bc_engine*, int, uint32_t, bc_text_fn, void*, uint64_t*);
  int (*merged)(bc_engine*, int, const uint32_t*, uint32_t, bc_text_fn, void*, uint64_t*);
};
const EnrichRender kEnrichRender[] = {
    /* None      */ {nullptr, nullptr},
    /* RowAdds   */ {nullptr, nullptr},
    /* Marginals */ {nullptr, nullptr},
    /* DenseText */ {bc_engine_render_enriched, bc_engine_render_enriched_merged},
    /* RawText   */ {bc_engine_render_raw_enriched, bc_engine_render_raw_enriched_merged},
};

// does the device render this family's files?
bool device_text(const Run& r, Enriched type) {
  return type == kFull ? kCountsRender[(int)r.writers.counts].single != nullptr
                       : kEnrichRender[(int)r.writers.enrich].single != nullptr;
}

// The device path of a file: `head` (the header of a sample's file, the header line of the merged one), then the text
// chunks as they leave the device.  `cols` are the engine's sample indices: one for a sample's file; for the merged file
// the columns in the header's order, a line per tuple (per key) that counts in any of them.  -> the number of lines
int text_to_file(const char* text, size_t n, void* user) { return fwrite(text, 1, n, (FILE*)user) == n ? 0 : 1; }
uint64_t render_file(Run& r, const std::string& name, const std::string& head, const std::vector<uint32_t>& cols, bool merged,
                     Enriched type) {
  const std::string path = out_path(r, name);
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) die("cannot create %s", path.c_str());
  if (fwrite(head.data(), 1, head.size(), f) != head.size()) die("%s: write failed", path.c_str());
  uint64_t n = 0;
  const uint32_t n_cols = (uint32_t)cols.size();
  int rc;
  if (type == kFull) {
    const CountsRender& via = kCountsRender[(int)r.writers.counts];
    rc = merged ? via.merged(r.engine, cols.data(), n_cols, text_to_file, f, &n) : via.single(r.engine, cols[0], text_to_file, f, &n);
  } else {
    const EnrichRender& via = kEnrichRender[(int)r.writers.enrich];
    rc = merged ? via.merged(r.engine, kEnrichKind[type], cols.data(), n_cols, text_to_file, f, &n)
                : via.single(r.engine, kEnrichKind[type], cols[0], text_to_file, f, &n);
  }
  if (rc != BC_OK) die("%s: %s", path.c_str(), ferror(f) ? "write failed" : bc_last_error());
  if (fclose(f) != 0) die("%s: write failed", path.c_str());
  return n;
}

// what add_counts_string prints while it walks n rows: a line every 50,000 rows, and the total
void print_rows_progress(uint64_t n) {
  for (uint64_t k = 50000; k <= n; k += 50000) printf("Barcodes counted: %s\r", commas(k).c_str());
  printf("Barcodes counted: %s\r\n", commas(n).c_str());
}

std::vector<std::string> ordered_samples(const Run& r, std::vector<std::string> keys) {
  // output.rs:91-97: with a sample file the keys are ordered by sample ID (for the merged columns)
  if (!r.samples.empty())
    std::stable_sort(keys.begin(), keys.end(),
                     [&](const std::string& a, const std::string& b) { return sample_name(r, a) < sample_name(r, b); });
  return keys;
}

// One family of files: the full counts (output.rs:74-181) or the Single / Double sums (output.rs:364-485).  A file per
// sample, then with -m the merged file.  A file's body comes from the host's strings (add_counts_string, which also
// collects the merged file's text and count) or from the device (render_file; stdout gets what add_counts_string would
// have printed for that many rows).
void write_family(Run& r, Enriched type) {
  const bool full = type == kFull, device = device_text(r, type);
  const std::string descriptor = full ? "" : (type == kSingle ? ".Single" : ".Double");
  // the host path of the Single / Double files lists the sample keys that have a map, the device path every key (as
  // every key has a map on the host path: add_sample_barcodes below)
  std::vector<std::string> keys;
  for (const auto& k : r.sample_keys)
    if (full || device || (type == kSingle ? r.single_hash : r.double_hash).count(k)) keys.push_back(k);
  const auto samples = ordered_samples(r, keys);
  if (full && (r.writers.enrich == EnrichWriter::RowAdds || r.writers.enrich == EnrichWriter::Marginals))
    for (const auto& k : samples) {  // ResultsEnrichment::add_sample_barcodes, info.rs:829-837
      r.single_hash[k];
      r.double_hash[k];
    }
  std::string header = create_header(r);
  if (r.args.merge_output) {
    if (full && samples.size() == 1) {
      fprintf(stderr, "Merged file cannot be created without multiple sample barcodes\n");
      printf("\n");
      r.args.merge_output = false;  // (for the Single / Double families too)
    } else {
      std::string h = header;
      for (const auto& sb : samples) h += "," + sample_name(r, sb);
      r.merge_text += h + "\n";
    }
  }
  header += ",Count\n";
  for (const auto& sb : samples) {
    const std::string file_name = r.args.prefix + "_" + sample_name(r, sb) + "_counts" + descriptor + ".csv";
    printf("%s\n", file_name.c_str());
    r.output_files.push_back(file_name);
    uint64_t count;
    if (device) {
      count = render_file(r, file_name, header, {r.sample_index.at(sb)}, false, type);
      print_rows_progress(count);
    } else {
      std::string text = header;
      count = add_counts_string(r, sb, samples, type, text);
      write_file(r, file_name, text);
    }
    r.output_counts.push_back(count);
  }
  if (r.args.merge_output) {
    const std::string merged = r.args.prefix + "_counts.all" + descriptor + ".csv";
    printf("%s\n", merged.c_str());
    r.output_files.push_back(merged);
    if (device) {
      std::vector<uint32_t> cols;
      for (const auto& sb : samples) cols.push_back(r.sample_index.at(sb));
      r.merged_count = render_file(r, merged, r.merge_text, cols, true, type);
    } else {
      write_file(r, merged, r.merge_text);
    }
    printf("Barcodes counted: %s\n", commas(r.merged_count).c_str());
    r.merge_text.clear();
    // output.rs:171 (the full family: the count to the front, though the file name went to the back), output.rs:478-481
    r.output_counts.insert(full ? r.output_counts.begin() : r.output_counts.end() - (long)samples.size(), r.merged_count);
    r.merged_count = 0;
  }
}

std::string time_text(time_t t) {
  char buf[64];
  strftime(buf, sizeof buf, "%Y-%m-%d %H:%M:%S", localtime(&t));
  return buf;
}

}  // namespace

void write_counts_files(Run& r) {
  write_family(r, kFull);
  if (r.writers.enrich == EnrichWriter::None) return;
  write_family(r, kSingle);
  if (r.barcode_num > 2) write_family(r, kDouble);
}

void write_stats_file(const Run& r, time_t start, double start_ms, const uint64_t counters[BC_NCOUNTERS], uint64_t total_reads) {
  // output.rs:488-576; the file is appended to
  const std::string path = out_path(r, r.args.prefix + "_barcode_stats.txt");
  FILE* f = fopen(path.c_str(), "ab");
  if (!f) die("cannot open %s", path.c_str());
  std::string s;
  s += "-TIME INFORMATION-\nStart: " + time_text(start) + "\nFinish: " + time_text(time(nullptr)) +
       "\nTotal time: " + elapsed_text(now_ms() - start_ms) + "\n\n";
  s += "-INPUT FILES-\nFastq: " + r.args.fastq + "\nFormat: " + r.args.format +
       "\nSamples: " + (r.args.has_samples ? r.args.sample_barcodes : std::string("None")) +
       "\nBarcodes: " + (r.args.has_counted ? r.args.counted_barcodes : std::string("None")) + "\n\n";
  s += format_display(r) + "\n\n";
  s += max_errors_display(r) + "\n";
  s += "-RESULTS-\nTotal sequences:             " + commas((uint32_t)total_reads) + "\n" + errors_display(counters) + strand_display(r) + "\n\n";
  s += "-OUTPUT FILES-\n";
  for (size_t i = 0; i < r.output_files.size() && i < r.output_counts.size(); ++i)
    s += "File & barcodes counted: " + r.output_files[i] + "\t" + commas(r.output_counts[i]) + "\n";
  s += "\n";
  const std::string& fq = r.args.fastq;
  if (fq.size() >= 2 && fq.compare(fq.size() - 2, 2, "gz") == 0 && (uint32_t)total_reads < 1000000) {
    const char* warning =
        "WARNING: The program may have stopped early with the gzipped file.  Unzip the fastq.gz and rerun the algorithm "
        "on the unzipped fastq file if the number of reads is expected to be above 1,000,000 ";
    printf("\n%s\n\n", warning);
    s += std::string("\n") + warning + "\n";
  }
  s += "--------------------------------------------------------------------------------------------------\n\n\n";
  fwrite(s.data(), 1, s.size(), f);
  fclose(f);
}
