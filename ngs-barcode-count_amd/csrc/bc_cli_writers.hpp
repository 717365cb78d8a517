// bc_cli_writers.hpp -- which writer a `barcode-count` run gets for its files, decided once from plain facts.
//
// Pure: no engine call, no getenv.  The caller (gather_facts, bc_cli_output.cpp) fills WriterFacts, choose_writers picks
// one writer for the full-counts files and one for the Single / Double files, and writer_reports / enrichment_report
// word what BC_WRITERS_VERBOSE / BC_ENRICH_VERBOSE print.  tests/cli/writers_host.cpp walks every combination.
#pragma once

#include <string>
#include <vector>

// the full-counts files
enum class CountsWriter {
  Rows,       // per-row host strings (bc_engine_finish + bc_engine_rows / bc_engine_row_text)
  DenseText,  // a dense plan's table as text from the device (bc_engine_render_counts / _merged)
  RawText,    // a raw-key plan's key map sorted and rendered on the device (bc_engine_render_raw_counts / _merged)
  WideText    // ... with keys several words wide (bc_engine_render_wide_counts / _merged)
};
// the Single / Double files
enum class EnrichWriter {
  None,       // no -e
  RowAdds,    // host maps, built by add_single / add_double on every row
  Marginals,  // host maps, filled at once from the device's marginal sums (bc_engine_enrich); can fail at run time
              // (BC_ERR_NOMEM), and the caller then falls back to RowAdds
  DenseText,  // text from the device, no host maps (bc_engine_render_enriched / _merged)
  RawText     // ... of a raw-key plan (bc_engine_render_raw_enriched / _merged)
};

struct WriterFacts {
  bool dense = false, raw = false;  // bc_plan_mode is 1, is 2 (a plan has one mode: with both set, dense counts)
  bool enrich = false;              // -e, after the "fewer than 2 counted barcodes" downgrade
  bool counted_named_all = false;   // the counted file names every counted barcode
  bool counted_whole = false;       // the counted file is absent, or leaves no counted barcode without names
  bool sample_group = false;        // the scheme has a sample barcode
  bool sample_ids = false;          // a sample file was loaded
  bool plain_ids = false;           // no counted ID holds a comma
  bool no_empty_id = false;         // no counted ID is empty
  bool wide = false;                // bc_engine_key_words() > 1
  bool enrich_entries_ok = false;   // bc_engine_enrich_entries() == BC_OK
  // the environment's switches, each as the boolean its polarity gives
  bool dense_text_off = false;         // BC_DEVICE_WRITERS=0
  bool dense_enrich_text_off = false;  // BC_DEVICE_ENRICH_WRITERS=0
  bool raw_text_on = false;            // BC_DEVICE_RAW_WRITERS=1
  bool raw_enrich_text_on = false;     // BC_DEVICE_RAW_ENRICH_WRITERS=1
};

struct Writers {
  CountsWriter counts = CountsWriter::Rows;
  EnrichWriter enrich = EnrichWriter::None;
};

inline Writers choose_writers(const WriterFacts& f) {
  // Dense plans: the table is rendered on the device and no row becomes a host string.  Kept on the rows: a counted file
  // that names only some of the barcodes, and a sample file next to a scheme without a sample group, whose "barcode" key
  // exists only once a row lands on it.
  const bool dense_text = f.dense && !f.dense_text_off && f.counted_named_all && (f.sample_group || !f.sample_ids);
  // Raw-key plans, only when asked for: the key map is sorted and rendered on the device.  Kept on the rows: a sample
  // barcode kept raw (its samples are captures), a sample file without a sample group (as above), a counted file that
  // names only some of the barcodes, and enrichment unless it is asked for as well and the keys are one word wide.
  // (No test of the IDs is needed, unlike for dense plans: with one-word keys and the sample barcode known or absent, a
  // plan is a raw-key plan only when some counted group has no names, so `counted_whole` holds only without a counted
  // file, and every field is then a capture, never an ID.)
  const bool raw_text = f.raw && !f.dense && f.raw_text_on && f.sample_group == f.sample_ids && f.counted_whole &&
                        (!f.enrich || (f.raw_enrich_text_on && !f.wide));
  Writers w;
  if (raw_text)
    w.counts = f.wide ? CountsWriter::WideText : CountsWriter::RawText;
  else if (dense_text && !(f.enrich && !f.plain_ids))  // (an ID with a comma needs the string path of enrichment: rows)
    w.counts = CountsWriter::DenseText;
  if (!f.enrich) return w;
  if (raw_text)
    w.enrich = EnrichWriter::RawText;
  // not with an empty ID: ",," is then the text of keys in different groups, which the reference's maps add up and the
  // device's key space keeps apart
  else if (dense_text && f.plain_ids && f.no_empty_id && !f.dense_enrich_text_off && f.enrich_entries_ok)
    w.enrich = EnrichWriter::DenseText;
  else if (f.dense && f.counted_named_all && f.plain_ids)
    w.enrich = EnrichWriter::Marginals;
  else
    w.enrich = EnrichWriter::RowAdds;
  return w;
}

// what BC_WRITERS_VERBOSE prints on stderr (tests assert these lines)
inline std::vector<std::string> writer_reports(const Writers& w, bool raw_plan) {
  const std::string rows = "per-row strings";
  std::vector<std::string> out;
  out.push_back("[barcode-count] writers: " + (w.counts == CountsWriter::DenseText ? "device text (bc_engine_render_counts)" : rows));
  if (w.enrich != EnrichWriter::None)
    out.push_back("[barcode-count] enrichment writers: " +
                  (w.enrich == EnrichWriter::RawText     ? "device text (bc_engine_render_raw_enriched)"
                   : w.enrich == EnrichWriter::DenseText ? "device text (bc_engine_render_enriched)"
                                                         : rows));
  if (raw_plan)
    out.push_back("[barcode-count] raw writers: " +
                  (w.counts == CountsWriter::RawText    ? "device text (bc_engine_render_raw_counts)"
                   : w.counts == CountsWriter::WideText ? "device text (bc_engine_render_wide_counts)"
                                                        : rows));
  return out;
}

// what BC_ENRICH_VERBOSE prints: which path builds the Single / Double sums ("" without -e).  For the caller this comes
// after its Marginals attempt, so Marginals here means that the maps are filled.
inline std::string enrichment_report(const Writers& w) {
  switch (w.enrich) {
    case EnrichWriter::None: return "";
    case EnrichWriter::RowAdds: return "[barcode-count] enrichment: per-row string adds";
    case EnrichWriter::Marginals: return "[barcode-count] enrichment: device marginal sums (bc_engine_enrich)";
    case EnrichWriter::DenseText: return "[barcode-count] enrichment: device marginal sums (bc_engine_render_enriched)";
    case EnrichWriter::RawText: return "[barcode-count] enrichment: device run sums (bc_engine_render_raw_enriched)";
  }
  return "";
}
