// writers_host -- choose_writers and its reports (csrc/bc_cli_writers.hpp) over every combination of the fifteen facts,
// compiled with sanitizers.  TEST-ONLY.
//
//   writers_host  ->  stdout, per combination (bit k of the number is FACTS[k] of tests/test_cli_writers.py):
//     <number> <counts writer> <enrichment writer>
//     every line of writer_reports, then the line of enrichment_report when there is one, each behind a tab
#include <stdio.h>

#include "../../ngs-barcode-count_amd/csrc/bc_cli_writers.hpp"

int main() {
  bool WriterFacts::*const facts[] = {
      &WriterFacts::dense, &WriterFacts::raw, &WriterFacts::enrich, &WriterFacts::counted_named_all,
      &WriterFacts::counted_whole, &WriterFacts::sample_group, &WriterFacts::sample_ids, &WriterFacts::plain_ids,
      &WriterFacts::no_empty_id, &WriterFacts::wide, &WriterFacts::enrich_entries_ok, &WriterFacts::dense_text_off,
      &WriterFacts::dense_enrich_text_off, &WriterFacts::raw_text_on, &WriterFacts::raw_enrich_text_on};
  const unsigned n_facts = sizeof facts / sizeof facts[0];
  static const char* const counts_names[] = {"Rows", "DenseText", "RawText", "WideText"};
  static const char* const enrich_names[] = {"None", "RowAdds", "Marginals", "DenseText", "RawText"};
  for (unsigned bits = 0; bits < (1u << n_facts); ++bits) {
    WriterFacts f;
    for (unsigned k = 0; k < n_facts; ++k) f.*facts[k] = (bits >> k) & 1;
    const Writers w = choose_writers(f);
    printf("%u %s %s\n", bits, counts_names[(int)w.counts], enrich_names[(int)w.enrich]);
    for (const auto& line : writer_reports(w, f.raw && !f.dense)) printf("\t%s\n", line.c_str());  // (one mode: dense first)
    const std::string enrichment = enrichment_report(w);
    if (!enrichment.empty()) printf("\t%s\n", enrichment.c_str());
  }
  return 0;
}
