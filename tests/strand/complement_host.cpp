// The complement table the orient kernel builds in LDS (csrc/bc_strand_kernels.h strand_complement), as host code: all 256
// bytes against the table written out here from the header's definition.  Built with -fsanitize=address,undefined by
// tests/test_strand_plan.py; prints the 256 complements as hex for the test to compare with the Python rc().
#include <stdio.h>
#include <string.h>

#include "../../ngs-barcode-count_amd/csrc/bc_strand_kernels.h"

int main() {
  unsigned char want[256];
  for (int c = 0; c < 256; ++c) want[c] = (unsigned char)c;
  const char* from = "ATCGMKRYVBHD";
  const char* to = "TAGCKMYRBVDH";
  for (size_t k = 0; k < strlen(from); ++k) {
    want[(unsigned char)from[k]] = (unsigned char)to[k];
    want[(unsigned char)(from[k] | 0x20)] = (unsigned char)(to[k] | 0x20);
  }
  int bad = 0;
  for (int c = 0; c < 256; ++c) {
    const unsigned char got = bc::strand_complement((unsigned char)c);
    if (got != want[c] || bc::strand_complement(got) != c) ++bad;
    printf("%02x", got);
  }
  printf("\n");
  return bad ? 1 : 0;
}
