// Host tool (no GPU): the rule by which the fp32-emulating dual launch may do batch norm's backward inside its dA blocks
// (csrc/x3_layout.h: dual_bnb_eligible) -- the very function the launcher calls.  Reads cases from stdin, one per line:
//   T chunk_rows k_da stacked max_tiles
// and prints 1 or 0 for each.
//   g++ -O1 -std=c++17 -I tfkaldi_amd/csrc tools/x3_dual_bnb_check.cpp -o /tmp/x3_dual_bnb_check
// tests/test_x3_dual_bnb.py checks the output.
#include <stdio.h>

#include "x3_layout.h"

int main() {
  int T, chunk_rows, k_da, stacked, max_tiles;
  while (scanf("%d %d %d %d %d", &T, &chunk_rows, &k_da, &stacked, &max_tiles) == 5)
    printf("%d\n", tfk::x3::dual_bnb_eligible(T, chunk_rows, k_da, stacked != 0, max_tiles) ? 1 : 0);
  return 0;
}
