// Host tool (no GPU): the tile lists of the dual launch as csrc/x3_layout.h deals them (dual_tiles_per_block, dual_short_blocks,
// dual_block_tiles) -- the very functions the launcher and the kernel call.  Reads problems from stdin, one per line:
//   n_long nk_long n_short nk_short      (tiles and ring tiles per tile of the long-K and of the short-K problem)
// and prints for each:  "P per blocks"  followed by one line  "B seq0 count"  per block of the short problem.
//   g++ -O1 -std=c++17 -I tfkaldi_amd/csrc tools/x3_dual_tiles_check.cpp -o /tmp/x3_dual_tiles_check
// tests/test_x3_dual_tiles.py checks the output.
#include <stdio.h>

#include "x3_layout.h"

int main() {
  int n_long, nk_long, n_short, nk_short;
  while (scanf("%d %d %d %d", &n_long, &nk_long, &n_short, &nk_short) == 4) {
    const int per = tfk::x3::dual_tiles_per_block(n_long, nk_long, n_short, nk_short);
    const int blocks = tfk::x3::dual_short_blocks(n_short, per);
    printf("P %d %d\n", per, blocks);
    for (int g = 0; g < blocks; ++g) {
      int seq0, count;
      tfk::x3::dual_block_tiles(n_short, per, g, seq0, count);
      printf("B %d %d\n", seq0, count);
    }
  }
  return 0;
}
