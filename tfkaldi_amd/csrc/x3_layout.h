// Memory and LDS layouts of the fp32-emulating contraction ("bf16x3", gemm_bf16.h) -- index arithmetic only, shared by the
// kernels (gemm_bf16.hip, kernels.hip) and by a host-side checker (tools/x3_layout_check.cpp, runs without a GPU).
//
// MEMORY.  An fp32 matrix [rows, ld] (ld a multiple of 32, rows rounded up to even) is held as three bf16 planes
// p0 + p1 + p2 = x exactly, TILED: the unit is the 2-row x 32-column block (R, B) = (row / 2, col / 32), 384 bytes =
// three 128-byte lines, one per plane, each line holding the block's two rows of that plane:
//       element (row, col), plane q  at  ((row / 2) * (ld / 32) + col / 32) * 192 + q * 64 + (row & 1) * 32 + col % 32
// (bf16 elements from the matrix's base).  Why: the L1-miss path from L2 into a CU moves whole 128-byte lines at ~36 B/clk/CU,
// and a ring slot of the contraction holds 32 k of both operands.  With one plane per array (round 4) a k-contiguous operand
// fetched a 64-byte piece per row, plane and slot -- half of every line it pulled, 21 B/clk/CU of useful bytes
// (profiles/r04_gemm_f32x3_ablation.txt); planes interleaved per row gave 192-byte runs, 1.5 lines each of which the second was
// shared with the NEXT slot: 27 B/clk/CU.  Here whatever a block stages in one slot consists of COMPLETE lines in both uses of a
// matrix: as the k-contiguous operand (a tile of 128 rows x 32 k = 64 units, each wholly inside it) and as the k-strided operand
// (32 k-rows x 128 columns = 16 row pairs x 4 units).
//
// LDS (one ring slot = 32 k of all three planes of both operands; every image is written lane-linearly by
// `buffer_load_dwordx4 ... lds`, 16-byte chunk n of an image at byte 16 n, so the permutations below are applied on the SOURCE
// side of the DMA and undone by the fragment reads; consecutive chunks of an image come from consecutive memory):
//   k-contiguous operand, EXT rows:   row pair P at P * 384: [plane q][row parity h][4 chunks of 8 k], the k-chunk c of row r at
//       slot c ^ ((r >> 2) & 3).  A lane's MFMA operand (8 consecutive k of one row and plane) is one ds_read_b128; the 16 lanes
//       of a service group touch 16 distinct 16-byte bank slots.
//   k-strided operand, EXT columns:   k-row pair P at P * (EXT / 32) * 384: per 32-column block b the unit's six 64-byte QUADRANTS
//       n = 6 b + 2 q + h (plane q, row parity h), quadrant n stored at n ^ (2 * (P & 1)): the four k-rows a 16-lane group of
//       ds_read_b64_tr_b16 reads (two pairs) then sit in four different quadrants of the 256-byte bank row.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define X3_HD __host__ __device__ __forceinline__
#else
#define X3_HD inline
#endif

namespace tfk {
namespace x3 {

constexpr int kSlotK = 32;  // k per ring slot = columns per unit

// elements a matrix of `rows` rows occupies (all three planes)
X3_HD size_t elems(size_t rows, int ld) { return ((rows + 1) >> 1) * (size_t)(ld >> 5) * 192; }
// element offset of plane 0 of element (row, col); planes 1, 2: + 64, + 128
X3_HD size_t at(size_t row, int col, int ld) {
  return ((row >> 1) * (size_t)(ld >> 5) + (size_t)(col >> 5)) * 192 + (row & 1) * 32 + (col & 31);
}

// ---- k-contiguous image: 24 chunks of 16 bytes per row pair ----
X3_HD int kc_swz(int r) { return (r >> 2) & 3; }
// chunk n of the image holds k-chunk c (k = 8 c .. 8 c + 7) of plane q of row r
X3_HD void kc_decode(int n, int& r, int& q, int& c) {
  const int P = n / 24, rem = n - P * 24;
  q = rem >> 3;
  r = 2 * P + ((rem >> 2) & 1);
  c = (rem & 3) ^ kc_swz(r);
}
X3_HD int kc_addr(int r, int q, int c) { return (r >> 1) * 384 + q * 128 + (r & 1) * 64 + ((c ^ kc_swz(r)) << 4); }

// ---- k-strided image: EXT / 32 units of 6 quadrants (64 bytes) per k-row pair ----
// chunk n of the image holds ext-chunk e8 (8 ext) of block b (32 ext), plane q, of k-row r
template <int EXT>
X3_HD void ks_decode(int n, int& r, int& b, int& q, int& e8) {
  constexpr int CPP = EXT / 32 * 24;  // chunks per row pair
  const int P = n / CPP, pos = n - P * CPP;
  const int nq = (pos >> 2) ^ ((P & 1) << 1);
  b = nq / 6;
  const int rem = nq - 6 * b;
  q = rem >> 1;
  r = 2 * P + (rem & 1);
  e8 = pos & 3;
}
template <int EXT>
X3_HD int ks_addr(int r, int b, int q, int e8) {
  const int P = r >> 1;
  return P * (EXT / 32 * 384) + ((((6 * b + 2 * q + (r & 1)) ^ ((P & 1) << 1)) << 2) + e8) * 16;
}

// ---- fragment reads: two per-lane byte offsets per operand, everything else an immediate ----
// k-contiguous (ds_read_b128): lane (i = lane & 31, kb = lane >> 5) reads row 32 * frag + i, k-chunk 2 ks + kb of plane q at
//   kc_lane_off(lane, frag0, ks) + kc_imm(f, q),  frag = frag0 + f
X3_HD int kc_lane_off(int lane, int frag0, int ks) { return kc_addr(frag0 * 32 + (lane & 31), 0, 2 * ks + (lane >> 5)); }
X3_HD int kc_imm(int f, int q) { return f * (16 * 384) + q * 128; }
// k-strided (two ds_read_b64_tr_b16, the second `hi` four k-rows further): lane (kb, half, j, qq) = (lane >> 5, (lane >> 4) & 1,
//   (lane >> 2) & 3, lane & 3) reads 8 bytes of k-row 16 ks + 8 kb + j (+ 4), columns 32 * frag + 16 half + 4 qq .. + 3, at
//   ks_lane_off(lane, frag0, X & 1) + ks_imm(X, ks, hi),  X = 3 f + q.  The 128-byte line of (frag, q) inside a row pair is
//   Xt = 3 frag + q, stored at Xt ^ t (t = parity of the lane's row pair): Xt + t for even Xt, Xt - t for odd.
template <int EXT>
X3_HD int ks_lane_off(int lane, int frag0, int x_odd) {
  const int kb = lane >> 5, half = (lane >> 4) & 1, j = (lane >> 2) & 3, qq = lane & 3;
  const int t = (j >> 1) & 1;
  const int base = (4 * kb + (j >> 1)) * (EXT / 32 * 384) + (j & 1) * 64 + (2 * half + (qq >> 1)) * 16 + ((qq & 1) << 3) +
                   128 * 3 * frag0;
  const int xt_odd = (frag0 + x_odd) & 1;  // parity of Xt = 3 frag0 + X
  // the immediate is 128 * X for even X and 128 * (X - 1) for odd X: an odd X carries its own + 128 here
  return base + (xt_odd ? -128 * t : 128 * t) + (x_odd ? 128 : 0);
}
template <int EXT>
X3_HD int ks_imm(int X, int ks, int hi) {
  return 128 * (X & ~1) + (ks * 8 + hi * 2) * (EXT / 32 * 384);
}

// ---- tile lists of the dual (dA + dW) launch ---------------------------------------------------------------------
// The two problems of a dual launch have tiles of different LENGTH (ring tiles of 32 k: 64 for dA against 32 for dW at 1024
// frames).  With one tile per block a CU that draws short tiles runs several blocks back to back and pays block dispatch, the
// ring's ramp and the drain in front of the epilogue once per tile, exposed; so a block of the SHORT problem is given a list of
// `per` consecutive tiles of the XCD-grouped tile sequence (tile_of_block in gemm_bf16.hip) and runs them without leaving its CU,
// the ring carrying on across the tile boundary.  Blocks of the long problem keep one tile each and come first in block order.
constexpr int kXcds = 8;
constexpr int kCus = 256;
// tiles per block of the short problem: the count that brings a block's ring tiles closest to a long block's (ties go down) --
// lowered, one by one, while the grouped grid would have fewer blocks than the chip has CUs (a CU left idle costs more than a
// second ramp)
X3_HD int dual_tiles_per_block(int n_long, int nk_long, int n_short, int nk_short) {
  int per = (nk_long + (nk_short - 1) / 2) / nk_short;
  if (per < 1) per = 1;
  while (per > 1 && n_long + (n_short + per - 1) / per < kCus) --per;
  return per;
}
// Block g of the short problem's blocks runs on the XCD that all blocks with g % 8 share and takes tiles [seq0, seq0 + count) of
// that XCD's contiguous run of the tile sequence (q or q + 1 tiles, as tile_of_block deals them): consecutive sequence numbers
// walk down a column of tiles first, so the tiles of a list share an operand panel and the second finds it in that XCD's L2.
// count == 0: a block past the end of a run that is one list shorter than another XCD's (it ends at once).
X3_HD void dual_block_tiles(int n_short, int per, int g, int& seq0, int& count) {
  const int xcd = g % kXcds, j = g / kXcds;
  const int q = n_short / kXcds, r = n_short % kXcds;
  const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  const int cnt = q + (xcd < r ? 1 : 0);
  const int left = cnt - j * per;
  seq0 = start + j * per;
  count = left <= 0 ? 0 : left < per ? left : per;
}
// blocks the short problem needs: up to the last block with a tile (at most seven empty ones in front of it)
X3_HD int dual_short_blocks(int n_short, int per) {
  const int q = n_short / kXcds, r = n_short % kXcds;
  if (q == 0) return r;
  const int j_q = (q + per - 1) / per, j_q1 = (q + 1 + per - 1) / per;  // lists of a run of q / of q + 1 tiles
  return (r > 0 && j_q1 > j_q) ? kXcds * j_q + r : kXcds * j_q;
}

// ---- batch norm's backward inside the dA blocks of the dual launch (gemm_bf16.hip: EPI_DACT_BN) --------------------
// The dA blocks may do the column-tiled apply kernel's work (kernels.hip: hb_apply_kernel) on their own 128-row tile when
//   * the pass is not stacked (one segment, one pair of column means);
//   * dA is the problem with the longer K (T <= k_da), so that every dA tile has a block of its own and those blocks are the
//     lowest block ids of the grid -- dispatched first, and the rendezvous of a block column waits for one-tile blocks only;
//   * the apply kernel's blocks of `chunk_rows` rows tile the 128-row GEMM tile exactly (a chunk never straddles two tiles);
//   * the slots fit: no more row tiles than `max_tiles` per-tile partial sums are summed by the apply kernel itself
//     (kernels.h: kMergeOnceChunks; beyond that a merge kernel runs in between and the sums associate differently).
constexpr int kDualTileRows = 128;
X3_HD bool dual_bnb_eligible(int T, int chunk_rows, int k_da, bool stacked, int max_tiles) {
  if (stacked || T < 1 || chunk_rows < 1) return false;
  if (kDualTileRows % chunk_rows != 0) return false;
  if (T > k_da) return false;
  return (T + kDualTileRows - 1) / kDualTileRows <= max_tiles;
}

#if defined(__HIPCC__)
// x = p1 + p2 + p3 exactly, each a bf16, by ROUND TO NEAREST (even): p1 = RN(x), p2 = RN(x - p1), p3 = x - p1 - p2.
// Both subtractions are exact in fp32 (x - p1 keeps the low 16 bits of x's significand, sign included; the remainder after
// two planes has at most 8 significant bits and IS a bf16).  |p2| <= 2^-8 |x| and |p3| <= 2^-16 |x| -- half of what truncation
// leaves (rounds 4 / 5) -- so the three plane products the contraction drops (a2 b3, a3 b2, a3 b3) are bounded by 2^-23 |a b|
// instead of 2^-21.  The planes of one value may differ in sign.  Edges: a finite |x| above bf16's largest value (2^127 * 1.9922)
// would round to Inf: that value is split by truncation instead (the split stays exact, the bound for such a value is truncation's);
// Inf splits into (Inf, NaN, NaN) and NaN into NaNs (Inf - Inf): a non-finite operand surfaces as NaN in every result it touches.
__device__ __forceinline__ void split3(float x, uint16_t& p1, uint16_t& p2, uint16_t& p3) {
  const uint32_t ux = __builtin_bit_cast(uint32_t, x);
  uint32_t b1 = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)x) << 16;
  const bool edge = (b1 & 0x7fffffffu) == 0x7f800000u && (ux & 0x7fffffffu) < 0x7f800000u;
  if (edge) b1 = ux & 0xffff0000u;
  const float r1 = x - __builtin_bit_cast(float, b1);
  uint32_t b2 = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)r1) << 16;
  if (edge) b2 = __builtin_bit_cast(uint32_t, r1) & 0xffff0000u;  // (planes of one sign: no partial sum of them exceeds |x|)
  const float r2 = r1 - __builtin_bit_cast(float, b2);
  p1 = (uint16_t)(b1 >> 16);
  p2 = (uint16_t)(b2 >> 16);
  p3 = (uint16_t)(__builtin_bit_cast(uint32_t, r2) >> 16);
}
#endif

}  // namespace x3
}  // namespace tfk
