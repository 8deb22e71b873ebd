// GPU tool: per-block timeline of ONE dual launch (gemm_bf16x3_dual: dA + dW of a layer) -- where on the chip and when every
// block and every tile of a block's list starts, reaches its first MFMA, leaves its last one and ends.  Compiles
// tfkaldi_amd/csrc/gemm_bf16.hip with the TFKB_TL hook defined: thread 0 of a block writes wall_clock64() (100 MHz) with plain
// stores into a scratch buffer, plus HW_REG_XCC_ID / HW_REG_HW_ID at entry.  The library is built without the hook.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I tfkaldi_amd/csrc tools/ubench/x3_dual_timeline.hip -o tools/bin/x3_dual_timeline
//   tools/bin/x3_dual_timeline [frames d_in d_out [bnb | unfused]]   (default 1024 2048 2048: bench.py's hidden layer)
// bnb: the launch with EPI_DACT_BN on its dA blocks (gemm_bf16.h: BnbArgs; ReLU, batch norm's backward in the blocks' tail) -- two
// more stamps per dA block, at its arrival at the column's rendezvous and (the end stamp) behind the fused epilogue; unfused: the
// same launch made to decide UNFUSED.
// Prints, in microseconds from the first block's entry: when the blocks of the long-K problem end, and for every CU that ran
// two short-K tiles the gap between the first tile's last MFMA and the second tile's first one, the epilogue's length, and the
// end of the launch; then the launch's average time over 200 back-to-back launches (with the stamps being written).
#include <hip/hip_runtime.h>

__device__ unsigned long long* tfkb_tl_buf;
constexpr int kTlTiles = 4, kTlWords = 6;  // per block: up to 4 tiles x {entry, first MFMA, last MFMA, end, arrival (EPI_DACT_BN), where}
__device__ __forceinline__ void tfkb_tl_stamp(int ev, int ti) {
  if (threadIdx.x != 0 || ti >= kTlTiles) return;
  unsigned long long* r = tfkb_tl_buf + ((size_t)blockIdx.x * kTlTiles + ti) * kTlWords;
  r[ev] = wall_clock64();
  if (ev == 0) {
    unsigned xcc, hwid;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    // HW_ID (gfx9): cu 11:8, sh 12, se 15:13
    r[5] = 1ull | ((unsigned long long)(xcc & 15) << 8) | ((unsigned long long)((hwid >> 8) & 0xff) << 16);
  }
}
#define TFKB_TL(ev, ti) tfkb_tl_stamp(ev, ti)
#include "../../tfkaldi_amd/csrc/gemm_bf16.hip"

#include <stdio.h>
#include <algorithm>
#include <map>
#include <vector>

// planes of a split fp32 value: plane q scaled by 2^-8q, random significands and signs
static uint16_t* planes(size_t rows, int ld, unsigned seed) {
  std::vector<uint16_t> h(tfk::x3::elems(rows, ld));
  unsigned s = seed;
  for (size_t i = 0; i < h.size(); ++i) {
    s = s * 1664525u + 1013904223u;
    const int q = (int)((i % 192) / 64);
    h[i] = (uint16_t)(0x3c00u + ((s >> 9) & 0x3ffu) + ((s >> 8) & 0x8000u) - q * (8u << 7));
  }
  uint16_t* d;
  hipMalloc(&d, h.size() * 2);
  hipMemcpy(d, h.data(), h.size() * 2, hipMemcpyHostToDevice);
  return d;
}
static double med(std::vector<double> v) {
  if (v.empty()) return 0.0;
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}
static double vmax(const std::vector<double>& v) { return v.empty() ? 0.0 : *std::max_element(v.begin(), v.end()); }
static double vmin(const std::vector<double>& v) { return v.empty() ? 0.0 : *std::min_element(v.begin(), v.end()); }

int main(int argc, char** argv) {
  const int T = argc > 3 ? atoi(argv[1]) : 1024, din = argc > 3 ? atoi(argv[2]) : 2048, dout = argc > 3 ? atoi(argv[3]) : 2048;
  auto p32 = [](int n) { return (n + 31) & ~31; };
  const int ld_in = p32(din), ld_out = p32(dout);
  uint16_t* dz = planes(T, ld_out, 1u);
  uint16_t* w = planes(din, ld_out, 2u);
  uint16_t* in = planes(T, ld_in, 3u);
  float *dA, *dW;
  hipMalloc(&dA, (size_t)T * ld_in * 4);
  hipMalloc(&dW, (size_t)din * ld_out * 4);
  tfk::GemmArgsB a = {}, g = {};
  a.A = dz; a.B = w; a.C = dA; a.M = T; a.N = din; a.K = dout; a.lda = ld_out; a.ldb = ld_out; a.ldc = ld_in;
  g.A = in; g.B = dz; g.C = dW; g.M = din; g.N = dout; g.K = T; g.lda = ld_in; g.ldb = ld_out; g.ldc = ld_out;
  const int ta = ((T + 127) / 128) * ((din + 127) / 128), tw = ((din + 127) / 128) * ((dout + 127) / 128);
  const int max_blocks = ta + tw;  // (a launch of tile lists has fewer)
  const bool tn_first = g.K > a.K;
  const int n_long = tn_first ? tw : ta;
  const size_t words = (size_t)max_blocks * kTlTiles * kTlWords;
  unsigned long long* buf;
  hipMalloc(&buf, words * 8);
  hipMemset(buf, 0, words * 8);
  hipMemcpyToSymbol(HIP_SYMBOL(tfkb_tl_buf), &buf, sizeof(buf));
  // bnb / unfused: the operands of the fused epilogue (zeros: a ReLU layer that passed nothing -- the timing does not depend on it)
  const int bnb = argc > 4 ? (argv[4][0] == 'b' ? 1 : 2) : 0;
  tfk::BnbArgs bn = {};
  if (bnb) {
    auto zeros = [](size_t bytes) { void* q; hipMalloc(&q, bytes); hipMemset(q, 0, bytes); return q; };
    a.act_a = (const float*)zeros((size_t)T * ld_in * 4);
    a.act_z = (const float*)zeros((size_t)T * ld_in * 4);
    a.act_mean = (const float*)zeros((size_t)ld_in * 4);
    a.act_rstd = (const float*)zeros((size_t)ld_in * 4);
    a.stats = (float*)zeros((size_t)3 * 256 * ld_in * 4);
    a.stats_stride = 256;
    a.err = (unsigned*)zeros(4);  // (where a rendezvous that ran out of time would say so: no fused launch without it)
    a.act_nonlin = 0;
    a.epi = tfk::EPI_DACT_BN;
    bn.words = (unsigned*)zeros(tfk::kBnbWords * 4);
    bn.force_unfused = bnb == 2;
    bn.rows_per = 32;
    bn.rs = (T + 31) / 32;
    bn.nt = 3;
    bn.twin = (uint16_t*)zeros(tfk::x3::elems((size_t)T, ld_in) * 2);
    bn.ld_twin = ld_in;
  }
  auto launch = [&]() {
    if (!bnb) return tfk::gemm_bf16x3_dual(a, g, 0);
    ++bn.gen;
    return tfk::gemm_bf16x3_dual_bnb(a, g, bn, 32, 0);
  };
  for (int i = 0; i < 50; ++i)
    if (launch() != 0) { printf("dual launch not eligible\n"); return 1; }
  hipDeviceSynchronize();
  hipMemset(buf, 0, words * 8);
  launch();
  if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
  std::vector<unsigned long long> h(words);
  hipMemcpy(h.data(), buf, words * 8, hipMemcpyDeviceToHost);

  struct Rec { int block, ti; double t[5]; };
  unsigned long long t0 = ~0ull;
  for (size_t r = 0; r < words; r += kTlWords)
    if (h[r + 5]) t0 = std::min(t0, h[r]);
  std::map<unsigned long long, std::vector<Rec>> by_cu;  // short-problem tiles per CU
  std::vector<double> long_entry, long_first, long_last, long_end, all_end, short_entry, long_arrive;
  int n_blocks = 0, n_tiles = 0;
  for (int b = 0; b < max_blocks; ++b)
    for (int ti = 0; ti < kTlTiles; ++ti) {
      const unsigned long long* r = &h[((size_t)b * kTlTiles + ti) * kTlWords];
      const unsigned long long where = h[((size_t)b * kTlTiles) * kTlWords + 5];  // (a list's later tiles: the block's CU)
      if (!r[0]) continue;
      Rec rec = {b, ti, {0, 0, 0, 0, 0}};
      for (int e = 0; e < 5; ++e) rec.t[e] = r[e] ? (double)(r[e] - t0) * 0.01 : 0.0;  // 100 MHz -> us
      n_tiles++;
      if (ti == 0) n_blocks++;
      all_end.push_back(rec.t[3]);
      if (b < n_long) {
        long_entry.push_back(rec.t[0]); long_first.push_back(rec.t[1]); long_last.push_back(rec.t[2]); long_end.push_back(rec.t[3]);
        if (r[4]) long_arrive.push_back(rec.t[4]);
      } else {
        if (ti == 0) short_entry.push_back(rec.t[0]);
        by_cu[where].push_back(rec);
      }
    }
  printf("# dual launch, frames %d, %d x %d: %d blocks, %d tiles (long-K problem: %d blocks of %d ring tiles; short-K: %d tiles of %d)\n", T,
         din, dout, n_blocks, n_tiles, n_long, ((tn_first ? g.K : a.K) + 31) / 32, n_tiles - n_long, ((tn_first ? a.K : g.K) + 31) / 32);
  printf("# microseconds from the first block's entry; median [min .. max]\n");
  printf("long-K blocks : entry %6.2f [%6.2f .. %6.2f]  first MFMA %6.2f  last MFMA %6.2f  end %6.2f [%6.2f .. %6.2f]\n", med(long_entry),
         vmin(long_entry), vmax(long_entry), med(long_first), med(long_last), med(long_end), vmin(long_end), vmax(long_end));
  if (!long_arrive.empty())  // (EPI_DACT_BN, decided FUSED: no arrival stamp otherwise)
    printf("long-K blocks : arrival at the rendezvous %6.2f [%6.2f .. %6.2f]; last MFMA -> arrival %6.2f, arrival -> end %6.2f (medians)\n",
           med(long_arrive), vmin(long_arrive), vmax(long_arrive), med(long_arrive) - med(long_last), med(long_end) - med(long_arrive));
  std::vector<double> ramp1, gap, epi1, epi2, end2, first_end, cus_tiles;
  for (auto& kv : by_cu) {
    auto& v = kv.second;
    std::sort(v.begin(), v.end(), [](const Rec& x, const Rec& y) { return x.t[0] < y.t[0]; });
    cus_tiles.push_back((double)v.size());
    ramp1.push_back(v[0].t[1] - v[0].t[0]);
    for (size_t k = 0; k < v.size(); ++k) (k + 1 < v.size() ? epi1 : epi2).push_back(v[k].t[3] - v[k].t[2]);
    for (size_t k = 1; k < v.size(); ++k) gap.push_back(v[k].t[1] - v[k - 1].t[2]);
    first_end.push_back(v[0].t[3]);
    end2.push_back(v.back().t[3]);
  }
  printf("short-K tiles : on %zu CUs, %.0f .. %.0f tiles per CU; first block's entry %6.2f [%6.2f .. %6.2f]\n", by_cu.size(), vmin(cus_tiles),
         vmax(cus_tiles), med(short_entry), vmin(short_entry), vmax(short_entry));
  printf("  entry -> first MFMA of a CU's first tile        %6.2f [%6.2f .. %6.2f]\n", med(ramp1), vmin(ramp1), vmax(ramp1));
  printf("  last MFMA of a tile -> first MFMA of the next   %6.2f [%6.2f .. %6.2f]   (%zu tile changes)\n", med(gap), vmin(gap), vmax(gap),
         gap.size());
  printf("  epilogue (last MFMA -> end), tile with a successor %6.2f [%6.2f .. %6.2f], a CU's last tile %6.2f [%6.2f .. %6.2f]\n", med(epi1),
         vmin(epi1), vmax(epi1), med(epi2), vmin(epi2), vmax(epi2));
  printf("  a CU's last short-K tile ends                   %6.2f [%6.2f .. %6.2f]\n", med(end2), vmin(end2), vmax(end2));
  printf("launch ends (last block's end stamp)              %6.2f;  long-K CUs idle for %6.2f (median) before it\n", vmax(all_end),
         vmax(all_end) - med(long_end));

  hipEvent_t e0, e1;
  hipEventCreate(&e0); hipEventCreate(&e1);
  const int iters = 200;
  hipEventRecord(e0, 0);
  for (int i = 0; i < iters; ++i) launch();
  hipEventRecord(e1, 0);
  hipEventSynchronize(e1);
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  printf("average of %d back-to-back launches: %.1f us\n", iters, ms / iters * 1e3);
  return 0;
}
