// CTC loss and its gradient w.r.t. the logits, gfx950 (wave64).  See ctc.h for what it restates.
//
//   ctc_softmax      one block per frame: softmax row (kept for the gradient) and its log-sum-exp
//   ctc_gather       log p_t(state) for the 2S+1 states of the frame's utterance, contiguous per frame; a WILDCARD gap
//                    (CtcBatch::wild) gets -wild_cost instead -- the sweeps below read this table and stay as they are
//   ctc_alpha_beta   ONE WAVE PER UTTERANCE: every lane owns R consecutive states in registers, the s-1 / s-2
//                    neighbours of a lane's first states come from the previous lane by DPP wave shifts -- the time
//                    recursion runs without LDS and without barriers.  The forward sweep (alpha, loss) and the
//                    backward sweep (beta) of an utterance are two independent waves of one launch
//   ctc_grad         one wave per frame: state posteriors from alpha, beta and log Z, folded onto the classes in
//                    LABEL ORDER (repeated labels
//                    and the S+1 blanks are summed in a fixed order, so the result is bitwise reproducible); with
//                    wildcard gaps their posterior mass W_t scales the softmax row by 1 - W_t and pulls on no class
//   ctc_viterbi      forced alignment, ONE WAVE PER UTTERANCE: the max-plus twin of the forward sweep on the raw logits
//                    with 2-bit back-pointers, then the backtrace over back-pointer rows staged 64 frames at a time in LDS
//                    (ctc_row_lse supplies the rows' log-sum-exps for the score)
//   ctc_score        N-best rescoring, ONE WAVE PER (utterance, hypothesis) PAIR: the forward sweep again, gathering the
//                    logits itself as ctc_viterbi does and storing nothing per frame; out: log p(labels | x) per pair
//   ctc_viterbi_wild alignment with WILDCARD GAPS, one wave per utterance: ctc_viterbi's twin whose flagged gap states emit
//                    the row maximum (ctc_row_max_lse supplies it beside the log-sum-exp, ctc_free_score sums the two)
//   ctc_spot         keyword spotting, ONE WAVE PER (utterance, pattern) PAIR: the same recursion storing nothing per frame,
//                    the path's start frame travelling beside every state value; out: score, start, end per pair
// Log space, fp32, with a large finite "minus infinity" so that no inf - inf can arise.
#include "ctc.h"

#include <math.h>
#include <string.h>

namespace tfk {
namespace {

constexpr float NEG = -1e30f;

// log(e^a + e^b + e^c) on the hardware exp2 / log2 units: the arguments are <= 0 and the sum lies in [1, 3], where
// v_exp_f32 / v_log_f32 are good to ~1 ulp -- the recursion is a chain of Tn dependent evaluations of this on ONE
// wave, so its instruction count is the kernel's run time
// The largest argument contributes e^0 = 1 exactly, so only the other two (v_min3 / v_med3) go through v_exp_f32:
// 2 exp + 1 log per evaluation instead of 3 + 1.
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  const float lo = fminf(a, fminf(b, c));
  const float mid = __builtin_amdgcn_fmed3f(a, b, c);
  return m + __logf(1.f + __expf(mid - m) + __expf(lo - m));
}
// value of the previous / next lane (wave64 shift by one lane as a DPP move, no LDS round trip); the lane shifted
// in at the end gets `fill`
__device__ __forceinline__ float lane_prev(float v, float fill, int lane) {
  const int r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  return lane == 0 ? fill : __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float lane_next(float v, float fill, int lane) {
  const int r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
  return lane == 63 ? fill : __builtin_bit_cast(float, r);
}
// maximum over the wave, identical in every lane: quad swaps and row rotations as DPP modifiers, then the four
// 16-lane rows through v_readlane
__device__ __forceinline__ float wave_max(float x) {
#define TFK_DPP(v, ctrl) \
  __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), (ctrl), 0xf, 0xf, false))
  x = fmaxf(x, TFK_DPP(x, 0xB1));   // quad_perm [1,0,3,2]
  x = fmaxf(x, TFK_DPP(x, 0x4E));   // quad_perm [2,3,0,1]
  x = fmaxf(x, TFK_DPP(x, 0x124));  // row_ror:4
  x = fmaxf(x, TFK_DPP(x, 0x128));  // row_ror:8
#undef TFK_DPP
  const int xi = __builtin_bit_cast(int, x);
  return fmaxf(fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 0)),
                     __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 16))),
               fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 32)),
                     __builtin_bit_cast(float, __builtin_amdgcn_readlane(xi, 48))));
}
__device__ __forceinline__ uint16_t to_bf16(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }

// utterance of frame t: largest u with seg[u] <= t
__device__ __forceinline__ int utt_of(const int32_t* __restrict__ seg, int U, int t) {
  int lo = 0, hi = U;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256)
ctc_softmax_kernel(const float* __restrict__ logits, int O, int ld, float* __restrict__ post, float* __restrict__ lse) {
  __shared__ float sm[8];
  const int row = blockIdx.x;
  const float* zr = logits + (size_t)row * ld;
  float* pr = post + (size_t)row * ld;
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < O; c += 256) mx = fmaxf(mx, zr[c]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  float se = 0.f;
  for (int c = threadIdx.x; c < O; c += 256) se += expf(zr[c] - mx);
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
  if ((threadIdx.x & 63) == 0) sm[4 + (threadIdx.x >> 6)] = se;
  __syncthreads();
  se = (sm[4] + sm[5]) + (sm[6] + sm[7]);
  const float inv = 1.f / se;
  for (int c = threadIdx.x; c < ld; c += 256) pr[c] = c < O ? expf(zr[c] - mx) * inv : 0.f;
  if (threadIdx.x == 0) lse[row] = mx + logf(se);
}

// WILD: b.wild is set (the plain instantiation is the kernel as it was before the wildcards came)
template <bool WILD>
__global__ void __launch_bounds__(256)
ctc_gather_kernel(CtcBatch b) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)b.T * b.sext) return;
  const int t = (int)(idx / b.sext), s = (int)(idx % b.sext);
  const int u = utt_of(b.seg, b.U, t);
  const int l0 = b.lab_off[u], n = 2 * (b.lab_off[u + 1] - l0) + 1;
  float v = NEG;
  if (s < n) {
    const int k = (s & 1) ? b.labels[l0 + (s >> 1)] : b.O - 1;
    v = b.logits[(size_t)t * b.ld + k] - b.lse[t];
    // a wildcard gap emits exp(-wild_cost) whatever the frame holds (a finite value: no new inf arithmetic downstream)
    if (WILD && !(s & 1) && b.wild[l0 + u + (s >> 1)]) v = -b.wild_cost;
  }
  b.lp[idx] = v;
}

template <int R>
__global__ void __launch_bounds__(64)
ctc_alpha_beta_kernel(CtcBatch b) {
  // blockIdx.y = 0: the forward variables and the loss; 1 (gradient only): the backward variables.  The two sweeps
  // need nothing from each other -- only the state posteriors do, and ctc_grad forms those -- so they run as two
  // independent waves and the chain of Tn dependent steps is paid once, not twice.
  const int u = blockIdx.x, lane = threadIdx.x;
  const bool backward_sweep = blockIdx.y != 0;
  const int r0 = b.seg[u], Tn = b.seg[u + 1] - r0;
  const int l0 = b.lab_off[u], S = b.lab_off[u + 1] - l0, n = 2 * S + 1;
  if (Tn <= 0) {  // an utterance without frames: only the empty labelling is possible
    if (lane == 0 && !backward_sweep) {
      b.utt_loss[u] = S == 0 ? 0.f : INFINITY;
      b.logz[u] = 0.0;
    }
    return;
  }
  const int s0 = lane * R;
  // transitions: `skip_in[r]`  s-2 -> s allowed (s is a label state whose label differs from the previous label)
  //              `skip_out[r]` s -> s+2 allowed (the same test for state s+2)
  bool skip_in[R], skip_out[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int s = s0 + r, j = s >> 1;
    const bool lab = (s & 1) && s < n;
    skip_in[r] = lab && j >= 1 && b.labels[l0 + j] != b.labels[l0 + j - 1];
    skip_out[r] = lab && j + 1 < S && b.labels[l0 + j + 1] != b.labels[l0 + j];
  }
  const float* lp = b.lp + (size_t)r0 * b.sext + s0;
  // The recursion is a chain of Tn dependent steps of ~100 cycles each, while a row of lp takes ~1000 cycles to
  // arrive: PFD rows are kept in flight in a register ring.  The ring is advanced with clamped row indices instead
  // of guards (a surplus step re-does the last row with the state held), so the unrolled body has no branches and
  // the compiler's wait counts stay exact.
  // Precision: log p of a long utterance runs into the thousands, where fp32 resolves only ~1e-4.  The state
  // vector is therefore kept RELATIVE to an offset: once per PFD steps its maximum is moved into `off` (double,
  // wave-uniform; stored per frame), so the per-state values stay small and exact to ~1e-6 whatever Tn is.
  constexpr int PFD = 8;
  float pre[PFD][R];
  double off = 0.0;
  if (!backward_sweep) {
    float* al = b.ab + (size_t)r0 * b.sext + s0;
    double* offs = b.off + r0;
    float a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float v = lp[r];
      a[r] = (s0 + r < 2 && s0 + r < n) ? v : NEG;
      al[r] = a[r];
    }
    if (lane == 0) offs[0] = 0.0;
#pragma unroll
    for (int j = 0; j < PFD; ++j)
#pragma unroll
      for (int r = 0; r < R; ++r) pre[j][r] = lp[(size_t)min(1 + j, Tn - 1) * b.sext + r];
    for (int t0 = 1; t0 < Tn; t0 += PFD) {
#pragma unroll
      for (int j = 0; j < PFD; ++j) {
        const int t = t0 + j;
        const bool live = t < Tn;
        const int row = min(t, Tn - 1);
        float cur[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          cur[r] = pre[j][r];
          pre[j][r] = lp[(size_t)min(t + PFD, Tn - 1) * b.sext + r];
        }
        const float up1 = lane_prev(a[R - 1], NEG, lane), up2 = lane_prev(a[R - 2], NEG, lane);
        float na[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float p1 = r >= 1 ? a[r - 1] : up1;
          const float p2 = r >= 2 ? a[r - 2] : (r == 1 ? up1 : up2);
          const float v = (s0 + r < n) ? lse3(a[r], p1, skip_in[r] ? p2 : NEG) + cur[r] : NEG;
          na[r] = live ? v : a[r];
        }
        if (j == PFD - 1) {  // compile-time: re-centre the state vector on its maximum
          float m = NEG;
#pragma unroll
          for (int r = 0; r < R; ++r) m = fmaxf(m, na[r]);
          m = wave_max(m);
          if (live && m > -1e29f) {
            off += (double)m;
#pragma unroll
            for (int r = 0; r < R; ++r) na[r] = fmaxf(na[r] - m, NEG);
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          a[r] = na[r];
          al[(size_t)row * b.sext + r] = a[r];
        }
        if (lane == 0 && live) offs[t] = off;
      }
    }
    // log p(labels) = alpha_T(n-1) (+) alpha_T(n-2)
    float m = NEG;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (s0 + r == n - 1 || s0 + r == n - 2) m = fmaxf(m, a[r]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float se = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (s0 + r == n - 1 || s0 + r == n - 2) se += expf(a[r] - m);
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    const float log_z_rel = m + logf(se);  // relative to the final offset
    const bool feasible = log_z_rel > -1e29f;
    const double log_z = off + (double)log_z_rel;
    if (lane == 0) {
      b.utt_loss[u] = feasible ? (float)-log_z : INFINITY;
      b.logz[u] = log_z;
    }
    return;
  }
  // backward variables beta~_t(s) (emission of frame t included), relative to their own offsets
  float* be = b.bb + (size_t)r0 * b.sext + s0;
  double* offs = b.offb + r0;
  float bt[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int s = s0 + r;
    bt[r] = (s == n - 1 || s == n - 2) ? lp[(size_t)(Tn - 1) * b.sext + r] : NEG;
    be[(size_t)(Tn - 1) * b.sext + r] = bt[r];
  }
  if (lane == 0) offs[Tn - 1] = 0.0;
#pragma unroll
  for (int j = 0; j < PFD; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) pre[j][r] = lp[(size_t)max(Tn - 2 - j, 0) * b.sext + r];
  for (int t0 = Tn - 2; t0 >= 0; t0 -= PFD) {
#pragma unroll
    for (int j = 0; j < PFD; ++j) {
      const int t = t0 - j;
      const bool live = t >= 0;
      const int row = max(t, 0);
      float cur[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        cur[r] = pre[j][r];
        pre[j][r] = lp[(size_t)max(t - PFD, 0) * b.sext + r];
      }
      const float dn1 = lane_next(bt[0], NEG, lane), dn2 = lane_next(bt[1], NEG, lane);
      float nb[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float q1 = r + 1 < R ? bt[r + 1] : dn1;
        const float q2 = r + 2 < R ? bt[r + 2] : (r + 1 < R ? dn1 : dn2);
        const float v = (s0 + r < n) ? lse3(bt[r], q1, skip_out[r] ? q2 : NEG) + cur[r] : NEG;
        nb[r] = live ? v : bt[r];
      }
      if (j == PFD - 1) {  // re-centre beta
        float m = NEG;
#pragma unroll
        for (int r = 0; r < R; ++r) m = fmaxf(m, nb[r]);
        m = wave_max(m);
        if (live && m > -1e29f) {
          off += (double)m;
#pragma unroll
          for (int r = 0; r < R; ++r) nb[r] = fmaxf(nb[r] - m, NEG);
        }
      }
      // (a surplus step holds the state and rewrites row 0 with the value it already has)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        bt[r] = nb[r];
        be[(size_t)row * b.sext + r] = bt[r];
      }
      if (lane == 0 && live) offs[t] = off;
    }
  }
}

// one wave per frame; dynamic LDS: the class row, then the frame's state posteriors
//   gamma_t(s) = exp((alpha~ + beta~ - lp) + (off_alpha(t) + off_beta(t) - log Z))
// (the exponent is summed in double and rounded once), then divided by its sum over the frame's states where
// that sum is one up to round-off
// WILD (b.wild is set): a wildcard gap's emission does not depend on the logits, so its posterior pulls on no class and the
// softmax row keeps only the mass of the other states: row <- softmax * (1 - W_t) - the label and blank-gap posteriors, with
// W_t = the posteriors of the frame's wildcard gaps, summed beside the blank sum in the same fixed order.  With no flag set
// W_t = 0.f, softmax * 1.f is exact and the blank sum adds the same terms: the plain kernel's bits.
// A flag array that is NULL counts as all zero.  dlogits has row stride ldd, columns [b.ld, ldd) are written as zero.
// One body for the two kernels below; ctc_grad_kernel's compiled form is the one it had before the wildcards came.
template <bool WILD>
__device__ __forceinline__ void ctc_grad_frame(const CtcBatch& b, float* __restrict__ dlogits, int ldd, int t, const Twin& tw) {
  extern __shared__ float row[];
  float* g = row + b.ld;
  const int lane = threadIdx.x;
  const int u = utt_of(b.seg, b.U, t);
  const int l0 = b.lab_off[u], S = b.lab_off[u + 1] - l0, n = 2 * S + 1;
  const bool live = b.utt_loss[u] < INFINITY;
  const float* pr = b.post + (size_t)t * b.ld;
  for (int c = lane; c < b.ld; c += 64) row[c] = live ? pr[c] : 0.f;
  {
    // (summed in double: between two re-centrings alpha~ and beta~ of a peaky model fall to ~ -200, where an fp32 sum
    // rounds by 1.5e-5 per state)
    const double shift = live ? b.off[t] + b.offb[t] - b.logz[u] : 0.0;
    const float* al = b.ab + (size_t)t * b.sext;
    const float* be = b.bb + (size_t)t * b.sext;
    const float* lp = b.lp + (size_t)t * b.sext;
    float tot = 0.f;
    for (int s = lane; s < n; s += 64) {
      g[s] = live ? __expf((float)((double)al[s] + (double)be[s] - (double)lp[s] + shift)) : 0.f;
      tot += g[s];
    }
    // sum_s gamma_t(s) = 1 at every frame.  alpha~ and beta~ each carry the round-off of a chain of up to Tn fp32 steps,
    // and the part of it that the frame's states share shows as a sum of 1 +- 1e-5 .. 1e-4: divide it out, so that a
    // row of dLogits sums to zero as far as the softmax row does (fixed order: lane-strided sums, then the butterfly).
    // The trade: whatever the frame's states share -- off, offb, log Z -- cancels in the quotient, so the division
    // would also hide a wrong offset or a wrong log Z from every check of the gradient.  It is therefore applied only
    // where the sum is within 1e-2 of one, >10x the round-off of the longest utterances (1600 frames) and far
    // below what a wrong offset gives (a re-centring moves the offset by tens; e^+-20).  Outside of that band the
    // posteriors stay as computed -- a sum that overflowed included, so no inf * 0 can arise -- and the error shows
    // in dLogits at its full size.
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    const float inv = fabsf(tot - 1.f) < 1e-2f ? 1.f / tot : 1.f;
    for (int s = lane; s < n; s += 64) g[s] *= inv;
  }
  __syncthreads();
  float blank = 0.f;
  if constexpr (WILD) {
    const uint8_t* w = b.wild ? b.wild + l0 + u : nullptr;
    float wsum = 0.f;
    for (int s = 2 * lane; s < n; s += 128) {
      const bool f = w && w[s >> 1] != 0;
      blank += f ? 0.f : g[s];
      wsum += f ? g[s] : 0.f;
    }
    for (int o = 32; o > 0; o >>= 1) blank += __shfl_xor(blank, o);
    for (int o = 32; o > 0; o >>= 1) wsum += __shfl_xor(wsum, o);
    const float keep = 1.f - wsum;
    for (int c = lane; c < b.ld; c += 64) row[c] *= keep;  // (the elements this lane loaded itself)
    __syncthreads();
  } else {
    for (int s = 2 * lane; s < n; s += 128) blank += g[s];
    for (int o = 32; o > 0; o >>= 1) blank += __shfl_xor(blank, o);
  }
  if (lane == 0 && live) {
    row[b.O - 1] -= blank;
    for (int j = 0; j < S; ++j) row[b.labels[l0 + j]] -= g[2 * j + 1];  // label order: deterministic for repeats
  }
  __syncthreads();
  float* dr = dlogits + (size_t)t * ldd;
  for (int c = lane; c < ldd; c += 64) dr[c] = c < b.ld ? row[c] : 0.f;
  if (tw.p)
    for (int c = lane; c < b.ld; c += 64) twin_put(tw, (size_t)t, c, row[c]);
}
__global__ void __launch_bounds__(64)
ctc_grad_kernel(CtcBatch b, float* __restrict__ dlogits, Twin tw) {
  ctc_grad_frame<false>(b, dlogits, b.ld, blockIdx.x, tw);
}
// the launch covers rows [row0, row0 + gridDim.x)
__global__ void __launch_bounds__(64)
ctc_grad_wild_kernel(CtcBatch b, float* __restrict__ dlogits, int ldd, int row0, Twin tw) {
  ctc_grad_frame<true>(b, dlogits, ldd, row0 + blockIdx.x, tw);
}

__global__ void __launch_bounds__(256)
ctc_loss_reduce_kernel(const float* __restrict__ utt_loss, const int32_t* __restrict__ lab_off, int U,
                       float* __restrict__ scalars, int overwrite) {
  __shared__ float sm[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < U; i += 256) s += utt_loss[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    const float labels = (float)(lab_off[U] - lab_off[0]);
    scalars[0] = overwrite ? s : scalars[0] + s;
    scalars[1] = overwrite ? labels : scalars[1] + labels;
    scalars[2] = overwrite ? 1.f : scalars[2] + 1.f;
  }
}

int regs_for(int max_labels) {
  const int n = 2 * max_labels + 1;
  int r = 2;
  while (64 * r < n) r *= 2;
  return r;
}

// ---- best-path decoding and label edit distance (tf.nn.ctc_greedy_decoder + tf.edit_distance) ----

__device__ __forceinline__ int lane_prev_i(int v, int fill, int lane) {
  const int r = __builtin_amdgcn_update_dpp(0, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  return lane == 0 ? fill : r;
}
// does (v, i) win against (bv, bi)?  Larger value; on ties the lower class (TF's row max); a NaN loses to every number
// (and, between NaNs, the lower class wins: a row of NaNs decodes as class 0)
__device__ __forceinline__ bool beats(float v, int i, float bv, int bi) {
  if (v > bv) return true;
  if (v < bv) return false;
  const bool vn = __builtin_isnan(v), bn = __builtin_isnan(bv);
  if (vn != bn) return bn;
  return i < bi;
}

// one wave per row: cls[t] = the winning class of logits row t.  One read of T x O floats.
__global__ void __launch_bounds__(256)
ctc_row_argmax_kernel(const float* __restrict__ logits, int ld, int O, int T, int32_t* __restrict__ cls) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* z = logits + (size_t)row * ld;
  float bv = __builtin_nanf("");
  int bi = 0x7fffffff;  // (NaN, beyond every class): loses to any element
  for (int c = lane; c < O; c += 64) {
    const float v = z[c];
    if (beats(v, c, bv, bi)) { bv = v; bi = c; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if (lane == 0) cls[row] = bi;
}

// ONE WAVE PER UTTERANCE: the frame's class and its predecessor's (a DPP shift; the last class of the previous 64-frame
// chunk is carried in) give the emit mask k != blank && k != k_prev by ballot; a label's output row is the count so far
// plus the emitting lanes below it (mbcnt).  hyp[seg[u] + n] = n-th label, -1 on the utterance's remaining rows.
__global__ void __launch_bounds__(64)
ctc_merge_kernel(const int32_t* __restrict__ cls, const int32_t* __restrict__ seg, int blank, int32_t* __restrict__ hyp,
                 int32_t* __restrict__ hyp_len) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const int r0 = seg[u], Tn = seg[u + 1] - r0;
  int carry = -1;  // class of the frame before the chunk: none before the first
  int n = 0;       // labels emitted so far (wave-uniform)
  for (int f0 = 0; f0 < Tn; f0 += 64) {
    const int f = f0 + lane;
    const int k = f < Tn ? cls[r0 + f] : blank;
    const int prev = lane_prev_i(k, carry, lane);
    const bool emit = k != blank && k != prev;
    const uint64_t m = __ballot(emit);
    const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (emit) hyp[r0 + n + below] = k;  // n + below <= f < Tn
    n += __popcll(m);
    carry = __builtin_amdgcn_readlane(k, 63);
  }
  for (int f = n + lane; f < Tn; f += 64) hyp[r0 + f] = -1;
  if (lane == 0) hyp_len[u] = n;
}

// Levenshtein distance D[H][S] (unit costs) of hyp[0, H) and ref[0, S): ONE WAVE PER PAIR, systolic over the
// anti-diagonals.  Lane k owns the R reference columns j = kR+1 .. kR+R in registers (prev[r] = D[i-1][j], the row above)
// and computes row i = s - k at step s.  The left boundary D[i][kR] and the hypothesis token h[i-1] are what lane k-1
// produced / used at step s-1, moved one lane up by DPP; the diagonal D[i-1][kR] is the boundary that arrived at step s-1.
// Lane 0 takes D[i][0] = i and its token from a 64-token register window (prefetched one window ahead).
// Bound: H + ceil(S / R) - 1 dependent steps of 2 DPP moves + ~3R + 8 VALU ops each -- no LDS, no barrier, one read of
// both sequences.  A pair with a negative length or a reference longer than min(64 R, kCtcMaxLabels) gets -1.
template <int R>
__global__ void __launch_bounds__(64)
edit_distance_kernel(const int32_t* __restrict__ hyp, const int32_t* __restrict__ hyp_off,
                     const int32_t* __restrict__ hyp_cnt, const int32_t* __restrict__ ref,
                     const int32_t* __restrict__ ref_off, int32_t* __restrict__ dist) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const int h0 = hyp_off[u], H = hyp_cnt ? hyp_cnt[u] : hyp_off[u + 1] - h0;
  const int g0 = ref_off[u], S = ref_off[u + 1] - g0;
  if (H < 0 || S < 0 || S > 64 * R || S > kCtcMaxLabels) {
    if (lane == 0) dist[u] = -1;
    return;
  }
  if (H == 0 || S == 0) {
    if (lane == 0) dist[u] = H + S;
    return;
  }
  const int c0 = lane * R;           // the lane's first column is j = c0 + 1
  const int steps = H + (S + R - 1) / R - 1;
  int rf[R], prev[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    rf[r] = c0 + r < S ? ref[g0 + c0 + r] : -1;  // (columns beyond S never reach D[H][S])
    prev[r] = c0 + r + 1;                        // D[0][j] = j
  }
  int out = c0 + R;      // the lane's last column in the row it holds: lane k+1's left boundary
  int tok = 0;           // the token of that row
  int left_prev = c0;    // the boundary received at the previous step: this step's diagonal
  int win = lane < H ? hyp[h0 + lane] : -1;
  int nxt = 64 + lane < H ? hyp[h0 + 64 + lane] : -1;
  for (int b = 0; 64 * b < steps; ++b) {
    for (int j = 0; j < 64; ++j) {
      const int s = 64 * b + j + 1;  // lane 0's row; its token is h[s - 1] = window lane j
      if (s > steps) break;
      const int i = s - lane;
      const int left = lane_prev_i(out, s, lane);  // lane 0: D[s][0] = s
      const int t = lane_prev_i(tok, __builtin_amdgcn_readlane(win, j), lane);
      if (i >= 1 && i <= H) {
        int l = left, d = left_prev;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int up = prev[r];
          const int v = min(min(up, l) + 1, d + (t != rf[r] ? 1 : 0));
          d = up;
          l = v;
          prev[r] = v;
        }
      }
      out = prev[R - 1];
      tok = t;
      left_prev = left;
    }
    win = nxt;
    const int q = 64 * (b + 2) + lane;
    nxt = q < H ? hyp[h0 + q] : -1;
  }
  int res = 0;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (c0 + r == S - 1) res = prev[r];
  if (lane == (S - 1) / R) dist[u] = res;
}


// ---- prefix beam search (tf.nn.ctc_beam_search_decoder, merge_repeated=False; the algorithm is stated in ctc.h) ----
//
// ONE WORKGROUP PER UTTERANCE, the beam resident in LDS (two sides, swapped per frame).  A frame step:
//   A  wave 0 turns the frame's logits (loaded one step ahead) into log-probabilities lp[c] in LDS; waves 1-2 mark, per
//      beam slot i, the labels c for which the extension (i, c) IS a prefix already in the beam (childmask)
//   B  the nb * O candidates -- (slot i, label c) = extension, (slot i, blank column) = "stay" -- are scored, a
//      contiguous run per thread; a stay candidate collects its parent's extension (at most three terms, fixed order);
//      an extension that equals a beam prefix is dead.  Keys (order-preserving uint32 of the total) go to LDS
//   C  the best W by an 8-bit radix select over the keys (4 histogram passes; integer LDS atomics, so the counts do
//      not depend on scheduling); only when the W-th and (W+1)-th key are equal, 4 more passes over the secondary key
//      (shorter prefix, then lower candidate index)
//   D  compaction in candidate order (block prefix sum), the survivors' (pb, pnb) re-centred on the best total (the
//      sum of the offsets is kept in double: the scores stay exact to ~1e-6 whatever T is); a surviving extension
//      finds or inserts its trie node
//   E  src[j] = the slot of prefix j's parent in the new beam (what A and B need at the next frame)
// The trie is an open-addressing table in global scratch keyed by (parent node, label); a node's id is its slot, so
// one label sequence has one id however often it leaves and re-enters the beam, and "extension (p, c) equals q" is
// q.parent == p.node && q.last == c.  Ids depend on the insertion order, results do not: nothing is ordered by id.
constexpr int kBeamThreads = 256;
constexpr int kBeamKeys = kCtcBeamMaxWidth * kCtcBeamMaxClasses;
constexpr int kBeamRoot = 0x7fffffff;  // node id of the empty prefix (never a table slot)
constexpr unsigned long long kTrieEmpty = ~0ull;

struct BeamSide {
  float pb[kCtcBeamMaxWidth], pnb[kCtcBeamMaxWidth], tot[kCtcBeamMaxWidth];
  int node[kCtcBeamMaxWidth], parent[kCtcBeamMaxWidth], last[kCtcBeamMaxWidth], len[kCtcBeamMaxWidth],
      src[kCtcBeamMaxWidth];
};
// with a language model every prefix also carries g = its weighted model score + label bonuses (a function of its label
// sequence alone) and ctx = its last order - 1 labels as base-O digits, the row of the table its extensions read
struct BeamSideLm : BeamSide {
  float g[kCtcBeamMaxWidth];
  int ctx[kCtcBeamMaxWidth];
};
// the model kind of a search: none (acoustic), the dense n-gram table, a deterministic graph over the labels
constexpr int kBeamAm = kCtcModelNone, kBeamNgram = kCtcModelNgram, kBeamGraph = kCtcModelGraph;
template <int LM>
struct BeamSideOf { typedef BeamSideLm type; };
template <>
struct BeamSideOf<kBeamAm> { typedef BeamSide type; };
// longest run of candidates one thread owns: ceil(kBeamKeys / kBeamThreads) | 1
constexpr int kBeamRun = ((kBeamKeys + kBeamThreads - 1) / kBeamThreads) | 1;

__device__ __forceinline__ float lae(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (!(m > -1e29f)) return NEG;
  return m + __logf(1.f + __expf(n - m));
}
// order-preserving map of a float onto uint32; 0 is kept free for "no candidate"
__device__ __forceinline__ uint32_t sortable(float x) {
  const uint32_t b = __builtin_bit_cast(uint32_t, x);
  const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return k ? k : 1u;
}
// (pb', pnb') of candidate (slot i, class c); c == blank is the stay candidate
__device__ __forceinline__ void beam_candidate(const BeamSide& b, const float* lp, int i, int c, int blank, float* pbn,
                                               float* pnbn) {
  if (c == blank) {
    const int l = b.last[i];
    *pbn = fmaxf(b.tot[i] + lp[blank], NEG);
    float v = l >= 0 ? fmaxf(b.pnb[i] + lp[l], NEG) : NEG;
    const int s = b.src[i];
    if (s >= 0) v = lae(v, fmaxf((b.last[s] == l ? b.pb[s] : b.tot[s]) + lp[l], NEG));
    *pnbn = v;
  } else {
    *pbn = NEG;
    *pnbn = fmaxf((c == b.last[i] ? b.pb[i] : b.tot[i]) + lp[c], NEG);
  }
}
// secondary key of candidate k (larger = preferred): shorter prefix, then lower candidate index
__device__ __forceinline__ uint32_t beam_tiebreak(int len, int k) {
  return ((uint32_t)(kCtcBeamMaxFrames + 1 - len) << 13) | (uint32_t)(kBeamKeys - 1 - k);
}

// g(p + c) = (g(p) + lm_weight * lm[ctx(p)][c]) + label_bonus: three roundings in this order wherever it is evaluated, so
// every route to a prefix gives the same bits
__device__ __forceinline__ float beam_lm_extend(float g, float w, float lmv, float bonus) {
#pragma clang fp contract(off)
  const float a = g + w * lmv;
  return a + bonus;
}
// the ranking value of a final prefix under TFK_CTC_LM_EOS: (tot + g) + lm_weight * lm[ctx][O - 1]
__device__ __forceinline__ float beam_lm_end(float key, float w, float lmv) {
#pragma clang fp contract(off)
  return key + w * lmv;
}

// f(q) for q in [0, cpt), cpt <= kBeamRun uniform over the wave (an SGPR): fully unrolled, so that q is a constant in every
// copy of f and a register array indexed by it stays in registers; scalar branches skip what lies beyond cpt, eight at a time
template <class F>
__device__ __forceinline__ void beam_for_run(int cpt, F f) {
#pragma unroll
  for (int q0 = 0; q0 < kBeamRun; q0 += 8)
    if (q0 < cpt) {
#pragma unroll
      for (int q = q0; q < (q0 + 8 < kBeamRun ? q0 + 8 : kBeamRun); ++q)
        if (q < cpt) f(q);
    }
}

// One wave's half of a radix pass: of the 256 bins of hist (the highest digit first) the one that holds the `need`-th key
// -> sel[0], the rank still wanted inside that bin -> sel[1], the bin's count -> sel[2]; hist is left cleared for the next pass.
__device__ __forceinline__ void radix_pick_bin(uint32_t* hist, int* sel, int need, int lane) {
  const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];  // bins 4 lane .. 4 lane + 3
  const int s = (int)(h.x + h.y + h.z + h.w);
  int incl = s;  // this lane's bins and every higher one
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_down(incl, o);
    if (lane + o < 64) incl += v;
  }
  int above = incl - s;
  const uint32_t hv[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
  for (int q = 3; q >= 0; --q) {
    const int c = (int)hv[q];
    if (need > above && need <= above + c) {
      sel[0] = 4 * lane + q;
      sel[1] = need - above;
      sel[2] = c;
    }
    above += c;
  }
  reinterpret_cast<uint4*>(hist)[lane] = make_uint4(0u, 0u, 0u, 0u);
}

// The `need`-th largest of the non-zero keys keyf(k), k in [k0, k1) over the block's threads (need <= their number):
// returns it; *take = how many candidates EQUAL to it belong to the best `need`, *have = how many there are.
template <class F>
__device__ __forceinline__ uint32_t beam_radix_select(F keyf, int k0, int k1, int need, uint32_t* hist, int* sel,
                                                      int* take, int* have) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t prefix = 0;
  int cnt = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int k = k0; k < k1; ++k) {
      const uint32_t key = keyf(k);
      if (key != 0 && (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))))
        atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) radix_pick_bin(hist, sel, need, lane);
    __syncthreads();
    prefix |= (uint32_t)sel[0] << shift;
    need = sel[1];
    cnt = sel[2];
  }
  *take = need;
  *have = cnt;
  return prefix;
}

// the model of a search as the kernels receive it: table = the n-gram table [C, O], or the graph's weight [S, O] with
// next [S, O] and start; eos = the end term counts.  The launchers build it once from CtcLm (beam_model).
struct BeamModel { const float* table; int C; float weight, bonus; int eos; const int32_t* next; int start; };

// A resumable search (the contract: tfk_ctc_stream_* in tfkaldi_hip.h).  A stream's lane keeps, in device memory of its own,
// what the frame step reads of the past: a header of kCtcStreamHdrWords words [live | nb | ndead | lm_weight | off (double) | 2
// spare] and kCtcStreamArrays arrays of W words [pb | pnb | tot | node | parent | last | len | src | g | ctx | end], end = the
// model's end term of the prefix's context, gathered when the state is saved so that reading a result needs no model.  live == 0:
// the lane has been reset and starts from beam_start's values.  The RESUME instantiations of the two kernels load that state
// in front of the unchanged frame loop and store it behind it; they neither rank nor trace back (ctc_stream_result_kernel does).
struct BeamResume {
  int32_t* hdr;    // [lanes, kCtcStreamHdrWords]
  uint32_t* arr;   // [lanes, kCtcStreamArrays, W]
  int max_frames;  // what the lane's share of the trie is sized by
};
template <int LM, class Side>
__device__ __forceinline__ void beam_resume_load(Side& b, const BeamResume& rs, int u, int W, int* s_nb, int* s_ndead,
                                                 double* off) {
  const int tid = threadIdx.x;
  const int32_t* hd = rs.hdr + (size_t)u * kCtcStreamHdrWords;
  if (!hd[0]) return;  // (uniform over the block)
  const uint32_t* a = rs.arr + (size_t)u * kCtcStreamArrays * (size_t)W;
  const int nb = hd[1];
  *off = *reinterpret_cast<const double*>(hd + 4);
  if (tid < nb) {
    b.pb[tid] = __builtin_bit_cast(float, a[tid]);
    b.pnb[tid] = __builtin_bit_cast(float, a[W + tid]);
    b.tot[tid] = __builtin_bit_cast(float, a[2 * W + tid]);
    b.node[tid] = (int)a[3 * W + tid];
    b.parent[tid] = (int)a[4 * W + tid];
    b.last[tid] = (int)a[5 * W + tid];
    b.len[tid] = (int)a[6 * W + tid];
    b.src[tid] = (int)a[7 * W + tid];
    if constexpr (LM) {
      b.g[tid] = __builtin_bit_cast(float, a[8 * W + tid]);
      b.ctx[tid] = (int)a[9 * W + tid];
    }
  }
  if (tid == 0) {  // (the thread that wrote beam_start's values)
    *s_nb = nb;
    *s_ndead = hd[2];
  }
}
template <int LM, class Side>
__device__ __forceinline__ void beam_resume_store(const Side& b, const BeamResume& rs, int u, int W, int nb, int ndead,
                                                  double off, const float* lm, int O, float lm_w) {
  const int tid = threadIdx.x;
  int32_t* hd = rs.hdr + (size_t)u * kCtcStreamHdrWords;
  uint32_t* a = rs.arr + (size_t)u * kCtcStreamArrays * (size_t)W;
  if (tid < nb) {
    a[tid] = __builtin_bit_cast(uint32_t, b.pb[tid]);
    a[W + tid] = __builtin_bit_cast(uint32_t, b.pnb[tid]);
    a[2 * W + tid] = __builtin_bit_cast(uint32_t, b.tot[tid]);
    a[3 * W + tid] = (uint32_t)b.node[tid];
    a[4 * W + tid] = (uint32_t)b.parent[tid];
    a[5 * W + tid] = (uint32_t)b.last[tid];
    a[6 * W + tid] = (uint32_t)b.len[tid];
    a[7 * W + tid] = (uint32_t)b.src[tid];
    if constexpr (LM) {
      a[8 * W + tid] = __builtin_bit_cast(uint32_t, b.g[tid]);
      a[9 * W + tid] = (uint32_t)b.ctx[tid];
      a[10 * W + tid] = __builtin_bit_cast(uint32_t, lm[(size_t)b.ctx[tid] * (size_t)O + (size_t)(O - 1)]);
    }
  }
  if (tid == 0) {
    hd[0] = 1;
    hd[1] = nb;
    hd[2] = ndead;
    hd[3] = (int32_t)__builtin_bit_cast(uint32_t, lm_w);
    *reinterpret_cast<double*>(hd + 4) = off;
  }
}

// The start of both searches: the beam is {(): (0, -inf)}, the block's LDS state cleared.  The caller's barrier follows.
// (It is the one part of the two kernels that is written once.  Shared bodies for phases B to E and for the epilogue were
// built and measured -- profiles/ctc_beam_refactor_ab.txt: every output stayed the parent's bit for bit, but each of them,
// the epilogue included, changes how the compiler lays out the frame loop, and the pruned kernel ran up to 2.6 % slower.  With
// this body alone all six instantiations compile to the parent's instruction streams.)
template <int LM, class Side>
__device__ __forceinline__ void beam_start(Side& b, int C, int gstart, uint32_t* hist, unsigned long long* childmask,
                                           int* path, int* s_nb, int* s_ndead) {
  const int tid = threadIdx.x;
  hist[tid] = 0u;
  if (tid < kCtcBeamMaxWidth) {
    childmask[tid] = 0ull;
    path[tid] = -1;
  }
  if (tid == 0) {
    b.pb[0] = 0.f; b.pnb[0] = NEG; b.tot[0] = 0.f;
    b.node[0] = kBeamRoot; b.parent[0] = -2; b.last[0] = -1; b.len[0] = 0; b.src[0] = -1;
    if constexpr (LM == kBeamGraph) { b.g[0] = 0.f; b.ctx[0] = gstart; }
    else if constexpr (LM) { b.g[0] = 0.f; b.ctx[0] = C - 1; }  // every position before the start is the digit O - 1
    *s_nb = 1;
    *s_ndead = 0;
  }
}

// LM: the search with a dense n-gram table lm [C, O] (the contract: tfk_ctc_beam_lm in tfkaldi_hip.h).  A frame's table
// values depend only on the beam (slot i reads row ctx[i]), not on the frame's logits: every thread issues the loads of its
// own run of candidates at the top of the step, into registers (a fully unrolled run of kBeamRun, cut short at the step's
// run length, which is uniform), phase A runs under them, and behind A's barrier they are parked in the thread's own
// keys[] entries, where phase B picks each one up before it writes the key over it.  A survivor's value is loaded once
// more in D, ahead of its trie probe (an atomic round trip that is on the chain anyway; the reload was not timed on its
// own).  Issuing the gathers one phase earlier, behind D's barrier of the frame before, was measured slower
// (profiles/ctc_decode_bench.txt).
//
// LM == kBeamGraph: lm is weight [S, O] and next [S, O] its transition table (the contract: tfk_ctc_graph_set in
// tfkaldi_hip.h); ctx holds the state, the empty prefix has `start`.  The gather at the top of the step is the same one and
// decides alone whether an extension exists (weight > -inf): phase B tests it before any arithmetic (0 * -inf is NaN), a
// missing arc is no candidate, and each wave's count of them travels in sel[] through the barrier that wmax[] already
// needs (sel is written again only behind the first barrier inside beam_radix_select), so that phase C's guard and the
// select's precondition see the true live count.  A merging extension is never a missing one (its child is in the beam, so
// the arc existed), hence live = N - ndead - missing.  next is read for survivors only, in D beside the weight's reload.
// RESUME: seg bounds the lanes' chunks, the trie is the stream's (a lane's share is sized by rs.max_frames, not by the chunk),
// and hyp / hyp_len / score / am_score / top_paths / eos are not read.
template <int LM, bool RESUME = false>
__global__ void __launch_bounds__(kBeamThreads)
ctc_beam_kernel(const float* __restrict__ logits, int ld, int O, const int32_t* __restrict__ seg, int U, int T, int W,
                int top_paths, unsigned long long* __restrict__ trie, int32_t* __restrict__ hyp,
                int32_t* __restrict__ hyp_len, float* __restrict__ score, const float* __restrict__ lm, int C, float lm_w,
                float lm_bonus, int eos, float* __restrict__ am_score, const int32_t* __restrict__ gnext, int gstart,
                BeamResume rs) {
  typedef typename BeamSideOf<LM>::type Side;
  __shared__ Side beam[2];
  __shared__ __attribute__((aligned(16))) uint32_t keys[kBeamKeys];
  __shared__ __attribute__((aligned(16))) uint32_t hist[256];
  __shared__ unsigned long long childmask[kCtcBeamMaxWidth];
  __shared__ float lp[kCtcBeamMaxClasses];
  __shared__ float wmax[4];
  __shared__ int wsum[4];
  __shared__ int sel[4];
  __shared__ int s_nb, s_ndead;
  __shared__ int path[kCtcBeamMaxWidth];

  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = seg[u], Tn = seg[u + 1] - r0;
  const int blank = O - 1;
  // this utterance's share of the table: load <= 1/2
  const uint32_t cap = 2u * (uint32_t)(RESUME ? rs.max_frames : Tn) * (uint32_t)W + 64u;
  unsigned long long* tab = RESUME ? trie + (unsigned long long)u * (unsigned long long)cap
                                   : trie + (2ull * (unsigned long long)r0 * (unsigned long long)W + 64ull * (unsigned long long)u);
  const uint32_t magic = (uint32_t)((0x100000000ull + (unsigned)O - 1u) / (unsigned)O);  // k / O for k < 2^13

  beam_start<LM>(beam[0], C, gstart, hist, childmask, path, &s_nb, &s_ndead);
  int cur = 0;
  double off = 0.0;  // what has been taken out of the beam's scores so far (uniform over the block)
  if constexpr (RESUME) beam_resume_load<LM>(beam[0], rs, u, W, &s_nb, &s_ndead, &off);
  float z_next = (wave == 0 && lane < O && Tn > 0) ? logits[(size_t)r0 * ld + lane] : 0.f;
  __syncthreads();

  for (int t = 0; t < Tn; ++t) {
    const Side& b = beam[cur];
    Side& nx = beam[cur ^ 1];
    const int nb = s_nb, ndead = s_ndead;
    float lmv[kBeamRun];
    if constexpr (LM) {  // this frame's table values: in flight under phase A
      const int N = nb * O, cpt = ((N + kBeamThreads - 1) / kBeamThreads) | 1;
      const int k0 = min(tid * cpt, N), k1 = min(k0 + cpt, N);
      beam_for_run(__builtin_amdgcn_readfirstlane(cpt), [&](int q) {
        const int k = k0 + q;
        lmv[q] = 0.f;
        if (k < k1) {
          const int i = (int)__umulhi((uint32_t)k, magic), c = k - i * O;
          lmv[q] = lm[(size_t)b.ctx[i] * (size_t)O + (size_t)c];
        }
      });
    }
    // A
    if (wave == 0) {
      const float z = lane < O ? z_next : -INFINITY;
      if (t + 1 < Tn && lane < O) z_next = logits[(size_t)(r0 + t + 1) * ld + lane];
      const float mx = wave_max(z);
      float se = lane < O ? expf(z - mx) : 0.f;
      for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
      if (lane < O) lp[lane] = z - (mx + logf(se));
    } else if (tid - 64 < nb) {
      const int j = tid - 64, s = b.src[j];
      if (s >= 0) atomicOr(&childmask[s], 1ull << b.last[j]);
    }
    __syncthreads();
    // B
    const int N = nb * O;
    const int cpt = ((N + kBeamThreads - 1) / kBeamThreads) | 1;  // an odd run per thread: conflict-free LDS strides
    const int k0 = min(tid * cpt, N), k1 = min(k0 + cpt, N);
    if constexpr (LM)
      beam_for_run(__builtin_amdgcn_readfirstlane(cpt), [&](int q) {
        if (k0 + q < k1) keys[k0 + q] = __builtin_bit_cast(uint32_t, lmv[q]);
      });
    float lmax = NEG;
    int missing = 0;  // (graph) this thread's extensions that have no arc
    for (int k = k0; k < k1; ++k) {
      const int i = (int)__umulhi((uint32_t)k, magic), c = k - i * O;
      float pbn, pnbn;
      beam_candidate(b, lp, i, c, blank, &pbn, &pnbn);
      bool live = c == blank || !((childmask[i] >> c) & 1ull);
      const float tot = lae(pbn, pnbn);
      float rank = tot;  // what the beam is cut by; the re-centring (lmax) stays on the acoustic part
      if constexpr (LM == kBeamGraph) {
        const float g = b.g[i], wv = __builtin_bit_cast(float, keys[k]);
        const bool arc = c == blank || wv > -INFINITY;
        missing += !arc;
        live = live && arc;
        rank = tot + (c == blank || !arc ? g : beam_lm_extend(g, lm_w, wv, lm_bonus));
      } else if constexpr (LM) {
        const float g = b.g[i];
        rank = tot + (c == blank ? g : beam_lm_extend(g, lm_w, __builtin_bit_cast(float, keys[k]), lm_bonus));
      }
      keys[k] = live ? sortable(rank) : 0u;
      if (live) lmax = fmaxf(lmax, tot);
    }
    lmax = wave_max(lmax);
    if (lane == 0) wmax[wave] = lmax;
    if constexpr (LM == kBeamGraph) {
      for (int o = 32; o > 0; o >>= 1) missing += __shfl_xor(missing, o);
      if (lane == 0) sel[wave] = missing;
    }
    __syncthreads();
    float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (!(m > -1e29f)) m = 0.f;
    int nlive = N - ndead;
    if constexpr (LM == kBeamGraph) nlive -= sel[0] + sel[1] + sel[2] + sel[3];
    // C
    uint32_t K = 0u, K2 = 0xffffffffu;  // select: key > K, or key == K and tie-break key >= K2
    if (nlive > W) {
      int take, have;
      K = beam_radix_select([&](int k) { return keys[k]; }, k0, k1, W, hist, sel, &take, &have);
      K2 = 0u;
      if (take < have) {
        int t2, h2;
        K2 = beam_radix_select(
            [&](int k) {
              const int i = (int)__umulhi((uint32_t)k, magic), c = k - i * O;
              return keys[k] == K ? beam_tiebreak(b.len[i] + (c != blank), k) : 0u;
            },
            k0, k1, take, hist, sel, &t2, &h2);
      }
    }
    // D
    int cnt = 0;
    for (int k = k0; k < k1; ++k) {
      const uint32_t key = keys[k];
      if (key > K) { ++cnt; continue; }
      if (key == K && K2 != 0xffffffffu) {
        const int i = (int)__umulhi((uint32_t)k, magic), c = k - i * O;
        cnt += beam_tiebreak(b.len[i] + (c != blank), k) >= K2;
      }
    }
    int incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int slot = incl - cnt;
    for (int w = 0; w < wave; ++w) slot += wsum[w];
    const int nb_new = min(wsum[0] + wsum[1] + wsum[2] + wsum[3], W);
    for (int k = k0; k < k1; ++k) {
      const uint32_t key = keys[k];
      const int i = (int)__umulhi((uint32_t)k, magic), c = k - i * O;
      const bool chosen = key > K || (key == K && K2 != 0xffffffffu && beam_tiebreak(b.len[i] + (c != blank), k) >= K2);
      if (!chosen) continue;
      if (slot < W) {
        float pbn, pnbn;
        beam_candidate(b, lp, i, c, blank, &pbn, &pnbn);
        pbn = fmaxf(pbn - m, NEG);
        pnbn = fmaxf(pnbn - m, NEG);
        nx.pb[slot] = pbn;
        nx.pnb[slot] = pnbn;
        nx.tot[slot] = lae(pbn, pnbn);
        if (c == blank) {
          nx.node[slot] = b.node[i]; nx.parent[slot] = b.parent[i]; nx.last[slot] = b.last[i]; nx.len[slot] = b.len[i];
          if constexpr (LM) { nx.g[slot] = b.g[i]; nx.ctx[slot] = b.ctx[i]; }
        } else {
          float lv = 0.f;
          int ns = 0;
          if constexpr (LM) lv = lm[(size_t)b.ctx[i] * (size_t)O + (size_t)c];  // issued ahead of the trie probe
          if constexpr (LM == kBeamGraph) ns = gnext[(size_t)b.ctx[i] * (size_t)O + (size_t)c];
          // find or insert (parent node, label): the slot is the node's id
          const unsigned long long nk = ((unsigned long long)(uint32_t)b.node[i] << 6) | (unsigned long long)c;
          uint32_t pos = __umulhi((uint32_t)((nk * 0x9E3779B97F4A7C15ull) >> 32), cap);
          int id = 0;
          for (uint32_t n = 0; n < cap; ++n) {
            const unsigned long long old = atomicCAS(&tab[pos], kTrieEmpty, nk);
            if (old == kTrieEmpty || old == nk) { id = (int)pos; break; }
            pos = pos + 1u == cap ? 0u : pos + 1u;
          }
          nx.node[slot] = id; nx.parent[slot] = b.node[i]; nx.last[slot] = c; nx.len[slot] = b.len[i] + 1;
          if constexpr (LM) {
            nx.g[slot] = beam_lm_extend(b.g[i], lm_w, lv, lm_bonus);
            if constexpr (LM == kBeamGraph) nx.ctx[slot] = ns;
            else nx.ctx[slot] = (int)(((uint32_t)b.ctx[i] * (uint32_t)O + (uint32_t)c) % (uint32_t)C);
          }
        }
      }
      ++slot;
    }
    if (tid == 0) {
      s_nb = nb_new;
      s_ndead = 0;
    }
    off += (double)m;
    __syncthreads();
    // E
    if (tid < kCtcBeamMaxWidth) childmask[tid] = 0ull;
    {
      int s = -1;
      if (tid < nb_new) {
        const int p = nx.parent[tid];
        for (int i = 0; i < nb_new; ++i)
          if (nx.node[i] == p) s = i;
        nx.src[tid] = s;
      }
      const int dead = __popcll(__ballot(s >= 0));
      if (lane == 0 && dead) atomicAdd(&s_ndead, dead);
    }
    cur ^= 1;
    __syncthreads();
  }

  if constexpr (RESUME) {
    beam_resume_store<LM>(beam[cur], rs, u, W, s_nb, s_ndead, off, lm, O, lm_w);
    return;
  }
  // the top_paths best of the final beam: higher total (LM: + g, + the end term under TFK_CTC_LM_EOS), then shorter, then
  // lower slot
  const Side& b = beam[cur];
  const int nb = s_nb;
  if constexpr (LM) {  // the combined values, parked in keys[] as floats
    if (tid < nb) {
      float v = b.tot[tid] + b.g[tid];
      if (eos) {
        const float fw = lm[(size_t)b.ctx[tid] * (size_t)O + (size_t)blank];
        if (LM == kBeamGraph && !(fw > -INFINITY)) v = -INFINITY;  // not final, whatever lm_weight is
        else v = beam_lm_end(v, lm_w, fw);
      }
      keys[tid] = __builtin_bit_cast(uint32_t, v);
    }
    __syncthreads();
  }
  auto final_value = [&](int i) -> float {
    if constexpr (LM) return __builtin_bit_cast(float, keys[i]);
    else return b.tot[i];
  };
  if (tid < nb) {
    const uint32_t kj = sortable(final_value(tid));
    const int lj = b.len[tid];
    int rank = 0;
    for (int i = 0; i < nb; ++i) {
      const uint32_t ki = sortable(final_value(i));
      const int li = b.len[i];
      rank += ki > kj || (ki == kj && (li < lj || (li == lj && i < tid)));
    }
    path[rank] = tid;
  }
  __syncthreads();
  for (int n = 0; n < top_paths; ++n) {
    const int j = path[n];
    const int L = j >= 0 ? min(b.len[j], Tn) : 0;
    int32_t* out = hyp + (size_t)n * T + r0;
    for (int f = L + tid; f < Tn; f += kBeamThreads) out[f] = -1;
    if (tid == 0) {
      hyp_len[(size_t)n * U + u] = L;
      const bool alive = j >= 0 && b.tot[j] > -1e29f;
      score[(size_t)n * U + u] = alive ? (float)(off + (double)final_value(j)) : -INFINITY;
      if constexpr (LM)
        if (am_score) am_score[(size_t)n * U + u] = alive ? (float)(off + (double)b.tot[j]) : -INFINITY;
    }
  }
  if (tid < top_paths && path[tid] >= 0) {  // back-trace through the parent links, labels land in forward order
    const int j = path[tid];
    int32_t* out = hyp + (size_t)tid * T + r0;
    uint32_t node = (uint32_t)b.node[j];
    for (int pos = min(b.len[j], Tn) - 1; pos >= 0 && node < cap; --pos) {
      const unsigned long long nk = __hip_atomic_load(&tab[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      out[pos] = (int32_t)(nk & 63ull);
      node = (uint32_t)(nk >> 6);
    }
  }
}

// ---- prefix beam search with per-frame label pruning (tfk_ctc_beam_topk; any output_dim up to kCtcTopkMaxClasses) ----
//
// Two launches.  ctc_row_topk_kernel, parallel over the frames and off the sequential chain, turns every row into what the
// search needs of it (kCtcTopkRowWords words): the K kept labels in ascending class order, their log-probabilities
// z - lsum, lsum = mx + logf(se) itself and the blank's log-probability.  ctc_beam_topk_kernel is the frame step of
// ctc_beam_kernel over nb * (K + 1) candidates: slot i's candidate q < K extends by the frame's q-th kept label, q == K stays.
// It is a sibling, not a third instantiation of that body: a class there is a 6-bit column of lp[] / childmask / the trie key,
// here a label is a position q in the frame's list plus a 16-bit class, and the existing code objects stay what they were.
// The two share the __device__ helpers, the start of the beam (beam_start) and the bin scan of a radix pass (radix_pick_bin,
// also the pre-pass's); the frame step and the epilogue are written in each, because every shared form of them that was
// tried moved the compiled frame loop and the pruned kernel's time (the comment at beam_start).

// ONE WAVE PER ROW (a block is one wave, so __syncthreads is a wave barrier).  The row is read from HBM once; the later
// passes (sum, the radix passes, the compaction) find it in the cache.  For O <= 64 lane c holds class c and mx / se are formed
// by the butterflies of ctc_beam_kernel's phase A: the same bits.  The K largest label logits by an 8-bit radix select over
// order-preserving keys (integer LDS atomics: the counts do not depend on scheduling); of the keys EQUAL to the K-th the
// lowest classes are taken, counted in class order during the compaction, which also leaves the labels ascending.
__global__ void __launch_bounds__(64)
ctc_row_topk_kernel(const float* __restrict__ logits, int ld, int O, int K, uint32_t* __restrict__ pre) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[256];
  __shared__ int sel[4];
  const int lane = threadIdx.x;
  const float* z = logits + (size_t)blockIdx.x * ld;
  uint32_t* out = pre + (size_t)blockIdx.x * kCtcTopkRowWords;
  const int blank = O - 1;
  float mx = -INFINITY;
  for (int c = lane; c < O; c += 64) mx = fmaxf(mx, z[c]);
  mx = wave_max(mx);
  float se = 0.f;
  for (int c = lane; c < O; c += 64) se += expf(z[c] - mx);
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
  const float lsum = mx + logf(se);
  for (int i = lane; i < 256; i += 64) hist[i] = 0u;
  __syncthreads();
  // the K-th largest key among the labels [0, blank): prefix; `need` of the keys equal to it belong to the K
  uint32_t prefix = 0;
  int need = K;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int c = lane; c < blank; c += 64) {
      const uint32_t key = sortable(z[c]);
      if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    // (the helper also leaves the bin's count in sel[2], one LDS store per pass that this kernel does not read: accepted, so
    // that the scan is one function without a switch; sel has 4 entries)
    radix_pick_bin(hist, sel, need, lane);
    __syncthreads();
    prefix |= (uint32_t)sel[0] << shift;
    need = sel[1];  // (the next pass writes sel behind its own barrier)
  }
  // compaction in class order: a label is kept if its key is above the K-th, or equals it and fewer than `need` such labels
  // lie below it
  int n = 0, ties = 0;  // kept so far, keys equal to the K-th seen so far (uniform)
  for (int c0 = 0; c0 < blank && n < K; c0 += 64) {
    const int c = c0 + lane;
    const float v = c < blank ? z[c] : 0.f;
    const uint32_t key = c < blank ? sortable(v) : 0u;
    const bool eq = key == prefix;
    const uint64_t me = __ballot(eq);
    const int eq_below = __builtin_amdgcn_mbcnt_hi((uint32_t)(me >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)me, 0u));
    const bool keep = key > prefix || (eq && ties + eq_below < need);
    const uint64_t mk = __ballot(keep);
    const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
    if (keep && n + below < K) {  // (n + below < K always holds for finite rows; the guard keeps a NaN row in bounds)
      out[n + below] = (uint32_t)c;
      out[64 + n + below] = __builtin_bit_cast(uint32_t, v - lsum);
    }
    n += __popcll(mk);
    ties += __popcll(me);
  }
  n = min(n, K);
  if (lane >= n) {  // the unused tail (and whatever a NaN row left open): no label, log-probability -inf
    out[lane] = 0x7fffffffu;
    out[64 + lane] = __builtin_bit_cast(uint32_t, NEG);
  }
  if (lane == 0) {
    out[128] = __builtin_bit_cast(uint32_t, lsum);
    out[129] = __builtin_bit_cast(uint32_t, z[blank] - lsum);
  }
}

// (pb', pnb') of the pruned search's candidates: beam_candidate's expressions with the log-probabilities handed in.
// stay: lpb = lp[blank], lpl = lp[last(i)] (the TRUE value, kept or not), merge = last(i) is kept at this frame, so its
// parent's extension exists and is collected
__device__ __forceinline__ void beam_topk_stay(const BeamSide& b, int i, float lpb, float lpl, bool merge, float* pbn,
                                               float* pnbn) {
  const int l = b.last[i];
  *pbn = fmaxf(b.tot[i] + lpb, NEG);
  float v = l >= 0 ? fmaxf(b.pnb[i] + lpl, NEG) : NEG;
  const int s = b.src[i];
  if (s >= 0 && merge) v = lae(v, fmaxf((b.last[s] == l ? b.pb[s] : b.tot[s]) + lpl, NEG));
  *pnbn = v;
}
__device__ __forceinline__ void beam_topk_extend(const BeamSide& b, int i, int c, float lpc, float* pbn, float* pnbn) {
  *pbn = NEG;
  *pnbn = fmaxf((c == b.last[i] ? b.pb[i] : b.tot[i]) + lpc, NEG);
}

// The frame step of ctc_beam_kernel (phases A to E as stated there) with these differences:
//   A  the frame's kept labels flab[K] / their log-probabilities fval[K] / lp[blank] were put into LDS by wave 0 in phase E of
//      the frame before, from registers it loaded from the pre-pass rows a whole step earlier; beam slot j gathers its own
//      z[t, last[j]] (issued at the top of the step, beside the model gathers) and subtracts lsum[t] -- the expression the
//      pre-pass evaluated for a kept label, so a stay and an extension by the same label use the same bits -- and looks
//      last[j] up in flab by binary search: lpos[j] = its position or -1.  The child mask is over POSITIONS.  The dead
//      candidates are counted here, not in phase E: a child kills its parent's extension only where lpos >= 0, and phase C
//      must run whenever the LIVE candidates exceed W
//   B-D  candidate k = i * (K + 1) + q: q < K extends by flab[q], q == K stays; a stay collects its parent's extension only if
//      lpos >= 0.  With K == O - 1 flab is 0 .. O - 2 and k, the keys, the tie-breaks and every value are ctc_beam_kernel's
//   the trie key holds a 16-bit label
//   RESUME: as ctc_beam_kernel's; the look-ahead registers are primed from the chunk's own pre-pass rows
template <int LM, bool RESUME = false>
__global__ void __launch_bounds__(kBeamThreads)
ctc_beam_topk_kernel(const float* __restrict__ logits, int ld, int O, int K, const uint32_t* __restrict__ pre,
                     const int32_t* __restrict__ seg, int U, int T, int W, int top_paths,
                     unsigned long long* __restrict__ trie, int32_t* __restrict__ hyp, int32_t* __restrict__ hyp_len,
                     float* __restrict__ score, const float* __restrict__ lm, int C, float lm_w, float lm_bonus, int eos,
                     float* __restrict__ am_score, const int32_t* __restrict__ gnext, int gstart, BeamResume rs) {
  typedef typename BeamSideOf<LM>::type Side;
  __shared__ Side beam[2];
  __shared__ __attribute__((aligned(16))) uint32_t keys[kBeamKeys];
  __shared__ __attribute__((aligned(16))) uint32_t hist[256];
  __shared__ unsigned long long childmask[kCtcBeamMaxWidth];
  __shared__ int flab[64];
  __shared__ float fval[64];
  __shared__ float lpl[kCtcBeamMaxWidth];
  __shared__ int lpos[kCtcBeamMaxWidth];
  __shared__ float s_lpb;
  __shared__ float wmax[4];
  __shared__ int wsum[4];
  __shared__ int sel[4];
  __shared__ int s_nb, s_ndead;
  __shared__ int path[kCtcBeamMaxWidth];

  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = seg[u], Tn = seg[u + 1] - r0;
  const int blank = O - 1, K1 = K + 1;
  // this utterance's share of the table: load <= 1/2
  const uint32_t cap = 2u * (uint32_t)(RESUME ? rs.max_frames : Tn) * (uint32_t)W + 64u;
  unsigned long long* tab = RESUME ? trie + (unsigned long long)u * (unsigned long long)cap
                                   : trie + (2ull * (unsigned long long)r0 * (unsigned long long)W + 64ull * (unsigned long long)u);
  const uint32_t magic = (uint32_t)((0x100000000ull + (unsigned)K1 - 1u) / (unsigned)K1);  // k / K1 for k < 2^13
  const uint32_t* prow = pre + (size_t)r0 * kCtcTopkRowWords;

  beam_start<LM>(beam[0], C, gstart, hist, childmask, path, &s_nb, &s_ndead);
  int cur = 0;
  double off = 0.0;  // what has been taken out of the beam's scores so far (uniform over the block)
  if constexpr (RESUME) beam_resume_load<LM>(beam[0], rs, u, W, &s_nb, &s_ndead, &off);
  // wave 0: the next frame's list, in registers until phase E; every thread: the next frame's lsum
  uint32_t lab_next = 0x7fffffffu, val_next = 0u, lpb_next = 0u;
  float lsum_next = 0.f;
  if (Tn > 0) {
    lsum_next = __builtin_bit_cast(float, prow[128]);
    if (wave == 0) {
      flab[lane] = min((int)prow[lane], blank - 1);  // (the list's unused tail is no label: kept inside the alphabet)
      fval[lane] = __builtin_bit_cast(float, prow[64 + lane]);
      if (lane == 0) s_lpb = __builtin_bit_cast(float, prow[129]);
    }
  }
  __syncthreads();

  for (int t = 0; t < Tn; ++t) {
    const Side& b = beam[cur];
    Side& nx = beam[cur ^ 1];
    const int nb = s_nb;
    const int N = nb * K1;
    const int cpt = ((N + kBeamThreads - 1) / kBeamThreads) | 1;  // an odd run per thread: conflict-free LDS strides
    const int k0 = min(tid * cpt, N), k1 = min(k0 + cpt, N);
    float lmv[kBeamRun];
    if constexpr (LM) {  // this frame's table values: in flight under phase A
      beam_for_run(__builtin_amdgcn_readfirstlane(cpt), [&](int q) {
        const int k = k0 + q;
        lmv[q] = 0.f;
        if (k < k1) {
          const int i = (int)__umulhi((uint32_t)k, magic), p = k - i * K1;
          if (p != K) lmv[q] = lm[(size_t)b.ctx[i] * (size_t)O + (size_t)flab[p]];
        }
      });
    }
    const float lsum = lsum_next;
    float zl = 0.f;
    int mylast = -1;
    if (wave != 0 && tid - 64 < nb) {
      mylast = b.last[tid - 64];
      if (mylast >= 0) zl = logits[(size_t)(r0 + t) * ld + mylast];
    }
    if (t + 1 < Tn) {
      const uint32_t* pn = prow + (size_t)(t + 1) * kCtcTopkRowWords;
      lsum_next = __builtin_bit_cast(float, pn[128]);
      if (wave == 0) {
        lab_next = pn[lane];
        val_next = pn[64 + lane];
        lpb_next = pn[129];
      }
    }
    // A
    bool kills = false;  // this slot's label is kept at this frame, so its parent's extension by it is dead
    if (wave != 0 && tid - 64 < nb) {
      const int j = tid - 64;
      int pos = -1;
      if (mylast >= 0) {
        int lo = 0, hi = K;  // the first position whose label is >= mylast
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (flab[mid] < mylast) lo = mid + 1; else hi = mid;
        }
        if (lo < K && flab[lo] == mylast) pos = lo;
      }
      lpl[j] = zl - lsum;
      lpos[j] = pos;
      const int s = b.src[j];
      kills = s >= 0 && pos >= 0;
      if (kills) atomicOr(&childmask[s], 1ull << pos);
    }
    if (wave != 0) {  // the dead candidates, counted exactly: a child whose label is pruned here kills nothing
      const int dead = __popcll(__ballot(kills));
      if (lane == 0 && dead) atomicAdd(&s_ndead, dead);
    }
    __syncthreads();
    const int ndead = s_ndead;
    // B
    const float lpb = s_lpb;
    if constexpr (LM)
      beam_for_run(__builtin_amdgcn_readfirstlane(cpt), [&](int q) {
        if (k0 + q < k1) keys[k0 + q] = __builtin_bit_cast(uint32_t, lmv[q]);
      });
    auto candidate = [&](int i, int p, float* pbn, float* pnbn) {
      if (p == K) beam_topk_stay(b, i, lpb, lpl[i], lpos[i] >= 0, pbn, pnbn);
      else beam_topk_extend(b, i, flab[p], fval[p], pbn, pnbn);
    };
    float lmax = NEG;
    int missing = 0;  // (graph) this thread's extensions that have no arc
    for (int k = k0; k < k1; ++k) {
      const int i = (int)__umulhi((uint32_t)k, magic), p = k - i * K1;
      float pbn, pnbn;
      candidate(i, p, &pbn, &pnbn);
      bool live = p == K || !((childmask[i] >> p) & 1ull);
      const float tot = lae(pbn, pnbn);
      float rank = tot;  // what the beam is cut by; the re-centring (lmax) stays on the acoustic part
      if constexpr (LM == kBeamGraph) {
        const float g = b.g[i], wv = __builtin_bit_cast(float, keys[k]);
        const bool arc = p == K || wv > -INFINITY;
        missing += !arc;
        live = live && arc;
        rank = tot + (p == K || !arc ? g : beam_lm_extend(g, lm_w, wv, lm_bonus));
      } else if constexpr (LM) {
        const float g = b.g[i];
        rank = tot + (p == K ? g : beam_lm_extend(g, lm_w, __builtin_bit_cast(float, keys[k]), lm_bonus));
      }
      keys[k] = live ? sortable(rank) : 0u;
      if (live) lmax = fmaxf(lmax, tot);
    }
    lmax = wave_max(lmax);
    if (lane == 0) wmax[wave] = lmax;
    if constexpr (LM == kBeamGraph) {  // as ctc_beam_kernel: the missing arcs ride through wmax's barrier in sel[]
      for (int o = 32; o > 0; o >>= 1) missing += __shfl_xor(missing, o);
      if (lane == 0) sel[wave] = missing;
    }
    __syncthreads();
    float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (!(m > -1e29f)) m = 0.f;
    int nlive = N - ndead;
    if constexpr (LM == kBeamGraph) nlive -= sel[0] + sel[1] + sel[2] + sel[3];
    // C
    uint32_t Kk = 0u, K2 = 0xffffffffu;  // select: key > Kk, or key == Kk and tie-break key >= K2
    if (nlive > W) {
      int take, have;
      Kk = beam_radix_select([&](int k) { return keys[k]; }, k0, k1, W, hist, sel, &take, &have);
      K2 = 0u;
      if (take < have) {
        int t2, h2;
        K2 = beam_radix_select(
            [&](int k) {
              const int i = (int)__umulhi((uint32_t)k, magic), p = k - i * K1;
              return keys[k] == Kk ? beam_tiebreak(b.len[i] + (p != K), k) : 0u;
            },
            k0, k1, take, hist, sel, &t2, &h2);
      }
    }
    // D
    int cnt = 0;
    for (int k = k0; k < k1; ++k) {
      const uint32_t key = keys[k];
      if (key > Kk) { ++cnt; continue; }
      if (key == Kk && K2 != 0xffffffffu) {
        const int i = (int)__umulhi((uint32_t)k, magic), p = k - i * K1;
        cnt += beam_tiebreak(b.len[i] + (p != K), k) >= K2;
      }
    }
    int incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int slot = incl - cnt;
    for (int w = 0; w < wave; ++w) slot += wsum[w];
    const int nb_new = min(wsum[0] + wsum[1] + wsum[2] + wsum[3], W);
    for (int k = k0; k < k1; ++k) {
      const uint32_t key = keys[k];
      const int i = (int)__umulhi((uint32_t)k, magic), p = k - i * K1;
      const bool chosen = key > Kk || (key == Kk && K2 != 0xffffffffu && beam_tiebreak(b.len[i] + (p != K), k) >= K2);
      if (!chosen) continue;
      if (slot < W) {
        float pbn, pnbn;
        candidate(i, p, &pbn, &pnbn);
        pbn = fmaxf(pbn - m, NEG);
        pnbn = fmaxf(pnbn - m, NEG);
        nx.pb[slot] = pbn;
        nx.pnb[slot] = pnbn;
        nx.tot[slot] = lae(pbn, pnbn);
        if (p == K) {
          nx.node[slot] = b.node[i]; nx.parent[slot] = b.parent[i]; nx.last[slot] = b.last[i]; nx.len[slot] = b.len[i];
          if constexpr (LM) { nx.g[slot] = b.g[i]; nx.ctx[slot] = b.ctx[i]; }
        } else {
          const int c = flab[p];
          float lv = 0.f;
          int ns = 0;
          if constexpr (LM) lv = lm[(size_t)b.ctx[i] * (size_t)O + (size_t)c];  // issued ahead of the trie probe
          if constexpr (LM == kBeamGraph) ns = gnext[(size_t)b.ctx[i] * (size_t)O + (size_t)c];
          // find or insert (parent node, label): the slot is the node's id
          const unsigned long long nk = ((unsigned long long)(uint32_t)b.node[i] << 16) | (unsigned long long)c;
          uint32_t pos = __umulhi((uint32_t)((nk * 0x9E3779B97F4A7C15ull) >> 32), cap);
          int id = 0;
          for (uint32_t n = 0; n < cap; ++n) {
            const unsigned long long old = atomicCAS(&tab[pos], kTrieEmpty, nk);
            if (old == kTrieEmpty || old == nk) { id = (int)pos; break; }
            pos = pos + 1u == cap ? 0u : pos + 1u;
          }
          nx.node[slot] = id; nx.parent[slot] = b.node[i]; nx.last[slot] = c; nx.len[slot] = b.len[i] + 1;
          if constexpr (LM) {
            nx.g[slot] = beam_lm_extend(b.g[i], lm_w, lv, lm_bonus);
            if constexpr (LM == kBeamGraph) nx.ctx[slot] = ns;
            else nx.ctx[slot] = (int)(((uint32_t)b.ctx[i] * (uint32_t)O + (uint32_t)c) % (uint32_t)C);
          }
        }
      }
      ++slot;
    }
    if (tid == 0) {
      s_nb = nb_new;
      s_ndead = 0;
    }
    off += (double)m;
    __syncthreads();
    // E
    if (tid < kCtcBeamMaxWidth) childmask[tid] = 0ull;
    if (wave == 0) {  // the next frame's list (nobody reads this frame's any more)
      flab[lane] = min((int)lab_next, blank - 1);
      fval[lane] = __builtin_bit_cast(float, val_next);
      if (lane == 0) s_lpb = __builtin_bit_cast(float, lpb_next);
    }
    {
      int s = -1;
      if (tid < nb_new) {
        const int p = nx.parent[tid];
        for (int i = 0; i < nb_new; ++i)
          if (nx.node[i] == p) s = i;
        nx.src[tid] = s;
      }
    }
    cur ^= 1;
    __syncthreads();
  }

  if constexpr (RESUME) {
    beam_resume_store<LM>(beam[cur], rs, u, W, s_nb, s_ndead, off, lm, O, lm_w);
    return;
  }
  // the top_paths best of the final beam, as ctc_beam_kernel
  const Side& b = beam[cur];
  const int nb = s_nb;
  if constexpr (LM) {  // the combined values, parked in keys[] as floats
    if (tid < nb) {
      float v = b.tot[tid] + b.g[tid];
      if (eos) {
        const float fw = lm[(size_t)b.ctx[tid] * (size_t)O + (size_t)blank];
        if (LM == kBeamGraph && !(fw > -INFINITY)) v = -INFINITY;  // not final, whatever lm_weight is
        else v = beam_lm_end(v, lm_w, fw);
      }
      keys[tid] = __builtin_bit_cast(uint32_t, v);
    }
    __syncthreads();
  }
  auto final_value = [&](int i) -> float {
    if constexpr (LM) return __builtin_bit_cast(float, keys[i]);
    else return b.tot[i];
  };
  if (tid < nb) {
    const uint32_t kj = sortable(final_value(tid));
    const int lj = b.len[tid];
    int rank = 0;
    for (int i = 0; i < nb; ++i) {
      const uint32_t ki = sortable(final_value(i));
      const int li = b.len[i];
      rank += ki > kj || (ki == kj && (li < lj || (li == lj && i < tid)));
    }
    path[rank] = tid;
  }
  __syncthreads();
  for (int n = 0; n < top_paths; ++n) {
    const int j = path[n];
    const int L = j >= 0 ? min(b.len[j], Tn) : 0;
    int32_t* out = hyp + (size_t)n * T + r0;
    for (int f = L + tid; f < Tn; f += kBeamThreads) out[f] = -1;
    if (tid == 0) {
      hyp_len[(size_t)n * U + u] = L;
      const bool alive = j >= 0 && b.tot[j] > -1e29f;
      score[(size_t)n * U + u] = alive ? (float)(off + (double)final_value(j)) : -INFINITY;
      if (am_score) am_score[(size_t)n * U + u] = alive ? (float)(off + (double)b.tot[j]) : -INFINITY;
    }
  }
  if (tid < top_paths && path[tid] >= 0) {  // back-trace through the parent links, labels land in forward order
    const int j = path[tid];
    int32_t* out = hyp + (size_t)tid * T + r0;
    uint32_t node = (uint32_t)b.node[j];
    for (int pos = min(b.len[j], Tn) - 1; pos >= 0 && node < cap; --pos) {
      const unsigned long long nk = __hip_atomic_load(&tab[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      out[pos] = (int32_t)(nk & 0xffffull);
      node = (uint32_t)(nk >> 16);
    }
  }
}

// The N-best of a stream's lanes from their saved state (BeamResume's layout) and tries: what the epilogue of the two kernels
// above produces, written beside them on purpose (the comment at beam_start says what sharing a body with them costs).  ONE
// WORKGROUP PER LANE; it reads no model -- the end terms were saved -- and writes neither the state nor the trie.  kind: the
// model the lane's state was saved under (kBeamAm: the value is tot; else tot + g, and with eos the end term on top, -inf for a
// graph state that is not final); lbits: the width of a trie key's label field (6: ctc_beam_kernel, 16: ctc_beam_topk_kernel).
// A lane that has not been pushed since its reset (live == 0) is the empty prefix with both scores 0.
// Out: hyp[(n * U + u) * stride + k] for k < hyp_len[n * U + u] (nothing beyond: the host pads), score / am_score [n * U + u].
__global__ void __launch_bounds__(kBeamThreads)
ctc_stream_result_kernel(const int32_t* __restrict__ hdr, const uint32_t* __restrict__ arr,
                         const unsigned long long* __restrict__ trie, int U, int W, int max_frames, int kind, int eos,
                         int lbits, int top_paths, int stride, int32_t* __restrict__ hyp, int32_t* __restrict__ hyp_len,
                         float* __restrict__ score, float* __restrict__ am_score) {
  __shared__ float val[kCtcBeamMaxWidth], tot[kCtcBeamMaxWidth];
  __shared__ int len[kCtcBeamMaxWidth], path[kCtcBeamMaxWidth];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int32_t* hd = hdr + (size_t)u * kCtcStreamHdrWords;
  const uint32_t* a = arr + (size_t)u * kCtcStreamArrays * (size_t)W;
  const uint32_t cap = 2u * (uint32_t)max_frames * (uint32_t)W + 64u;
  const unsigned long long* tab = trie + (unsigned long long)u * (unsigned long long)cap;
  const bool live = hd[0] != 0;
  const int nb = live ? hd[1] : 1;
  const double off = live ? *reinterpret_cast<const double*>(hd + 4) : 0.0;
  const float lm_w = __builtin_bit_cast(float, (uint32_t)hd[3]);
  if (tid < kCtcBeamMaxWidth) path[tid] = -1;
  if (tid < nb) {
    const float t = live ? __builtin_bit_cast(float, a[2 * W + tid]) : 0.f;
    float v = t;
    if (kind != kBeamAm) {
      v = t + (live ? __builtin_bit_cast(float, a[8 * W + tid]) : 0.f);
      if (eos) {
        const float fw = __builtin_bit_cast(float, a[10 * W + tid]);
        if (kind == kBeamGraph && !(fw > -INFINITY)) v = -INFINITY;  // not final, whatever lm_weight is
        else v = beam_lm_end(v, lm_w, fw);
      }
    }
    tot[tid] = t;
    val[tid] = v;
    len[tid] = live ? (int)a[6 * W + tid] : 0;
  }
  __syncthreads();
  if (tid < nb) {  // higher value, then shorter, then lower slot
    const uint32_t kj = sortable(val[tid]);
    const int lj = len[tid];
    int rank = 0;
    for (int i = 0; i < nb; ++i) {
      const uint32_t ki = sortable(val[i]);
      const int li = len[i];
      rank += ki > kj || (ki == kj && (li < lj || (li == lj && i < tid)));
    }
    path[rank] = tid;
  }
  __syncthreads();
  if (tid < top_paths) {
    const int j = path[tid];
    const size_t at = (size_t)tid * U + u;
    const int L = j >= 0 ? min(len[j], stride) : 0;
    hyp_len[at] = L;
    const bool alive = j >= 0 && tot[j] > -1e29f;
    score[at] = alive ? (float)(off + (double)val[j]) : -INFINITY;
    if (am_score) am_score[at] = alive ? (float)(off + (double)tot[j]) : -INFINITY;
    if (j >= 0 && live) {  // back-trace through the parent links, labels land in forward order
      int32_t* out = hyp + at * (size_t)stride;
      uint32_t node = a[3 * W + j];
      const unsigned long long mask = (1ull << lbits) - 1ull;
      for (int pos = L - 1; pos >= 0 && node < cap; --pos) {
        const unsigned long long nk = __hip_atomic_load(&tab[node], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out[pos] = (int32_t)(nk & mask);
        node = (uint32_t)(nk >> lbits);
      }
    }
  }
}

// ---- forced alignment (the Viterbi path of the CTC lattice; the contract is stated in ctc.h) ----

// one wave per row: lse[t] = log-sum-exp of logits row t (what the alignment score subtracts per frame)
__global__ void __launch_bounds__(256)
ctc_row_lse_kernel(const float* __restrict__ logits, int ld, int O, int T, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* z = logits + (size_t)row * ld;
  float mx = -INFINITY;
  for (int c = lane; c < O; c += 64) mx = fmaxf(mx, z[c]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float se = 0.f;
  for (int c = lane; c < O; c += 64) se += expf(z[c] - mx);
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
  if (lane == 0) lse[row] = mx + logf(se);
}

// back-pointers of one lane and one frame: 2 bits per state, the lane's R states in one unit (R = 2 uses half a byte)
template <int R> struct BpUnit { typedef uint8_t type; };
template <> struct BpUnit<8> { typedef uint16_t type; };
template <> struct BpUnit<16> { typedef uint32_t type; };
constexpr int bp_row_bytes(int R) { return 64 * (R <= 4 ? 1 : R / 4); }

// ONE WAVE PER UTTERANCE, two chains of Tn dependent steps:
//   forward    the max-plus twin of ctc_alpha_beta's forward sweep on the RAW logits of the states' classes (gathered here,
//              PFD rows in flight in a register ring): lane-owned states, DPP neighbour shifts, the state vector re-centred
//              on its maximum with the sum of the shifts in double.  lse3 becomes the ordered max of (stay, advance by 1,
//              advance by 2) -- a later candidate wins only if strictly larger -- whose index is the back-pointer; a lane
//              stores the 2-bit back-pointers of its R states of a frame as ONE unit, a frame is bp_row_bytes(R) bytes
//   backtrace  the back-pointer rows of 64 frames (<= 16 KB) are staged in LDS by all lanes (the block before it is already
//              in flight in registers), then walked at LDS latency: one dependent ds_read per frame instead of one L2 round
//              trip; the walk is wave-uniform, lane j keeps the state of the block's frame j and all lanes store ali
// score = (offset + value of the end state) - sum of the rows' log-sum-exps, both sums in double.
template <int R>
__global__ void __launch_bounds__(64)
ctc_viterbi_kernel(const float* __restrict__ logits, int ld, int O, const int32_t* __restrict__ seg,
                   const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_off, const float* __restrict__ lse,
                   unsigned char* __restrict__ bp, int32_t* __restrict__ ali, float* __restrict__ score) {
  typedef typename BpUnit<R>::type Unit;
  constexpr int kRowBytes = bp_row_bytes(R);
  constexpr int NV = kRowBytes / 16;  // 16-byte words per lane of a 64-frame block = per frame row
  __shared__ uint4 stage[64 * NV];
  const int u = blockIdx.x, lane = threadIdx.x;
  const int r0 = seg[u], Tn = seg[u + 1] - r0;
  const int l0 = lab_off[u], S = lab_off[u + 1] - l0, n = 2 * S + 1;
  if (Tn <= 0) {  // an utterance without frames: only the empty labelling has a path (the empty one)
    if (lane == 0) score[u] = S == 0 ? 0.f : -INFINITY;
    return;
  }
  const int s0 = lane * R;
  int cls[R];
  bool skip_in[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int s = s0 + r, j = s >> 1;
    const bool lab = (s & 1) && s < n;
    cls[r] = lab ? min(max(labels[l0 + j], 0), O - 1) : O - 1;  // (clamped: a bad label must not become a bad address)
    skip_in[r] = lab && j >= 1 && labels[l0 + j] != labels[l0 + j - 1];
  }
  const float* zu = logits + (size_t)r0 * ld;
  Unit* bpu = reinterpret_cast<Unit*>(bp + (size_t)r0 * kRowBytes) + lane;
  constexpr int PFD = 8;
  float pre[PFD][R];
  double off = 0.0;
  float a[R];
#pragma unroll
  for (int r = 0; r < R; ++r) a[r] = (s0 + r < 2 && s0 + r < n) ? zu[cls[r]] : NEG;
  bpu[0] = (Unit)0;  // the first frame has no predecessor; the walk reads the row all the same
#pragma unroll
  for (int j = 0; j < PFD; ++j)
#pragma unroll
    for (int r = 0; r < R; ++r) pre[j][r] = zu[(size_t)min(1 + j, Tn - 1) * ld + cls[r]];
  for (int t0 = 1; t0 < Tn; t0 += PFD) {
#pragma unroll
    for (int j = 0; j < PFD; ++j) {
      const int t = t0 + j;
      const bool live = t < Tn;
      float cur[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        cur[r] = pre[j][r];
        pre[j][r] = zu[(size_t)min(t + PFD, Tn - 1) * ld + cls[r]];
      }
      const float up1 = lane_prev(a[R - 1], NEG, lane), up2 = lane_prev(a[R - 2], NEG, lane);
      float na[R];
      uint32_t code = 0u;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float p1 = r >= 1 ? a[r - 1] : up1;
        const float p2 = r >= 2 ? a[r - 2] : (r == 1 ? up1 : up2);
        float best = a[r];
        uint32_t d = 0u;
        if (p1 > best) { best = p1; d = 1u; }
        if (skip_in[r] && p2 > best) { best = p2; d = 2u; }
        const float v = (s0 + r < n) ? best + cur[r] : NEG;
        na[r] = live ? v : a[r];
        code |= d << (2 * r);
      }
      if (j == PFD - 1) {  // compile-time: re-centre the state vector on its maximum
        float m = NEG;
#pragma unroll
        for (int r = 0; r < R; ++r) m = fmaxf(m, na[r]);
        m = wave_max(m);
        if (live && m > -1e29f) {
          off += (double)m;
#pragma unroll
          for (int r = 0; r < R; ++r) na[r] = fmaxf(na[r] - m, NEG);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = na[r];
      if (live) bpu[(size_t)t * (kRowBytes / sizeof(Unit))] = (Unit)code;  // (a surplus step holds the state and stores nothing)
    }
  }
  // the end state: n - 1 unless n - 2 is strictly larger
  float e1 = -INFINITY, e2 = -INFINITY;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (s0 + r == n - 1) e1 = a[r];
    if (s0 + r == n - 2) e2 = a[r];
  }
  e1 = wave_max(e1);
  e2 = wave_max(e2);
  int s = e2 > e1 ? n - 2 : n - 1;
  const float vend = fmaxf(e1, e2);
  if (!(vend > -1e29f)) {  // too short for its labels: no path
    for (int f = lane; f < Tn; f += 64) ali[r0 + f] = -2;
    if (lane == 0) score[u] = -INFINITY;
    return;
  }
  double ls = 0.0;
  for (int f = lane; f < Tn; f += 64) ls += (double)lse[r0 + f];
  for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o);
  if (lane == 0) score[u] = (float)((off + (double)vend) - ls);

  __threadfence();  // the back-pointers this wave stored, read back by other lanes
  const uint4* g = reinterpret_cast<const uint4*>(bp + (size_t)r0 * kRowBytes);
  const int words = Tn * NV;  // the utterance's rows in 16-byte words (Tn <= T, NV <= 16)
  uint4 nxt[NV];
  const int nblk = (Tn + 63) >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int w = (nblk - 1) * 64 * NV + i * 64 + lane;
    nxt[i] = w < words ? g[w] : make_uint4(0u, 0u, 0u, 0u);
  }
  const uint32_t* rows = reinterpret_cast<const uint32_t*>(stage);
  for (int b = nblk - 1; b >= 0; --b) {
    __syncthreads();  // (one wave: orders the walk's reads before the next block's writes)
#pragma unroll
    for (int i = 0; i < NV; ++i) stage[i * 64 + lane] = nxt[i];
    if (b > 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) nxt[i] = g[(b - 1) * 64 * NV + i * 64 + lane];  // a full block of the utterance's rows
    }
    __syncthreads();
    const int f0 = 64 * b, cnt = min(64, Tn - f0);
    int mine = 0;
    for (int j = cnt - 1; j >= 0; --j) {
      if (lane == j) mine = s;
      const int bit = R == 2 ? 8 * (s >> 1) + 2 * (s & 1) : 2 * s;
      const uint32_t w = rows[j * (kRowBytes / 4) + (bit >> 5)];
      s = max(s - (int)((w >> (bit & 31)) & 3u), 0);
    }
    if (lane < cnt) ali[r0 + f0 + lane] = (mine & 1) ? mine >> 1 : -1;
  }
}

// ---- N-best rescoring (the exact log p(labels | x) of named label sequences; the contract is stated in ctc.h) ----

// ONE WAVE PER (utterance, hypothesis) PAIR: the forward sweep of ctc_alpha_beta_kernel in the sum-product semiring -- lse3,
// lane-owned states, DPP neighbour shifts, PFD rows in flight with clamped row indices, the state vector re-centred on its
// maximum every PFD steps with the sum of the shifts in double, the end reduction over n - 1 and n - 2 -- fed as
// ctc_viterbi_kernel is: the lane gathers the logits of its states' classes itself and nothing is stored per frame.  The
// emission is lp = z[t, cls] - lse[t] in fp32, the expression ctc_gather_kernel evaluates; lse[t] (ctc_row_lse_kernel, one
// value per frame whatever the number of pairs) rides in the ring beside the row.  The pairs of one utterance are adjacent
// in the grid and read the same rows: the first wave brings a row into the cache, its neighbours find it there.
template <int R>
__global__ void __launch_bounds__(64)
ctc_score_kernel(const float* __restrict__ logits, int ld, int O, const int32_t* __restrict__ seg, int U,
                 const int32_t* __restrict__ pair_utt, const int32_t* __restrict__ labels,
                 const int32_t* __restrict__ lab_off, const float* __restrict__ lse, float* __restrict__ score) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int u = min(max(pair_utt[p], 0), U - 1);  // (clamped: a bad index must not become a bad address)
  const int r0 = seg[u], Tn = seg[u + 1] - r0;
  const int l0 = lab_off[p], S = lab_off[p + 1] - l0, n = 2 * S + 1;
  if (Tn <= 0) {  // an utterance without frames: only the empty labelling is possible
    if (lane == 0) score[p] = S == 0 ? 0.f : -INFINITY;
    return;
  }
  if (S < 0 || n > 64 * R) {  // not this launch's register tile (the launcher's max_labels rules it out)
    if (lane == 0) score[p] = __builtin_nanf("");
    return;
  }
  const int s0 = lane * R;
  int cls[R];
  bool skip_in[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int s = s0 + r, j = s >> 1;
    const bool lab = (s & 1) && s < n;
    cls[r] = lab ? min(max(labels[l0 + j], 0), O - 1) : O - 1;
    skip_in[r] = lab && j >= 1 && labels[l0 + j] != labels[l0 + j - 1];
  }
  const float* zu = logits + (size_t)r0 * ld;
  const float* lu = lse + r0;
  constexpr int PFD = 8;
  float pre[PFD][R], prl[PFD];
  double off = 0.0;
  float a[R];
  {
    const float l = lu[0];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = (s0 + r < 2 && s0 + r < n) ? zu[cls[r]] - l : NEG;
  }
#pragma unroll
  for (int j = 0; j < PFD; ++j) {
    const int row = min(1 + j, Tn - 1);
    prl[j] = lu[row];
#pragma unroll
    for (int r = 0; r < R; ++r) pre[j][r] = zu[(size_t)row * ld + cls[r]];
  }
  for (int t0 = 1; t0 < Tn; t0 += PFD) {
#pragma unroll
    for (int j = 0; j < PFD; ++j) {
      const int t = t0 + j;
      const bool live = t < Tn;
      const int nrow = min(t + PFD, Tn - 1);
      float cur[R];
      const float curl = prl[j];
      prl[j] = lu[nrow];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        cur[r] = pre[j][r] - curl;
        pre[j][r] = zu[(size_t)nrow * ld + cls[r]];
      }
      const float up1 = lane_prev(a[R - 1], NEG, lane), up2 = lane_prev(a[R - 2], NEG, lane);
      float na[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float p1 = r >= 1 ? a[r - 1] : up1;
        const float p2 = r >= 2 ? a[r - 2] : (r == 1 ? up1 : up2);
        const float v = (s0 + r < n) ? lse3(a[r], p1, skip_in[r] ? p2 : NEG) + cur[r] : NEG;
        na[r] = live ? v : a[r];
      }
      if (j == PFD - 1) {  // compile-time: re-centre the state vector on its maximum
        float m = NEG;
#pragma unroll
        for (int r = 0; r < R; ++r) m = fmaxf(m, na[r]);
        m = wave_max(m);
        if (live && m > -1e29f) {
          off += (double)m;
#pragma unroll
          for (int r = 0; r < R; ++r) na[r] = fmaxf(na[r] - m, NEG);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = na[r];
    }
  }
  // log p(labels) = alpha_T(n-1) (+) alpha_T(n-2)
  float m = NEG;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (s0 + r == n - 1 || s0 + r == n - 2) m = fmaxf(m, a[r]);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float se = 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (s0 + r == n - 1 || s0 + r == n - 2) se += expf(a[r] - m);
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
  const float log_z_rel = m + logf(se);  // relative to the final offset
  if (lane == 0) score[p] = log_z_rel > -1e29f ? (float)(off + (double)log_z_rel) : -INFINITY;
}

// ---- alignment with wildcard gaps and keyword spotting (the contract is stated in ctc.h and at tfk_ctc_align_wild) ----
//
// The lattice of ctc_viterbi_kernel with one change: a GAP (an even state) whose flag is set emits the frame's largest logit
// instead of the blank's.  No transition, tie or shift changes, so these are twins of ctc_viterbi_kernel / ctc_score_kernel
// with their own text: the tuned loops above stay as they are.

// one wave per row: rowmax[t] = largest logit of row t, lse[t] = its log-sum-exp (the expression of ctc_row_lse_kernel)
__global__ void __launch_bounds__(256)
ctc_row_max_lse_kernel(const float* __restrict__ logits, int ld, int O, int T, float* __restrict__ rowmax,
                       float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= T) return;
  const float* z = logits + (size_t)row * ld;
  float mx = -INFINITY;
  for (int c = lane; c < O; c += 64) mx = fmaxf(mx, z[c]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float se = 0.f;
  for (int c = lane; c < O; c += 64) se += expf(z[c] - mx);
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
  if (lane == 0) {
    rowmax[row] = mx;
    lse[row] = mx + logf(se);
  }
}

// one wave per utterance: free[u] = sum_t (rowmax[t] - lse[t]) in double, the log-probability of the per-frame best path
__global__ void __launch_bounds__(64)
ctc_free_score_kernel(const int32_t* __restrict__ seg, const float* __restrict__ rowmax, const float* __restrict__ lse,
                      float* __restrict__ free_score) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const int r0 = seg[u], Tn = seg[u + 1] - r0;
  double fs = 0.0;
  for (int f = lane; f < Tn; f += 64) fs += (double)rowmax[r0 + f] - (double)lse[r0 + f];
  for (int o = 32; o > 0; o >>= 1) fs += __shfl_xor(fs, o);
  if (lane == 0) free_score[u] = (float)fs;
}

// the emission of a gap state: the row maximum where mask is all ones, the blank's logit where it is zero (v_bfi_b32)
__device__ __forceinline__ float wild_pick(uint32_t mask, float rowmax, float blank) {
  return __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, rowmax) & mask) | (__builtin_bit_cast(uint32_t, blank) & ~mask));
}
__device__ __forceinline__ int lane_prev_int(int v, int fill, int lane) {
  const int r = __builtin_amdgcn_update_dpp(0, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
  return lane == 0 ? fill : r;
}

// ONE WAVE PER UTTERANCE: ctc_viterbi_kernel's two chains (the PFD ring, the re-centring, the 2-bit back-pointer units, the
// LDS-staged back-trace) with the emission select, decided before the frame loop: a lane's states are R / 2 (gap, label)
// couples; the ring holds per row the label states' logits, the blank's logit and the row maximum (both wave-uniform), and
// a per-couple mask picks the gap's emission from those two.
// wild: the flags of utterance u are wild[lab_off[u] + u + g], g in [0, S]; NULL: none set.
template <int R>
__global__ void __launch_bounds__(64)
ctc_viterbi_wild_kernel(const float* __restrict__ logits, int ld, int O, const int32_t* __restrict__ seg,
                        const int32_t* __restrict__ labels, const int32_t* __restrict__ lab_off,
                        const uint8_t* __restrict__ wild, const float* __restrict__ rowmax, const float* __restrict__ lse,
                        unsigned char* __restrict__ bp, int32_t* __restrict__ ali, float* __restrict__ score) {
  typedef typename BpUnit<R>::type Unit;
  constexpr int kRowBytes = bp_row_bytes(R);
  constexpr int NV = kRowBytes / 16;
  __shared__ uint4 stage[64 * NV];
  const int u = blockIdx.x, lane = threadIdx.x;
  const int r0 = seg[u], Tn = seg[u + 1] - r0;
  const int l0 = lab_off[u], S = lab_off[u + 1] - l0, n = 2 * S + 1;
  if (Tn <= 0) {
    if (lane == 0) score[u] = S == 0 ? 0.f : -INFINITY;
    return;
  }
  const int s0 = lane * R;
  const float* zu = logits + (size_t)r0 * ld;
  const float* mu = rowmax + r0;
  constexpr int H = R / 2;  // the lane's R states are H (gap, label) couples: s0 is even
  int lo[H];        // class of the couple's label state
  uint32_t wm[H];   // all ones where the couple's gap is a wildcard
  bool skip_in[H];  // the label state may be entered by a step of 2
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const int s = s0 + 2 * k, j = s >> 1;
    const bool lab = s + 1 < n;
    lo[k] = lab ? min(max(labels[l0 + j], 0), O - 1) : O - 1;  // (clamped: a bad label must not become a bad address)
    wm[k] = (wild && s < n && wild[(size_t)l0 + u + j] != 0) ? ~0u : 0u;
    skip_in[k] = lab && j >= 1 && labels[l0 + j] != labels[l0 + j - 1];
  }
  Unit* bpu = reinterpret_cast<Unit*>(bp + (size_t)r0 * kRowBytes) + lane;
  constexpr int PFD = 8;
  float pre[PFD][H], prb[PFD], prm[PFD];  // a row in flight: the label states' logits, the blank's, the row maximum
  double off = 0.0;
  float a[R];
#pragma unroll
  for (int r = 0; r < R; ++r) a[r] = NEG;
  if (lane == 0) {
    a[0] = wild_pick(wm[0], mu[0], zu[O - 1]);
    if (n > 1) a[1] = zu[lo[0]];
  }
  bpu[0] = (Unit)0;
#pragma unroll
  for (int j = 0; j < PFD; ++j) {
    const int row = min(1 + j, Tn - 1);
    const float* zr = zu + (size_t)row * ld;
    prb[j] = zr[O - 1];
    prm[j] = mu[row];
#pragma unroll
    for (int k = 0; k < H; ++k) pre[j][k] = zr[lo[k]];
  }
  for (int t0 = 1; t0 < Tn; t0 += PFD) {
#pragma unroll
    for (int j = 0; j < PFD; ++j) {
      const int t = t0 + j;
      const bool live = t < Tn;
      const int nrow = min(t + PFD, Tn - 1);
      float cur[R];
      {
        const float* zr = zu + (size_t)nrow * ld;
        const float cb = prb[j], cm = prm[j];
        prb[j] = zr[O - 1];
        prm[j] = mu[nrow];
#pragma unroll
        for (int k = 0; k < H; ++k) {
          cur[2 * k] = wild_pick(wm[k], cm, cb);
          cur[2 * k + 1] = pre[j][k];
          pre[j][k] = zr[lo[k]];
        }
      }
      const float up1 = lane_prev(a[R - 1], NEG, lane), up2 = lane_prev(a[R - 2], NEG, lane);
      float na[R];
      uint32_t code = 0u;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float p1 = r >= 1 ? a[r - 1] : up1;
        const float p2 = r >= 2 ? a[r - 2] : (r == 1 ? up1 : up2);
        float best = a[r];
        uint32_t d = 0u;
        if (p1 > best) { best = p1; d = 1u; }
        if ((r & 1) && skip_in[r >> 1] && p2 > best) { best = p2; d = 2u; }
        const float v = (s0 + r < n) ? best + cur[r] : NEG;
        na[r] = live ? v : a[r];
        code |= d << (2 * r);
      }
      if (j == PFD - 1) {  // compile-time: re-centre the state vector on its maximum
        float m = NEG;
#pragma unroll
        for (int r = 0; r < R; ++r) m = fmaxf(m, na[r]);
        m = wave_max(m);
        if (live && m > -1e29f) {
          off += (double)m;
#pragma unroll
          for (int r = 0; r < R; ++r) na[r] = fmaxf(na[r] - m, NEG);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = na[r];
      if (live) bpu[(size_t)t * (kRowBytes / sizeof(Unit))] = (Unit)code;
    }
  }
  // the end state: n - 1 unless n - 2 is strictly larger
  float e1 = -INFINITY, e2 = -INFINITY;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (s0 + r == n - 1) e1 = a[r];
    if (s0 + r == n - 2) e2 = a[r];
  }
  e1 = wave_max(e1);
  e2 = wave_max(e2);
  int s = e2 > e1 ? n - 2 : n - 1;
  const float vend = fmaxf(e1, e2);
  if (!(vend > -1e29f)) {  // too short for its labels: no path
    for (int f = lane; f < Tn; f += 64) ali[r0 + f] = -2;
    if (lane == 0) score[u] = -INFINITY;
    return;
  }
  double ls = 0.0;
  for (int f = lane; f < Tn; f += 64) ls += (double)lse[r0 + f];
  for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o);
  if (lane == 0) score[u] = (float)((off + (double)vend) - ls);

  __threadfence();  // the back-pointers this wave stored, read back by other lanes
  const uint4* g = reinterpret_cast<const uint4*>(bp + (size_t)r0 * kRowBytes);
  const int words = Tn * NV;
  uint4 nxt[NV];
  const int nblk = (Tn + 63) >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int w = (nblk - 1) * 64 * NV + i * 64 + lane;
    nxt[i] = w < words ? g[w] : make_uint4(0u, 0u, 0u, 0u);
  }
  const uint32_t* rows = reinterpret_cast<const uint32_t*>(stage);
  for (int b = nblk - 1; b >= 0; --b) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) stage[i * 64 + lane] = nxt[i];
    if (b > 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) nxt[i] = g[(b - 1) * 64 * NV + i * 64 + lane];
    }
    __syncthreads();
    const int f0 = 64 * b, cnt = min(64, Tn - f0);
    int mine = 0;
    for (int j = cnt - 1; j >= 0; --j) {
      if (lane == j) mine = s;
      const int bit = R == 2 ? 8 * (s >> 1) + 2 * (s & 1) : 2 * s;
      const uint32_t w = rows[j * (kRowBytes / 4) + (bit >> 5)];
      s = max(s - (int)((w >> (bit & 31)) & 3u), 0);
    }
    if (lane < cnt) ali[r0 + f0 + lane] = (mine & 1) ? mine >> 1 : -1;  // (a gap frame, blank or wildcard: -1)
  }
}

// ONE WAVE PER (utterance, pattern) PAIR: the same max-plus recursion with nothing stored per frame, as ctc_score_kernel
// stores nothing.  Beside every state value travels the START FRAME of the path that reaches it: set when the path enters
// state 1 from state 0 (or starts there), inherited from the predecessor the tie rule picks, shifted between lanes as the
// values are.  The end frame is read at state n - 1: a gap state keeps the frame at which it was last entered from the label
// before it (a label state needs none: its path's last label frame is the current one).  The arithmetic
// -- raw logits, the re-centring every PFD steps, the sums in double -- is ctc_viterbi_wild_kernel's expression for
// expression, so score equals its score bit for bit and (start, end) are its path's.
// wild: the flags of pair p are wild[lab_off[p] + p + g]; NULL: none set.
template <int R>
__global__ void __launch_bounds__(64)
ctc_spot_kernel(const float* __restrict__ logits, int ld, int O, const int32_t* __restrict__ seg, int U,
                const int32_t* __restrict__ pair_utt, const int32_t* __restrict__ labels,
                const int32_t* __restrict__ lab_off, const uint8_t* __restrict__ wild, const float* __restrict__ rowmax,
                const float* __restrict__ lse, float* __restrict__ score, int32_t* __restrict__ start,
                int32_t* __restrict__ end) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int u = min(max(pair_utt[p], 0), U - 1);  // (clamped: a bad index must not become a bad address)
  const int r0 = seg[u], Tn = seg[u + 1] - r0;
  const int l0 = lab_off[p], S = lab_off[p + 1] - l0, n = 2 * S + 1;
  if (Tn <= 0) {  // an utterance without frames: only the empty pattern has a path (the empty one)
    if (lane == 0) {
      score[p] = S == 0 ? 0.f : -INFINITY;
      start[p] = end[p] = S == 0 ? 0 : -1;
    }
    return;
  }
  if (S < 0 || n > 64 * R) {  // not this launch's register tile (the launcher's max_labels rules it out)
    if (lane == 0) {
      score[p] = __builtin_nanf("");
      start[p] = end[p] = -1;
    }
    return;
  }
  const int s0 = lane * R;
  const float* zu = logits + (size_t)r0 * ld;
  const float* mu = rowmax + r0;
  constexpr int H = R / 2;  // the lane's R states are H (gap, label) couples: s0 is even
  int lo[H];        // class of the couple's label state
  uint32_t wm[H];   // all ones where the couple's gap is a wildcard
  bool skip_in[H];  // the label state may be entered by a step of 2
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const int s = s0 + 2 * k, j = s >> 1;
    const bool lab = s + 1 < n;
    lo[k] = lab ? min(max(labels[l0 + j], 0), O - 1) : O - 1;  // (clamped: a bad label must not become a bad address)
    wm[k] = (wild && s < n && wild[(size_t)l0 + p + j] != 0) ? ~0u : 0u;
    skip_in[k] = lab && j >= 1 && labels[l0 + j] != labels[l0 + j - 1];
  }
  constexpr int PFD = 8;
  float pre[PFD][H], prb[PFD], prm[PFD];
  double off = 0.0;
  float a[R];
  int st[R];  // start frame of the best path into the state (state 0: unused)
  int en[H];  // per gap state: one past the last label frame of the best path into it = the frame it was entered at
#pragma unroll
  for (int r = 0; r < R; ++r) {
    a[r] = NEG;
    st[r] = 0;
    en[r >> 1] = 0;
  }
  if (lane == 0) {
    a[0] = wild_pick(wm[0], mu[0], zu[O - 1]);
    if (n > 1) a[1] = zu[lo[0]];
  }
#pragma unroll
  for (int j = 0; j < PFD; ++j) {
    const int row = min(1 + j, Tn - 1);
    const float* zr = zu + (size_t)row * ld;
    prb[j] = zr[O - 1];
    prm[j] = mu[row];
#pragma unroll
    for (int k = 0; k < H; ++k) pre[j][k] = zr[lo[k]];
  }
  for (int t0 = 1; t0 < Tn; t0 += PFD) {
#pragma unroll
    for (int j = 0; j < PFD; ++j) {
      const int t = t0 + j;
      const bool live = t < Tn;
      const int nrow = min(t + PFD, Tn - 1);
      float cur[R];
      {
        const float* zr = zu + (size_t)nrow * ld;
        const float cb = prb[j], cm = prm[j];
        prb[j] = zr[O - 1];
        prm[j] = mu[nrow];
#pragma unroll
        for (int k = 0; k < H; ++k) {
          cur[2 * k] = wild_pick(wm[k], cm, cb);
          cur[2 * k + 1] = pre[j][k];
          pre[j][k] = zr[lo[k]];
        }
      }
      const float up1 = lane_prev(a[R - 1], NEG, lane), up2 = lane_prev(a[R - 2], NEG, lane);
      const int us1 = lane_prev_int(st[R - 1], 0, lane), us2 = lane_prev_int(st[R - 2], 0, lane);
      float na[R];
      int ns[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float p1 = r >= 1 ? a[r - 1] : up1;
        const float p2 = r >= 2 ? a[r - 2] : (r == 1 ? up1 : up2);
        const int q1 = r == 1 ? (lane == 0 ? t : st[0]) : (r >= 1 ? st[r - 1] : us1);  // state 0 -> 1: the path starts here
        const int q2 = r >= 2 ? st[r - 2] : (r == 1 ? us1 : us2);
        float best = a[r];
        int bs = st[r];
        bool from1 = false;
        if (p1 > best) { best = p1; bs = q1; from1 = true; }
        if ((r & 1) && skip_in[r >> 1] && p2 > best) { best = p2; bs = q2; from1 = false; }
        const float v = (s0 + r < n) ? best + cur[r] : NEG;
        na[r] = live ? v : a[r];
        ns[r] = live ? bs : st[r];
        if (!(r & 1) && live && from1) en[r >> 1] = t;  // (a gap is entered from the label before it, whose last frame is t - 1)
      }
      if (j == PFD - 1) {  // compile-time: re-centre the state vector on its maximum
        float m = NEG;
#pragma unroll
        for (int r = 0; r < R; ++r) m = fmaxf(m, na[r]);
        m = wave_max(m);
        if (live && m > -1e29f) {
          off += (double)m;
#pragma unroll
          for (int r = 0; r < R; ++r) na[r] = fmaxf(na[r] - m, NEG);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        a[r] = na[r];
        st[r] = ns[r];
      }
    }
  }
  // the end state: n - 1 unless n - 2 is strictly larger
  float e1 = -INFINITY, e2 = -INFINITY;
  int b1 = -1, b2 = -1, f1 = -1;  // start frames of n - 1 / n - 2, end frame of n - 1: from the lanes that own them
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (s0 + r == n - 1) { e1 = a[r]; b1 = st[r]; f1 = en[r >> 1]; }
    if (s0 + r == n - 2) { e2 = a[r]; b2 = st[r]; }
  }
  e1 = wave_max(e1);
  e2 = wave_max(e2);
  for (int o = 32; o > 0; o >>= 1) {
    b1 = max(b1, __shfl_xor(b1, o));
    b2 = max(b2, __shfl_xor(b2, o));
    f1 = max(f1, __shfl_xor(f1, o));
  }
  const bool last_label = e2 > e1;
  const float vend = fmaxf(e1, e2);
  if (!(vend > -1e29f)) {  // too short for its labels: no path
    if (lane == 0) {
      score[p] = -INFINITY;
      start[p] = end[p] = -1;
    }
    return;
  }
  double ls = 0.0;
  for (int f = lane; f < Tn; f += 64) ls += (double)lse[r0 + f];
  for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o);
  if (lane == 0) {
    score[p] = (float)((off + (double)vend) - ls);
    start[p] = S == 0 ? 0 : (last_label ? b2 : b1);
    end[p] = S == 0 ? 0 : (last_label ? Tn : f1);
  }
}

// ---- expected label errors over an N-best list (MWER; the contract is stated in ctc.h and at tfk_accumulate_ctc_mwer) ----
//
// Every (utterance, hypothesis) pair -- and, under ctc_weight > 0, every (utterance, reference) -- is one "utterance" of a
// pair-level CtcBatch whose rows are the pair's own copy of its utterance's frames: ctc_alpha_beta_kernel runs on it unchanged.

// lp[prow[p] + f, s] = z[seg[u] + f, class(s)] - lse[seg[u] + f], u = pair_utt[p]: ctc_gather_kernel through the pair map
__global__ void __launch_bounds__(256)
ctc_pair_gather_kernel(CtcMwer m) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)m.PR * m.sext) return;
  const int pr = (int)(idx / m.sext), s = (int)(idx % m.sext);
  const int32_t* prow = ctc_mwer_prow(m);
  const int32_t* lab_off = ctc_mwer_lab_off(m);
  const int p = utt_of(prow, m.NP, pr);
  const int l0 = lab_off[p], n = 2 * (lab_off[p + 1] - l0) + 1;
  float v = NEG;
  if (s < n) {
    const size_t t = (size_t)(m.seg[ctc_mwer_pair_utt(m)[p]] + (pr - prow[p]));
    const int k = (s & 1) ? min(max(m.labels[l0 + (s >> 1)], 0), m.O - 1) : m.O - 1;  // (clamped: never a bad address)
    v = m.logits[t * m.ld + k] - m.lse[t];
  }
  m.lp[idx] = v;
}

// acc + v(lane 0) + v(lane 1) + ... + v(lane 63), one addition after the other: the same in every lane, in lane order
__device__ __forceinline__ double wave_add_in_order(double acc, double v) {
  for (int l = 0; l < 64; ++l) acc += __shfl(v, l);
  return acc;
}

// ONE WAVE PER UTTERANCE: the distribution over its list, the expected number of label errors and the weights of the
// gradient, in double and in pair order from the pairs' log Z:
//   p_i = exp(s_i - m) / sum_j exp(s_j - m) (m = the largest feasible s_j; an infeasible pair: p_i = 0),
//   R = sum_i p_i e_i,   w_i = p_i (e_i - R), rounded to float once;   no feasible pair: R = 0, w = 0
__global__ void __launch_bounds__(64)
ctc_mwer_weights_kernel(CtcMwer m) {
  const int u = blockIdx.x, lane = threadIdx.x;
  const int32_t* ufirst = ctc_mwer_ufirst(m);
  const int p0 = ufirst[u], p1 = ufirst[u + 1];
  double mx = -INFINITY;
  for (int p = p0 + lane; p < p1; p += 64)
    if (m.utt_loss[p] < INFINITY) mx = fmax(mx, m.logz[p]);
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  const bool any = mx > -INFINITY;
  double Z = 0.0;
  for (int q = p0; q < p1; q += 64) {
    const int p = q + lane;
    const double ex = (any && p < p1 && m.utt_loss[p] < INFINITY) ? exp(m.logz[p] - mx) : 0.0;
    Z = wave_add_in_order(Z, ex);
  }
  double R = 0.0;
  for (int q = p0; q < p1; q += 64) {
    const int p = q + lane;
    const double ex = (any && p < p1 && m.utt_loss[p] < INFINITY) ? exp(m.logz[p] - mx) : 0.0;
    R = wave_add_in_order(R, any && p < p1 ? ex / Z * (double)m.edits[p] : 0.0);
  }
  for (int p = p0 + lane; p < p1; p += 64) {
    const bool ok = any && m.utt_loss[p] < INFINITY;
    const double pi = ok ? exp(m.logz[p] - mx) / Z : 0.0;
    m.w[p] = (float)(pi * ((double)m.edits[p] - R));
    m.score[p] = m.utt_loss[p] < INFINITY ? (float)m.logz[p] : -INFINITY;
  }
  if (lane == 0) m.risk[u] = (float)R;
}

// ONE WAVE PER LOGITS ROW t = row0 + blockIdx.x of utterance u, frame f; dynamic LDS: the class row, then one pair's state
// posteriors.  row[c] = ctc_weight * softmax(z_t)[c] (only where the reference is feasible), then for the utterance's pairs
// in pair order, and last for its reference with the coefficient -ctc_weight:
//   gamma(s) exactly as ctc_grad_kernel forms it from the pair's rows (double exponent, divided by its sum where that is
//   within 1e-2 of one), row[class(s)] += coefficient * gamma(s)
// The fold: lane c % 64 owns class c and scans the pair's labels in label order, so every class sees its terms in the
// order ctc_grad_kernel's lane 0 adds them -- pairs, then labels; the blanks as there: lane-strided sums, then the butterfly --
// while the N * S serial LDS updates become N * S broadcast reads.  A pair with coefficient zero (a single hypothesis, an
// infeasible one) is skipped: its rows stay exactly zero.  No atomics: the same input gives the same bits.
__global__ void __launch_bounds__(64)
ctc_mwer_grad_kernel(CtcMwer m, int row0, float* __restrict__ dlogits, int ldd, Twin tw) {
  extern __shared__ float row[];
  float* g = row + m.ld;
  const int t = row0 + blockIdx.x, lane = threadIdx.x;
  const int u = utt_of(m.seg, m.U, t);
  const int f = t - m.seg[u];
  const int32_t* prow = ctc_mwer_prow(m);
  const int32_t* lab_off = ctc_mwer_lab_off(m);
  const int32_t* ufirst = ctc_mwer_ufirst(m);
  const int p0 = ufirst[u], nh = ufirst[u + 1] - p0;
  const bool ref_live = m.NP > m.P && m.utt_loss[m.P + u] < INFINITY;
  {
    // (read before anything is written: dlogits may be the logits themselves)
    const float* z = m.logits + (size_t)t * m.ld;
    const float l = m.lse[t];
    for (int c = lane; c < m.O; c += 64) row[c] = ref_live ? m.ctc_weight * expf(z[c] - l) : 0.f;
  }
  for (int i = 0; i < nh + (ref_live ? 1 : 0); ++i) {
    const int p = i < nh ? p0 + i : m.P + u;
    const float coef = i < nh ? m.w[p] : -m.ctc_weight;
    if (coef == 0.f || !(m.utt_loss[p] < INFINITY)) continue;  // (uniform over the wave)
    const int l0 = lab_off[p], S = lab_off[p + 1] - l0, n = 2 * S + 1;
    const size_t pr = (size_t)prow[p] + f;
    const double shift = m.off[pr] + m.offb[pr] - m.logz[p];
    const float* al = m.ab + pr * m.sext;
    const float* be = m.bb + pr * m.sext;
    const float* lp = m.lp + pr * m.sext;
    float tot = 0.f;
    for (int s = lane; s < n; s += 64) {
      g[s] = __expf((float)((double)al[s] + (double)be[s] - (double)lp[s] + shift));
      tot += g[s];
    }
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    const float inv = fabsf(tot - 1.f) < 1e-2f ? 1.f / tot : 1.f;
    for (int s = lane; s < n; s += 64) g[s] *= inv;
    __syncthreads();
    float blank = 0.f;
    for (int s = 2 * lane; s < n; s += 128) blank += g[s];
    for (int o = 32; o > 0; o >>= 1) blank += __shfl_xor(blank, o);
    for (int cb = 0; cb < m.O; cb += 64) {
      const int c = cb + lane;
      float acc = c < m.O ? row[c] : 0.f;
      if (c == m.O - 1) acc += coef * blank;
      for (int j = 0; j < S; ++j)
        if (m.labels[l0 + j] == c) acc += coef * g[2 * j + 1];
      if (c < m.O) row[c] = acc;
    }
    __syncthreads();
  }
  __syncthreads();
  float* dr = dlogits + (size_t)t * ldd;
  for (int c = lane; c < ldd; c += 64) dr[c] = c < m.O ? row[c] : 0.f;
  if (tw.p)
    for (int c = lane; c < ldd; c += 64) twin_put(tw, (size_t)t, c, c < m.O ? row[c] : 0.f);
}

// scalars[0] (+)= sum_u risk[u] (+ ctc_weight * the references' losses), scalars[1] (+)= labels, scalars[2] (+)= 1
__global__ void __launch_bounds__(256)
ctc_mwer_loss_reduce_kernel(const float* __restrict__ risk, const float* __restrict__ ref_loss, int U, float ctc_weight,
                            float labels, float* __restrict__ scalars, int overwrite) {
  __shared__ float sm[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < U; i += 256) s += ref_loss ? risk[i] + ctc_weight * ref_loss[i] : risk[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    scalars[0] = overwrite ? s : scalars[0] + s;
    scalars[1] = overwrite ? labels : scalars[1] + labels;
    scalars[2] = overwrite ? 1.f : scalars[2] + 1.f;
  }
}

// ---- MMI against a denominator graph: the exact sum over every label sequence a grammar accepts (the contract is stated at
// tfk_accumulate_ctc_mmi in tfkaldi_hip.h, the tables and the two phases of a frame at CtcDenGraph in ctc.h) ----

struct DenTab {
  const int32_t *fx, *bx, *g0, *ffirst, *fterm, *flo, *fhi, *bfirst, *bterm, *blo, *bhi, *cfirst;
};
__host__ __device__ inline DenTab den_tab(const int32_t* t, int S, int A, int K) {
  DenTab d;
  d.fx = t;                    d.bx = d.fx + A;             d.g0 = d.bx + A;
  d.ffirst = d.g0 + S + 1;     d.fterm = d.ffirst + S + 1;  d.flo = d.fterm + A;  d.fhi = d.flo + K;
  d.bfirst = d.fhi + K;        d.bterm = d.bfirst + S + 1;  d.blo = d.bterm + A;  d.bhi = d.blo + K;
  d.cfirst = d.bhi + K;
  return d;
}

// wexp[i] = exp(lm_scale * logw[i]) for the A arc weights and the S final weights (-inf: exactly 0, also at lm_scale = 0)
__global__ void __launch_bounds__(256)
ctc_den_prep_kernel(CtcDen d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.A + d.S) return;
  const float w = d.logw[i];
  d.wexp[i] = w > -INFINITY ? (float)exp((double)d.lm_scale * (double)w) : 0.f;
}

constexpr int kDenPF = 4;  // rows of the softmax in flight ahead of the chain

// the power of two that brings m into [1, 2), as (factor, its binary exponent): exact in fp32, so the offset (a count of
// binary exponents) says exactly what the stored values were multiplied by.  m == 0 (no path survives) or not finite: (1, 0)
__device__ __forceinline__ float den_scale(float m, int* e) {
  const int eb = (__builtin_bit_cast(int, m) >> 23) & 0xff;
  const bool ok = m > 0.f && eb != 0xff;
  *e = ok ? eb - 127 : 0;
  return ok ? __builtin_bit_cast(float, (254 - eb) << 23) : 1.f;
}

// phase 1 of a frame: thread per graph state g, sums[g] = v[B_g] + every term, sums[S + k] = v[B_g] + the terms outside
// group k's own [lo, hi) -- a suffix recorded on the way down, then a prefix added on the way up
template <int NT, bool BWD>
__device__ __forceinline__ void den_phase1(const float* v, float* sums, const float* __restrict__ wexp, int S,
                                           const int32_t* __restrict__ g0, const int32_t* __restrict__ first,
                                           const int32_t* __restrict__ term, const int32_t* __restrict__ lo,
                                           const int32_t* __restrict__ hi) {
  for (int g = threadIdx.x; g < S; g += NT) {
    const int j0 = first[g], j1 = first[g + 1], k0 = g0[g], k1 = g0[g + 1];
    const float self = v[g];
    if (k1 - k0 == 1 && lo[k0] == j0 && hi[k0] == j1) {  // one group that is every term (a trie, an n-gram): a select
      float tot = 0.f;
      for (int j = j0; j < j1; ++j) {
        const int a = term[j];
        tot += BWD ? wexp[a] * v[S + a] : v[S + a];
      }
      sums[S + k0] = self;
      sums[g] = self + tot;
      continue;
    }
    if (k1 > k0) {
      float suf = 0.f;
      int k = k1 - 1;
      for (int j = j1 - 1; j >= j0; --j) {
        while (k >= k0 && hi[k] > j) sums[S + k--] = suf;
        const int a = term[j];
        suf += BWD ? wexp[a] * v[S + a] : v[S + a];
      }
      while (k >= k0) sums[S + k--] = suf;
    }
    float pre = 0.f;
    int k = k0;
    for (int j = j0; j < j1; ++j) {
      for (; k < k1 && lo[k] <= j; ++k) sums[S + k] = self + (pre + sums[S + k]);
      const int a = term[j];
      pre += BWD ? wexp[a] * v[S + a] : v[S + a];
    }
    for (; k < k1; ++k) sums[S + k] = self + (pre + sums[S + k]);
    sums[g] = self + pre;
  }
}

template <int NT>
__device__ __forceinline__ void den_block_max(float mx, float* wmax) {
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
}

// One direction of one utterance on one workgroup.  v [N]: the running vector, sums [S + K]: phase 1's results -- both in LDS
// or both in the workgroup's own global scratch; prow [O] and wmax [NT / 64] in LDS.
// Forward: v_{-1} = 1 at B_start, frame t: B_g <- p(blank) sums[g], L_a <- p(c_a) (v[L_a] + w_a sums[fx(a)]); at the end
// Z = sum_g f_g sums[g] of one more phase 1.  Backward: v_T = f_g at B_g, frame t: B_g <- p(blank) sums[g] (terms w_a v[L_a]),
// L_a <- p(c_a) (v[L_a] + sums[bx(a)]) -- beta with the emission of its own frame, as ctc_alpha_beta_kernel has it.
template <int NT, bool BWD>
__device__ __forceinline__ void den_sweep_body(const CtcDen& d, int u, float* v, float* sums, float* prow, float* wmax,
                                               double* zpart, const int32_t* tab, const float* wexp) {
  const int tid = threadIdx.x;
  const int r0 = d.seg[u], Tn = d.seg[u + 1] - r0;
  const int S = d.S, N = d.N, O = d.O;
  const float* fexp = wexp + d.A;
  const float* __restrict__ fexp_g = d.wexp + d.A;  // (the global copy: what may be read before the first barrier)
  if (Tn <= 0) {  // an utterance without frames: only the empty sequence, accepted if the start is final
    if (!BWD && tid == 0)
      d.logz[u] = fexp_g[d.start] > 0.f ? (double)d.lm_scale * (double)d.logw[d.A + d.start] : -(double)INFINITY;
    return;
  }
  const DenTab tb = den_tab(tab, S, d.A, d.K);
  const int32_t* __restrict__ first = BWD ? tb.bfirst : tb.ffirst;
  const int32_t* __restrict__ term = BWD ? tb.bterm : tb.fterm;
  const int32_t* __restrict__ lo = BWD ? tb.blo : tb.flo;
  const int32_t* __restrict__ hi = BWD ? tb.bhi : tb.fhi;
  const int32_t* __restrict__ ax = BWD ? tb.bx : tb.fx;
  float* __restrict__ rows = (BWD ? d.vb : d.va) + (size_t)r0 * d.stride;
  double* __restrict__ offs = (BWD ? d.offb : d.offa) + r0;
  {
    float mx = 0.f;
    for (int i = tid; i < N; i += NT) {
      const float x = BWD ? (i < S ? fexp_g[i] : 0.f) : (i == d.start ? 1.f : 0.f);
      v[i] = x;
      mx = fmaxf(mx, x);
    }
    den_block_max<NT>(mx, wmax);
  }
  // The chain is Tn dependent frames; a row of the softmax takes longer to arrive than a frame of a small graph lasts, so
  // kDenPF rows are in flight in registers (one class per thread), with clamped row indices instead of guards.
  const float* pbase = d.post + (size_t)r0 * d.ld + min(tid, O - 1);
  float pre[kDenPF];
#pragma unroll
  for (int j = 0; j < kDenPF; ++j) {
    const int n = min(j, Tn - 1);
    pre[j] = pbase[(size_t)(BWD ? Tn - 1 - n : n) * d.ld];
  }
  long long eacc = 0;  // the offset in binary exponents: off = eacc * ln 2
  __syncthreads();
  for (int n0 = 0; n0 < Tn; n0 += kDenPF) {
#pragma unroll
    for (int j = 0; j < kDenPF; ++j) {
      const int n = n0 + j;
      const float cur = pre[j];
      {
        const int nn = min(n + kDenPF, Tn - 1);
        pre[j] = pbase[(size_t)(BWD ? Tn - 1 - nn : nn) * d.ld];
      }
      if (n < Tn) {  // (uniform over the workgroup)
        const int t = BWD ? Tn - 1 - n : n;
        float m = wmax[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, wmax[w]);
        int e;
        const float scale = den_scale(m, &e);
        eacc += e;
        if (tid < O) prow[tid] = cur;
        den_phase1<NT, BWD>(v, sums, wexp, S, tb.g0, first, term, lo, hi);
        __syncthreads();
        const float pb = prow[O - 1] * scale;
        float mx = 0.f;
        float* __restrict__ row = rows + (size_t)t * d.stride;
        for (int i = tid; i < N; i += NT) {
          float nv;
          if (i < S) {
            nv = pb * sums[i];
          } else {
            const int a = i - S;
            const uint32_t wd = (uint32_t)ax[a];
            const float in = sums[wd & 0xffffu];
            nv = (prow[wd >> 16] * scale) * (v[i] + (BWD ? in : wexp[a] * in));
          }
          v[i] = nv;
          row[i] = nv;
          mx = fmaxf(mx, nv);
        }
        den_block_max<NT>(mx, wmax);
        if (tid == 0) offs[t] = (double)eacc * 0.6931471805599453;
        __syncthreads();
      }
    }
  }
  if (BWD) return;
  den_phase1<NT, false>(v, sums, wexp, S, tb.g0, first, term, lo, hi);
  __syncthreads();
  double z = 0.0;  // fixed order: thread-strided, the butterfly, then the waves one after the other
  for (int g = tid; g < S; g += NT) z += (double)fexp[g] * (double)sums[g];
  for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o);
  if ((tid & 63) == 0) zpart[tid >> 6] = z;
  __syncthreads();
  if (tid == 0) {
    z = 0.0;
    for (int w = 0; w < NT / 64; ++w) z += zpart[w];
    d.logz[u] = z > 0.0 ? (double)eacc * 0.6931471805599453 + log(z) : -(double)INFINITY;
  }
}

// blockIdx.x: the utterance; blockIdx.y = 0: the forward sweep and log Z, 1 (gradient only): the backward sweep -- two
// independent workgroups of one launch, as ctc_alpha_beta_kernel's two waves
template <int NT, bool LDS>
__global__ void __launch_bounds__(NT)
ctc_den_sweep_kernel(CtcDen d) {
  extern __shared__ float den_lds[];
  __shared__ float wmax[NT / 64];
  __shared__ double zpart[NT / 64];
  const int u = blockIdx.x, wg = blockIdx.y * d.U + blockIdx.x;
  float* prow = den_lds;
  const int orow = (d.O + 63) & ~63;
  float* v = LDS ? den_lds + orow : d.gv + (size_t)wg * d.stride;
  float* sums = LDS ? den_lds + orow + d.N : d.gs + (size_t)wg * (d.S + d.K);
  // The index tables and the weights are the same at every frame, and a frame of a small graph is a handful of DEPENDENT
  // loads of them: where they fit beside the vector they are copied into LDS once (generic pointers from here on: the
  // loads are flat instructions, which serve both address spaces).  The barrier that follows the initial vector covers them.
  const int32_t* tab = d.tab;
  const float* wexp = d.wexp;
  if (LDS && d.tab_lds) {
    const int words = 4 * d.A + 3 * (d.S + 1) + 4 * d.K + d.O;
    int32_t* lt = reinterpret_cast<int32_t*>(den_lds + orow + d.N + d.S + d.K);
    float* lw = reinterpret_cast<float*>(lt + words);
    for (int i = threadIdx.x; i < words; i += NT) lt[i] = d.tab[i];
    for (int i = threadIdx.x; i < d.A + d.S; i += NT) lw[i] = d.wexp[i];
    tab = lt;
    wexp = lw;
  }
  if (blockIdx.y == 0) den_sweep_body<NT, false>(d, u, v, sums, prow, wmax, zpart, tab, wexp);
  else den_sweep_body<NT, true>(d, u, v, sums, prow, wmax, zpart, tab, wexp);
}

// utt_loss[u] = -(log p_ctc(y_u) + lm_scale G(y_u)) + log Z_u in double, rounded once; +inf where the reference does not fit
// its frames, the graph rejects it, or no accepted sequence fits the frames
__global__ void __launch_bounds__(256)
ctc_den_loss_kernel(CtcDen d, const double* __restrict__ num_logz, const float* __restrict__ num_loss,
                    float* __restrict__ logz_out) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= d.U) return;
  const bool ok = num_loss[u] < INFINITY && d.logz[u] > -INFINITY && d.gy[u] > -INFINITY;
  if (logz_out) logz_out[u] = (float)d.logz[u];
  d.utt_loss[u] = ok ? (float)(-(num_logz[u] + (double)d.lm_scale * d.gy[u]) + d.logz[u]) : INFINITY;
}

// One workgroup of four waves per logits row t; dynamic LDS: occ [O].  Class c's composed states are contiguous (the blank:
// the S states B_g; label c: arcs [cfirst[c], cfirst[c + 1])), so occ[c] = sum over them of alpha_t beta_t e^(offa + offb -
// log Z) / p_t(c) is a segmented sum in a fixed order: wave c % 4 takes class c, lane-strided, then the butterfly.  The
// product is formed in double (alpha and beta are each relative to their own offset, and the exponent can be large where the
// two sweeps put their mass on different states).  occ is divided by its sum where that is within 1e-2 of one, as
// ctc_grad_kernel does and for its reasons.
__global__ void __launch_bounds__(256)
ctc_den_grad_kernel(CtcDen d, const float* g, int ldg, int row0, float* dlogits, int ldd, Twin tw) {
  extern __shared__ float occ[];
  __shared__ float inv_s;
  const int t = row0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u = utt_of(d.seg, d.U, t);
  const bool live = d.utt_loss[u] < INFINITY;
  const float* pr = d.post + (size_t)t * d.ld;
  if (live) {  // (uniform)
    const DenTab tb = den_tab(d.tab, d.S, d.A, d.K);
    const double sc = exp(d.offa[t] + d.offb[t] - d.logz[u]);
    const float* al = d.va + (size_t)t * d.stride;
    const float* be = d.vb + (size_t)t * d.stride;
    for (int c = wave; c < d.O; c += 4) {
      const int i0 = c == d.O - 1 ? 0 : d.S + tb.cfirst[c];
      const int i1 = c == d.O - 1 ? d.S : d.S + tb.cfirst[c + 1];
      float acc = 0.f;
      for (int i = i0 + lane; i < i1; i += 64) acc += (float)((double)al[i] * (double)be[i] * sc);
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
      const float p = pr[c];
      if (lane == 0) occ[c] = p > 0.f ? acc / p : 0.f;
    }
    __syncthreads();
    if (wave == 0) {
      float tot = 0.f;
      for (int c = lane; c < d.O; c += 64) tot += occ[c];
      for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
      if (lane == 0) inv_s = fabsf(tot - 1.f) < 1e-2f ? 1.f / tot : 1.f;
    }
    __syncthreads();
  }
  const float inv = live ? inv_s : 0.f, k = 1.f + d.ctc_weight;
  const float* gr = g + (size_t)t * ldg;
  float* dr = dlogits + (size_t)t * ldd;
  for (int c = tid; c < ldd; c += 256) {
    // (read before the write: dlogits may be g itself)
    const float x = (live && c < d.O) ? (occ[c] * inv - pr[c]) + k * gr[c] : 0.f;
    dr[c] = x;
    if (tw.p) twin_put(tw, (size_t)t, c, x);
  }
}

}  // namespace

int ctc_state_stride(int max_labels) { return 64 * regs_for(max_labels); }

static void loss_grad(hipStream_t s, const CtcBatch& b, float* dlogits, int ldd, int row0, int rows, int with_grad, Twin tw) {
  if (b.T <= 0 || b.U <= 0) return;
  hipLaunchKernelGGL(ctc_softmax_kernel, dim3(b.T), dim3(256), 0, s, b.logits, b.O, b.ld, b.post, b.lse);
  const size_t n = (size_t)b.T * b.sext;
  if (b.wild) hipLaunchKernelGGL(ctc_gather_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b);
  else hipLaunchKernelGGL(ctc_gather_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, b);
  const dim3 grid(b.U, with_grad ? 2 : 1);
  switch (b.sext / 64) {
    case 2: hipLaunchKernelGGL(ctc_alpha_beta_kernel<2>, grid, dim3(64), 0, s, b); break;
    case 4: hipLaunchKernelGGL(ctc_alpha_beta_kernel<4>, grid, dim3(64), 0, s, b); break;
    case 8: hipLaunchKernelGGL(ctc_alpha_beta_kernel<8>, grid, dim3(64), 0, s, b); break;
    default: hipLaunchKernelGGL(ctc_alpha_beta_kernel<16>, grid, dim3(64), 0, s, b); break;
  }
  if (!with_grad || rows <= 0) return;
  const size_t lds = (size_t)(b.ld + b.sext) * sizeof(float);
  if (b.wild || ldd != b.ld || row0 != 0 || rows != b.T)
    hipLaunchKernelGGL(ctc_grad_wild_kernel, dim3(rows), dim3(64), lds, s, b, dlogits, ldd, row0, tw);
  else
    hipLaunchKernelGGL(ctc_grad_kernel, dim3(b.T), dim3(64), lds, s, b, dlogits, tw);
}

void ctc_loss_grad(hipStream_t s, const CtcBatch& b, float* dlogits, int with_grad, Twin tw) {
  loss_grad(s, b, dlogits, b.ld, 0, b.T, with_grad, tw);
}

void ctc_loss_grad_rows(hipStream_t s, const CtcBatch& b, float* dlogits, int ldd, int row0, int rows, int with_grad) {
  loss_grad(s, b, dlogits, ldd, row0, rows, with_grad, Twin());
}

void ctc_loss_reduce(hipStream_t s, const float* utt_loss, const int32_t* lab_off, int U, float* scalars,
                     bool overwrite) {
  hipLaunchKernelGGL(ctc_loss_reduce_kernel, dim3(1), dim3(256), 0, s, utt_loss, lab_off, U, scalars, overwrite ? 1 : 0);
}

void ctc_best_path(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U, int32_t* cls,
                   int32_t* hyp, int32_t* hyp_len) {
  if (T > 0) hipLaunchKernelGGL(ctc_row_argmax_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, logits, ld, O, T, cls);
  if (U > 0) hipLaunchKernelGGL(ctc_merge_kernel, dim3(U), dim3(64), 0, s, cls, seg, O - 1, hyp, hyp_len);
}

size_t ctc_beam_scratch_words(int T, int U, int W) { return 2 * (size_t)T * (size_t)W + 64 * (size_t)U; }

const char* ctc_beam_limits(int O, int T, int U, int W, int top_paths) {
  if (W < 1 || W > kCtcBeamMaxWidth) return "beam_width outside [1, 128]";
  if (O < 2 || O > kCtcBeamMaxClasses) return "output_dim outside [2, 64] (63 labels + blank)";
  if (top_paths < 1 || top_paths > W) return "top_paths outside [1, beam_width]";
  if (T < 0 || T > kCtcBeamMaxFrames) return "more than 524286 frames";
  if (U < 0 || U > (1 << 20)) return "more than 1048576 utterances";
  return nullptr;
}

int ctc_lm_contexts(int O, int order) {
  int C = 1;
  for (int n = 1; n < order; ++n) C *= O;
  return C;
}

// which instantiation a search is, and the model arguments its kernel receives (no model: no table, one context)
static int beam_kind(const CtcLm* lm) { return !lm ? kBeamAm : lm->next ? kBeamGraph : kBeamNgram; }
static BeamModel beam_model(const CtcLm* lm, int O) {
  if (!lm) return {nullptr, 1, 0.f, 0.f, 0, nullptr, 0};
  if (lm->next) return {lm->table, lm->num_states, lm->weight, lm->bonus, (int)lm->eos, lm->next, lm->start};
  return {lm->table, ctc_lm_contexts(O, lm->order), lm->weight, lm->bonus, (int)lm->eos, nullptr, 0};
}

void ctc_beam_search(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U, int W,
                     int top_paths, unsigned long long* trie, int32_t* hyp, int32_t* hyp_len, float* score, const CtcLm* lm,
                     float* am_score) {
  if (U <= 0) return;
  (void)hipMemsetAsync(trie, 0xff, ctc_beam_scratch_words(T, U, W) * sizeof(unsigned long long), s);
  const int kind = beam_kind(lm);
  const BeamModel m = beam_model(lm, O);
  // (am_score: NULL without a model, the value this launch has always passed; the acoustic kernel never reads the argument)
  hipLaunchKernelGGL(kind == kBeamGraph ? ctc_beam_kernel<kBeamGraph>
                     : kind == kBeamNgram ? ctc_beam_kernel<kBeamNgram> : ctc_beam_kernel<kBeamAm>,
                     dim3(U), dim3(kBeamThreads), 0, s, logits, ld, O, seg, U, T, W, top_paths, trie, hyp, hyp_len, score,
                     m.table, m.C, m.weight, m.bonus, m.eos, lm ? am_score : nullptr, m.next, m.start, BeamResume{});
}

size_t ctc_beam_topk_scratch_words(int T) { return (size_t)(T > 0 ? T : 0) * kCtcTopkRowWords; }

const char* ctc_beam_topk_limits(int O, int T, int U, int W, int top_paths, int label_topk) {
  if (W < 1 || W > kCtcBeamMaxWidth) return "beam_width outside [1, 128]";
  if (O < 2 || O > kCtcTopkMaxClasses) return "output_dim outside [2, 65536]";
  if (label_topk < 1 || label_topk > kCtcTopkMaxLabels) return "label_topk outside [1, 63]";
  if (top_paths < 1 || top_paths > W) return "top_paths outside [1, beam_width]";
  if (T < 0 || T > kCtcBeamMaxFrames) return "more than 524286 frames";
  if (U < 0 || U > (1 << 20)) return "more than 1048576 utterances";
  return nullptr;
}

size_t ctc_lm_entries(int O, int order) {
  size_t n = 1;
  for (int i = 0; i < order && n <= kCtcLmMaxEntries; ++i) n *= (size_t)O;
  return n;
}

void ctc_beam_topk_rows(hipStream_t s, const float* logits, int ld, int O, int T, int label_topk, uint32_t* pre) {
  if (T <= 0) return;
  hipLaunchKernelGGL(ctc_row_topk_kernel, dim3((unsigned)T), dim3(64), 0, s, logits, ld, O, min(label_topk, O - 1), pre);
}

void ctc_beam_topk_search(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U, int W,
                          int top_paths, int label_topk, unsigned long long* trie, const uint32_t* pre, int32_t* hyp,
                          int32_t* hyp_len, float* score, const CtcLm* lm, float* am_score) {
  if (U <= 0) return;
  const int K = min(label_topk, O - 1);
  (void)hipMemsetAsync(trie, 0xff, ctc_beam_scratch_words(T, U, W) * sizeof(unsigned long long), s);
  const int kind = beam_kind(lm);
  const BeamModel m = beam_model(lm, O);
  hipLaunchKernelGGL(kind == kBeamGraph ? ctc_beam_topk_kernel<kBeamGraph>
                     : kind == kBeamNgram ? ctc_beam_topk_kernel<kBeamNgram> : ctc_beam_topk_kernel<kBeamAm>,
                     dim3(U), dim3(kBeamThreads), 0, s, logits, ld, O, K, pre, seg, U, T, W, top_paths, trie, hyp, hyp_len,
                     score, m.table, m.C, m.weight, m.bonus, m.eos, am_score, m.next, m.start, BeamResume{});
}

static size_t stream_lane_words(const CtcStreamState& st) { return ctc_beam_scratch_words(st.max_frames, 1, st.W); }

void ctc_stream_reset(hipStream_t s, const CtcStreamState& st, int lane) {
  const size_t first = lane < 0 ? 0 : (size_t)lane, n = lane < 0 ? (size_t)st.lanes : 1;
  (void)hipMemsetAsync(st.trie + first * stream_lane_words(st), 0xff, n * stream_lane_words(st) * sizeof(unsigned long long), s);
  (void)hipMemsetAsync(st.hdr + first * kCtcStreamHdrWords, 0, n * kCtcStreamHdrWords * sizeof(int32_t), s);
}

void ctc_stream_push(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, const CtcStreamState& st,
                     int label_topk, const uint32_t* pre, const CtcLm* lm) {
  const int kind = beam_kind(lm);
  const BeamModel m = beam_model(lm, O);
  const BeamResume rs = {st.hdr, st.arr, st.max_frames};
  if (label_topk) {
    auto* const kernel = kind == kBeamGraph   ? (ctc_beam_topk_kernel<kBeamGraph, true>)
                         : kind == kBeamNgram ? (ctc_beam_topk_kernel<kBeamNgram, true>)
                                              : (ctc_beam_topk_kernel<kBeamAm, true>);
    hipLaunchKernelGGL(kernel, dim3(st.lanes), dim3(kBeamThreads), 0, s, logits, ld, O, min(label_topk, O - 1), pre, seg, st.lanes, T,
                       st.W, 0, st.trie, nullptr, nullptr, nullptr, m.table, m.C, m.weight, m.bonus, 0, nullptr, m.next,
                       m.start, rs);
  } else {
    auto* const kernel = kind == kBeamGraph   ? (ctc_beam_kernel<kBeamGraph, true>)
                         : kind == kBeamNgram ? (ctc_beam_kernel<kBeamNgram, true>)
                                              : (ctc_beam_kernel<kBeamAm, true>);
    hipLaunchKernelGGL(kernel, dim3(st.lanes), dim3(kBeamThreads), 0, s, logits, ld, O, seg, st.lanes, T, st.W, 0, st.trie, nullptr,
                       nullptr, nullptr, m.table, m.C, m.weight, m.bonus, 0, nullptr, m.next, m.start, rs);
  }
}

void ctc_stream_result(hipStream_t s, const CtcStreamState& st, int kind, bool eos, bool pruned, int top_paths, int stride,
                       int32_t* hyp, int32_t* hyp_len, float* score, float* am_score) {
  hipLaunchKernelGGL(ctc_stream_result_kernel, dim3(st.lanes), dim3(kBeamThreads), 0, s, st.hdr, st.arr, st.trie, st.lanes, st.W,
                     st.max_frames, kind, eos ? 1 : 0, pruned ? 16 : 6, top_paths, stride, hyp, hyp_len, score, am_score);
}

// scratch of ctc_viterbi_align: [back-pointer rows T x bp_row_bytes(R) | row log-sum-exps T floats]
size_t ctc_align_scratch_bytes(int T, int max_labels) {
  return (size_t)(T > 0 ? T : 0) * ((size_t)bp_row_bytes(regs_for(max_labels)) + sizeof(float));
}

const char* ctc_align_limits(int O, int T, int U, int max_labels) {
  if (O < 2) return "output_dim < 2 (one label + blank)";
  if (max_labels < 0) return "a negative length";
  if (max_labels > kCtcMaxLabels) return "more than 511 labels in one utterance";
  if (T < 0 || T > kCtcAlignMaxFrames) return "more than 8388607 frames";
  if (U < 0 || U > (1 << 20)) return "more than 1048576 utterances";
  return nullptr;
}

void ctc_viterbi_align(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U,
                       const int32_t* labels, const int32_t* lab_off, int max_labels, void* scratch, int32_t* ali,
                       float* score) {
  if (U <= 0) return;
  const int R = regs_for(max_labels);
  unsigned char* bp = static_cast<unsigned char*>(scratch);
  float* lse = reinterpret_cast<float*>(bp + (size_t)(T > 0 ? T : 0) * bp_row_bytes(R));
  if (T > 0) hipLaunchKernelGGL(ctc_row_lse_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, logits, ld, O, T, lse);
  switch (R) {
    case 2: hipLaunchKernelGGL(ctc_viterbi_kernel<2>, dim3(U), dim3(64), 0, s, logits, ld, O, seg, labels, lab_off, lse, bp, ali, score); break;
    case 4: hipLaunchKernelGGL(ctc_viterbi_kernel<4>, dim3(U), dim3(64), 0, s, logits, ld, O, seg, labels, lab_off, lse, bp, ali, score); break;
    case 8: hipLaunchKernelGGL(ctc_viterbi_kernel<8>, dim3(U), dim3(64), 0, s, logits, ld, O, seg, labels, lab_off, lse, bp, ali, score); break;
    default: hipLaunchKernelGGL(ctc_viterbi_kernel<16>, dim3(U), dim3(64), 0, s, logits, ld, O, seg, labels, lab_off, lse, bp, ali, score); break;
  }
}

size_t ctc_score_scratch_bytes(int T) { return (size_t)(T > 0 ? T : 0) * sizeof(float); }

const char* ctc_score_limits(int O, int T, int U, int P, int max_labels) {
  if (O < 2) return "output_dim < 2 (one label + blank)";
  if (max_labels < 0) return "a negative length";
  if (max_labels > kCtcMaxLabels) return "more than 511 labels in one hypothesis";
  if (T < 0 || T > kCtcAlignMaxFrames) return "more than 8388607 frames";
  if (U < 0 || U > (1 << 20)) return "more than 1048576 utterances";
  if (P < 0 || P > kCtcScoreMaxPairs) return "more than 1048576 (utterance, hypothesis) pairs";
  return nullptr;
}

void ctc_score(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U,
               const int32_t* pair_utt, int P, const int32_t* labels, const int32_t* lab_off, int max_labels, void* scratch,
               float* score) {
  if (P <= 0 || U <= 0) return;
  float* lse = static_cast<float*>(scratch);
  if (T > 0) hipLaunchKernelGGL(ctc_row_lse_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, logits, ld, O, T, lse);
  switch (regs_for(max_labels)) {
    case 2: hipLaunchKernelGGL(ctc_score_kernel<2>, dim3(P), dim3(64), 0, s, logits, ld, O, seg, U, pair_utt, labels, lab_off, lse, score); break;
    case 4: hipLaunchKernelGGL(ctc_score_kernel<4>, dim3(P), dim3(64), 0, s, logits, ld, O, seg, U, pair_utt, labels, lab_off, lse, score); break;
    case 8: hipLaunchKernelGGL(ctc_score_kernel<8>, dim3(P), dim3(64), 0, s, logits, ld, O, seg, U, pair_utt, labels, lab_off, lse, score); break;
    default: hipLaunchKernelGGL(ctc_score_kernel<16>, dim3(P), dim3(64), 0, s, logits, ld, O, seg, U, pair_utt, labels, lab_off, lse, score); break;
  }
}

// scratch of ctc_viterbi_align_wild: [back-pointer rows T x bp_row_bytes(R) | row log-sum-exps T floats | row maxima T floats]
size_t ctc_align_wild_scratch_bytes(int T, int max_labels) {
  return (size_t)(T > 0 ? T : 0) * ((size_t)bp_row_bytes(regs_for(max_labels)) + 2 * sizeof(float));
}

void ctc_viterbi_align_wild(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U,
                            const int32_t* labels, const int32_t* lab_off, const uint8_t* wild, int max_labels,
                            void* scratch, int32_t* ali, float* score, float* free_score) {
  if (U <= 0) return;
  const int R = regs_for(max_labels);
  const size_t rows = (size_t)(T > 0 ? T : 0);
  unsigned char* bp = static_cast<unsigned char*>(scratch);
  float* lse = reinterpret_cast<float*>(bp + rows * bp_row_bytes(R));
  float* mx = lse + rows;
  if (T > 0)
    hipLaunchKernelGGL(ctc_row_max_lse_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, logits, ld, O, T, mx, lse);
  hipLaunchKernelGGL(ctc_free_score_kernel, dim3(U), dim3(64), 0, s, seg, mx, lse, free_score);
#define TFK_WILD(RR) \
  hipLaunchKernelGGL(ctc_viterbi_wild_kernel<RR>, dim3(U), dim3(64), 0, s, logits, ld, O, seg, labels, lab_off, wild, mx, lse, \
                     bp, ali, score)
  switch (R) {
    case 2: TFK_WILD(2); break;
    case 4: TFK_WILD(4); break;
    case 8: TFK_WILD(8); break;
    default: TFK_WILD(16); break;
  }
#undef TFK_WILD
}

// scratch of ctc_spot: [row log-sum-exps T floats | row maxima T floats]
size_t ctc_spot_scratch_bytes(int T) { return (size_t)(T > 0 ? T : 0) * 2 * sizeof(float); }

void ctc_spot(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U, const int32_t* pair_utt,
              int P, const int32_t* labels, const int32_t* lab_off, const uint8_t* wild, int max_labels, void* scratch,
              float* score, int32_t* start, int32_t* end, float* free_score) {
  if (U <= 0) return;
  float* lse = static_cast<float*>(scratch);
  float* mx = lse + (size_t)(T > 0 ? T : 0);
  if (T > 0)
    hipLaunchKernelGGL(ctc_row_max_lse_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, logits, ld, O, T, mx, lse);
  hipLaunchKernelGGL(ctc_free_score_kernel, dim3(U), dim3(64), 0, s, seg, mx, lse, free_score);
  if (P <= 0) return;
#define TFK_SPOT(RR) \
  hipLaunchKernelGGL(ctc_spot_kernel<RR>, dim3(P), dim3(64), 0, s, logits, ld, O, seg, U, pair_utt, labels, lab_off, wild, mx, \
                     lse, score, start, end)
  switch (regs_for(max_labels)) {
    case 2: TFK_SPOT(2); break;
    case 4: TFK_SPOT(4); break;
    case 8: TFK_SPOT(8); break;
    default: TFK_SPOT(16); break;
  }
#undef TFK_SPOT
}

const char* ctc_mwer_limits(int O, int64_t ld, int T, int U, int P, int max_labels, int64_t PR) {
  if (O < 2) return "output_dim < 2 (one label + blank)";
  if (max_labels < 0) return "a negative length";
  if (max_labels > kCtcMaxLabels) return "more than 511 labels in one hypothesis or reference";
  if (T < 0 || T > kCtcAlignMaxFrames) return "more than 8388607 frames";
  if (U < 0 || U > (1 << 20)) return "more than 1048576 utterances";
  if (P < 0 || P > kCtcScoreMaxPairs) return "more than 1048576 (utterance, hypothesis) pairs";
  const int64_t sext = ctc_state_stride(max_labels);
  if (PR < 0 || PR * sext > kCtcMwerMaxStates)
    return "more than 2^33 lattice states (frames x hypotheses x padded states per frame) in one call";
  if (ld < O || (ld + sext) * (int64_t)sizeof(float) > kCtcMwerMaxLds)
    return "the class row and the state row of one frame exceed 64 KiB of LDS";
  return nullptr;
}

size_t ctc_mwer_table_words(int U, int P, int NP) { return 3 * (size_t)NP + 2 + (size_t)U + 1 + 2 * (size_t)P; }

void ctc_mwer_table(const int32_t* utt_len, int U, const int32_t* hyp_count, const int32_t* hyp_len, const int32_t* ref_len,
                    bool with_ref, int32_t* tab) {
  int P = 0;
  for (int u = 0; u < U; ++u) P += hyp_count[u];
  const int NP = with_ref ? P + U : P;
  int32_t* prow = tab;
  int32_t* lab_off = prow + NP + 1;
  int32_t* pair_utt = lab_off + NP + 1;
  int32_t* ufirst = pair_utt + NP;
  int32_t* ref_at = ufirst + U + 1;
  int32_t* ref_cnt = ref_at + P;
  int32_t hyp_total = 0;
  for (int p = 0; p < P; ++p) hyp_total += hyp_len[p];
  prow[0] = lab_off[0] = ufirst[0] = 0;
  int p = 0;
  int32_t ref_first = hyp_total;
  for (int u = 0; u < U; ++u) {
    for (int h = 0; h < hyp_count[u]; ++h, ++p) {
      pair_utt[p] = u;
      prow[p + 1] = prow[p] + utt_len[u];
      lab_off[p + 1] = lab_off[p] + hyp_len[p];
      ref_at[p] = ref_first;
      ref_cnt[p] = ref_len[u];
    }
    ufirst[u + 1] = p;
    ref_first += ref_len[u];
  }
  for (int u = 0; with_ref && u < U; ++u) {
    pair_utt[P + u] = u;
    prow[P + u + 1] = prow[P + u] + utt_len[u];
    lab_off[P + u + 1] = lab_off[P + u] + ref_len[u];
  }
}

size_t ctc_mwer_scratch_bytes(int T, int NP, int P, int64_t PR, int sext) {
  const size_t rows = (size_t)PR, t = (size_t)(T > 0 ? T : 0);
  return (2 * rows + (size_t)NP) * sizeof(double) + (3 * rows * (size_t)sext + t + (size_t)NP + (size_t)P) * sizeof(float) + 16;
}

void ctc_mwer_carve(void* scratch, CtcMwer* m) {
  const size_t rows = (size_t)m->PR;
  double* d = static_cast<double*>(scratch);
  m->off = d;
  m->offb = d + rows;
  m->logz = d + 2 * rows;
  float* f = reinterpret_cast<float*>(d + 2 * rows + (size_t)m->NP);
  m->lp = f;
  m->ab = f + rows * m->sext;
  m->bb = f + 2 * rows * m->sext;
  f += 3 * rows * m->sext;
  m->lse = f;
  m->utt_loss = f + (m->T > 0 ? m->T : 0);
  m->w = m->utt_loss + m->NP;
}

static void ctc_mwer_sweep(hipStream_t s, const CtcMwer& m, bool with_grad);

void ctc_mwer(hipStream_t s, const CtcMwer& m, float* dlogits, int ldd, int row0, int rows, Twin tw, int stages) {
  if (m.U <= 0) return;
  if (stages & kCtcMwerSweep) ctc_mwer_sweep(s, m, dlogits != nullptr);
  // the distance is symmetric: the references are the kernel's `hyp` operand (start and length per pair), the pairs'
  // labels its `ref` operand (the one that selects the register tile)
  if ((stages & kCtcMwerWeights) && m.P > 0)
    label_edit_distance(s, m.labels, ctc_mwer_ref_at(m), ctc_mwer_ref_cnt(m), m.labels, ctc_mwer_lab_off(m), m.P, m.max_hyp,
                        m.edits);
  if (stages & kCtcMwerWeights) hipLaunchKernelGGL(ctc_mwer_weights_kernel, dim3(m.U), dim3(64), 0, s, m);
  if ((stages & kCtcMwerGrad) && dlogits && rows > 0)
    hipLaunchKernelGGL(ctc_mwer_grad_kernel, dim3(rows), dim3(64), (size_t)(m.ld + m.sext) * sizeof(float), s, m, row0, dlogits,
                       ldd, tw);
}

// row log-sum-exps, the pairs' emissions, the sweeps (backward too: with_grad)
static void ctc_mwer_sweep(hipStream_t s, const CtcMwer& m, bool with_grad) {
  if (m.T > 0)
    hipLaunchKernelGGL(ctc_row_lse_kernel, dim3((unsigned)((m.T + 3) / 4)), dim3(256), 0, s, m.logits, m.ld, m.O, m.T, m.lse);
  const size_t n = (size_t)m.PR * m.sext;
  if (n > 0) hipLaunchKernelGGL(ctc_pair_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m);
  if (m.NP > 0) {
    CtcBatch b = {};
    b.seg = ctc_mwer_prow(m); b.labels = m.labels; b.lab_off = ctc_mwer_lab_off(m);
    b.U = m.NP; b.T = (int)m.PR; b.O = m.O; b.sext = m.sext;
    b.lp = m.lp; b.ab = m.ab; b.bb = m.bb; b.off = m.off; b.offb = m.offb; b.logz = m.logz; b.utt_loss = m.utt_loss;
    const dim3 grid(m.NP, with_grad ? 2 : 1);
    switch (m.sext / 64) {
      case 2: hipLaunchKernelGGL(ctc_alpha_beta_kernel<2>, grid, dim3(64), 0, s, b); break;
      case 4: hipLaunchKernelGGL(ctc_alpha_beta_kernel<4>, grid, dim3(64), 0, s, b); break;
      case 8: hipLaunchKernelGGL(ctc_alpha_beta_kernel<8>, grid, dim3(64), 0, s, b); break;
      default: hipLaunchKernelGGL(ctc_alpha_beta_kernel<16>, grid, dim3(64), 0, s, b); break;
    }
  }
}

void ctc_mwer_loss_reduce(hipStream_t s, const CtcMwer& m, int ref_labels, float* scalars, bool overwrite) {
  hipLaunchKernelGGL(ctc_mwer_loss_reduce_kernel, dim3(1), dim3(256), 0, s, m.risk,
                     m.NP > m.P ? m.utt_loss + m.P : (const float*)nullptr, m.U, m.ctc_weight, (float)ref_labels, scalars,
                     overwrite ? 1 : 0);
}

const char* ctc_den_graph_limits(int O, int64_t num_states, int64_t arcs) {
  if (O < 2 || O > kCtcDenMaxClasses) return "output_dim outside [2, 1024]";
  if (num_states < 1) return "num_states < 1";
  if (num_states * O > (int64_t)kCtcGraphMaxEntries) return "more than 2^25 entries per table (S x O)";
  if (num_states + arcs > kCtcDenMaxStates) return "more than 65536 composed states (N = states + arcs)";
  return nullptr;
}

const char* ctc_den_limits(int O, int T, int U, int N) {
  if (O < 2 || O > kCtcDenMaxClasses) return "output_dim outside [2, 1024]";
  if (N < 1 || N > kCtcDenMaxStates) return "more than 65536 composed states (N = states + arcs)";
  if (T < 0 || T > kCtcAlignMaxFrames) return "more than 8388607 frames";
  if (U < 0 || U > (1 << 20)) return "more than 1048576 utterances";
  if ((int64_t)T * ctc_den_stride(N) > kCtcDenMaxCells)
    return "more than 2^31 lattice cells (frames x padded composed states) in one call";
  return nullptr;
}

void ctc_den_compile(const float* weight, const int32_t* next, int S, int O, int start, CtcDenGraph* g) {
  struct Arc { int src, c, dst; float w; };
  std::vector<Arc> arcs;
  std::vector<int32_t> cfirst(O, 0);
  for (int c = 0; c < O - 1; ++c) {  // arc order: (label, source)
    cfirst[c] = (int32_t)arcs.size();
    for (int s = 0; s < S; ++s) {
      const float w = weight[(size_t)s * O + c];
      if (w > -INFINITY) arcs.push_back({s, c, next[(size_t)s * O + c], w});
    }
  }
  const int A = (int)arcs.size();
  cfirst[O - 1] = A;
  // per state: outgoing arcs by label, incoming arcs by (label, arc) -- both fall out of the arc order
  std::vector<std::vector<int32_t>> out(S), in(S);
  for (int a = 0; a < A; ++a) {
    out[arcs[a].src].push_back(a);
    in[arcs[a].dst].push_back(a);
  }
  // groups: the runs of one label in a state's incoming list
  std::vector<int32_t> g0(S + 1, 0), ffirst(S + 1, 0), bfirst(S + 1, 0), fterm, bterm, flo, fhi, blo, bhi, garc(A, 0);
  std::vector<int32_t> glabel;
  for (int s = 0; s < S; ++s) {
    for (size_t j = 0; j < in[s].size(); ++j) {
      const int a = in[s][j];
      if (j == 0 || arcs[in[s][j - 1]].c != arcs[a].c) {
        if (j > 0) fhi.push_back((int32_t)fterm.size());
        flo.push_back((int32_t)fterm.size());
        glabel.push_back(arcs[a].c);
      }
      garc[a] = (int32_t)flo.size() - 1;
      fterm.push_back(a);
    }
    if (!in[s].empty()) fhi.push_back((int32_t)fterm.size());
    g0[s + 1] = (int32_t)flo.size();
    ffirst[s + 1] = (int32_t)fterm.size();
    for (int a : out[s]) bterm.push_back(a);
    bfirst[s + 1] = (int32_t)bterm.size();
  }
  const int K = (int)flo.size();
  blo.assign(K, 0);
  bhi.assign(K, 0);
  for (int s = 0; s < S; ++s)
    for (int k = g0[s]; k < g0[s + 1]; ++k) {  // the out-arc of the group's label: out[s] is ordered by label
      size_t j = 0;
      while (j < out[s].size() && arcs[out[s][j]].c < glabel[k]) ++j;
      blo[k] = bfirst[s] + (int32_t)j;
      bhi[k] = blo[k] + ((j < out[s].size() && arcs[out[s][j]].c == glabel[k]) ? 1 : 0);
    }
  g->O = O; g->S = S; g->A = A; g->K = K; g->N = S + A; g->start = start;
  g->tab.assign(ctc_den_tab_words(S, A, K, O), 0);
  int32_t* t = g->tab.data();
  int32_t* fx = t;
  int32_t* bx = fx + A;
  for (int a = 0; a < A; ++a) {
    const Arc& r = arcs[a];
    int x = r.src;  // the source's total, unless it is entered by this label too
    for (int k = g0[r.src]; k < g0[r.src + 1]; ++k)
      if (glabel[k] == r.c) x = S + k;
    fx[a] = (int32_t)(((uint32_t)r.c << 16) | (uint32_t)x);
    bx[a] = (int32_t)(((uint32_t)r.c << 16) | (uint32_t)(S + garc[a]));
  }
  int32_t* p = bx + A;
  auto put = [&p](const std::vector<int32_t>& v) {
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(int32_t));
    p += v.size();
  };
  put(g0); put(ffirst); put(fterm); put(flo); put(fhi); put(bfirst); put(bterm); put(blo); put(bhi); put(cfirst);
  g->logw.resize((size_t)A + S);
  for (int a = 0; a < A; ++a) g->logw[a] = arcs[a].w;
  for (int s = 0; s < S; ++s) g->logw[(size_t)A + s] = weight[(size_t)s * O + O - 1];
  g->ofirst = bfirst;
  g->olabel.resize(A); g->odst.resize(A); g->oweight.resize(A);
  for (int j = 0; j < A; ++j) {
    g->olabel[j] = arcs[bterm[j]].c; g->odst[j] = arcs[bterm[j]].dst; g->oweight[j] = arcs[bterm[j]].w;
  }
}

double ctc_den_walk(const CtcDenGraph& g, const int32_t* labels, int n) {
  int s = g.start;
  double total = 0.0;
  for (int i = 0; i < n; ++i) {
    int lo = g.ofirst[s], hi = g.ofirst[s + 1];
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (g.olabel[mid] < labels[i]) lo = mid + 1; else hi = mid;
    }
    if (lo >= g.ofirst[s + 1] || g.olabel[lo] != labels[i]) return -(double)INFINITY;
    total += (double)g.oweight[lo];
    s = g.odst[lo];
  }
  return total + (double)g.logw[(size_t)g.A + s];
}

size_t ctc_den_lds_bytes(int O, int N, int S, int K, bool lds) {
  return ((size_t)((O + 63) & ~63) + (lds ? (size_t)N + S + K : 0)) * sizeof(float);
}

int ctc_den_residence(int O, int N, int S, int A, int K) {
  const size_t vec = ctc_den_lds_bytes(O, N, S, K, true);
  if (vec > kCtcDenMaxLds) return 0;
  return vec + (ctc_den_tab_words(S, A, K, O) + (size_t)A + S) * sizeof(float) <= kCtcDenMaxLds ? 2 : 1;
}

size_t ctc_den_scratch_bytes(const CtcDen& d, bool with_grad) {
  const size_t t = (size_t)(d.T > 0 ? d.T : 0), u = (size_t)(d.U > 0 ? d.U : 0), stride = (size_t)ctc_den_stride(d.N);
  const bool lds = ctc_den_residence(d.O, d.N, d.S, d.A, d.K) >= 1;
  return (2 * t + u) * sizeof(double) +
         ((with_grad ? 2 : 1) * t * stride + (size_t)d.A + d.S + (lds ? 0 : 2 * u * (stride + d.S + d.K))) * sizeof(float) + 16;
}

void ctc_den_carve(void* scratch, CtcDen* d, bool with_grad) {
  const size_t t = (size_t)(d->T > 0 ? d->T : 0), u = (size_t)(d->U > 0 ? d->U : 0);
  d->stride = ctc_den_stride(d->N);
  const int where = ctc_den_residence(d->O, d->N, d->S, d->A, d->K);
  d->lds = where >= 1;
  d->tab_lds = where >= 2;
  double* p = static_cast<double*>(scratch);
  d->offa = p;
  d->offb = p + t;
  d->logz = p + 2 * t;
  float* f = reinterpret_cast<float*>(p + 2 * t + u);
  d->va = f;
  f += t * d->stride;
  d->vb = with_grad ? f : nullptr;
  if (with_grad) f += t * d->stride;
  d->wexp = f;
  f += (size_t)d->A + d->S;
  d->gv = d->lds ? nullptr : f;
  d->gs = d->lds ? nullptr : f + 2 * u * d->stride;
}

template <int NT, bool LDS>
static void den_launch(hipStream_t s, const CtcDen& d, bool with_grad) {
  const size_t lds = ctc_den_lds_bytes(d.O, d.N, d.S, d.K, LDS) +
                     (LDS && d.tab_lds ? (ctc_den_tab_words(d.S, d.A, d.K, d.O) + (size_t)d.A + d.S) * sizeof(float) : 0);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ctc_den_sweep_kernel<NT, LDS>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((ctc_den_sweep_kernel<NT, LDS>), dim3(d.U, with_grad ? 2 : 1), dim3(NT), lds, s, d);
}

void ctc_den_sweep(hipStream_t s, const CtcDen& d, const CtcBatch& num, bool with_grad, float* logz_out) {
  if (d.U <= 0) return;
  hipLaunchKernelGGL(ctc_den_prep_kernel, dim3((unsigned)((d.A + d.S + 255) / 256)), dim3(256), 0, s, d);
  // a workgroup of 256 threads while that leaves a thread at most 8 composed states (and one class of the row each); such a
  // graph is at most 256 + 2 * 2048 floats, so its residence is always LDS
  const bool big = d.N > 2048 || d.O > 256;
  if (!big) den_launch<256, true>(s, d, with_grad);
  else if (d.lds) den_launch<1024, true>(s, d, with_grad);
  else den_launch<1024, false>(s, d, with_grad);
  hipLaunchKernelGGL(ctc_den_loss_kernel, dim3((unsigned)((d.U + 255) / 256)), dim3(256), 0, s, d, num.logz, num.utt_loss,
                     logz_out);
}

void ctc_den_grad(hipStream_t s, const CtcDen& d, const float* g, int ldg, float* dlogits, int ldd, int row0, int rows,
                  Twin tw) {
  if (rows <= 0 || d.U <= 0) return;
  hipLaunchKernelGGL(ctc_den_grad_kernel, dim3(rows), dim3(256), (size_t)d.O * sizeof(float), s, d, g, ldg, row0, dlogits, ldd,
                     tw);
}

void ctc_den_loss_reduce(hipStream_t s, const CtcDen& d, const float* ctc_utt_loss, int ref_labels, float* scalars,
                         bool overwrite) {
  hipLaunchKernelGGL(ctc_mwer_loss_reduce_kernel, dim3(1), dim3(256), 0, s, d.utt_loss,
                     d.ctc_weight > 0.f ? ctc_utt_loss : (const float*)nullptr, d.U, d.ctc_weight, (float)ref_labels, scalars,
                     overwrite ? 1 : 0);
}

void label_edit_distance(hipStream_t s, const int32_t* hyp, const int32_t* hyp_off, const int32_t* hyp_cnt,
                         const int32_t* ref, const int32_t* ref_off, int U, int max_ref, int32_t* dist) {
  if (U <= 0) return;
  const int r = max_ref <= 64 ? 1 : max_ref <= 128 ? 2 : max_ref <= 256 ? 4 : 8;
  switch (r) {
    case 1: hipLaunchKernelGGL(edit_distance_kernel<1>, dim3(U), dim3(64), 0, s, hyp, hyp_off, hyp_cnt, ref, ref_off, dist); break;
    case 2: hipLaunchKernelGGL(edit_distance_kernel<2>, dim3(U), dim3(64), 0, s, hyp, hyp_off, hyp_cnt, ref, ref_off, dist); break;
    case 4: hipLaunchKernelGGL(edit_distance_kernel<4>, dim3(U), dim3(64), 0, s, hyp, hyp_off, hyp_cnt, ref, ref_off, dist); break;
    default: hipLaunchKernelGGL(edit_distance_kernel<8>, dim3(U), dim3(64), 0, s, hyp, hyp_off, hyp_cnt, ref, ref_off, dist); break;
  }
}

}  // namespace tfk
