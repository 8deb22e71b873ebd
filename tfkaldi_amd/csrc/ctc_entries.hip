// The stand-alone CTC entries of the C ABI (include/tfkaldi_hip.h): they take a stream and logits in HBM and need no
// tfk_engine.  Host code only -- every kernel is ctc.hip's.  What the entries share is written once here:
//   fetch_tables   the small tables that only the device knows come back first, in one synchronisation
//   ctc_tables.h   the checks of those tables (plain C++, run on the CPU by tools/ctc_tables_check.cpp)
//   Scratch        the call's own stream-ordered scratch, released whatever happened in between
//   carve_batch    a CtcBatch out of one allocation (the arithmetic: ctc_batch_layout in ctc_tables.h)
#include "../../include/tfkaldi_hip.h"
#include "ctc.h"
#include "ctc_tables.h"
#include "tfk_error.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <vector>

using namespace tfk;

namespace {

// Small device arrays of 4-byte words come back to the host after ONE synchronisation: back to back in *h (int32 tables), or
// at `to` where the caller keeps them elsewhere (a float table).  A part whose dev is NULL is skipped and reads as zeros.
struct Table {
  const void* dev;
  size_t words;
  void* to = nullptr;
};
int fetch_tables(hipStream_t st, std::initializer_list<Table> parts, std::vector<int32_t>* h) {
  size_t all = 0;
  for (const Table& t : parts) all += t.to ? 0 : t.words;
  h->assign(all > 0 ? all : 1, 0);
  size_t at = 0;
  for (const Table& t : parts) {
    void* dst = t.to ? t.to : h->data() + at;
    if (t.dev && t.words > 0) HIPCHK(hipMemcpyAsync(dst, t.dev, t.words * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    at += t.to ? 0 : t.words;
  }
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

// The scratch of one call, allocated and released in stream order.  done() is the end of a call that got as far as its
// launches: the scratch is freed even when a copy or the launch failed, and the launch error is reported before the free
// error.  A call that returns earlier frees through the destructor.
class Scratch {
 public:
  explicit Scratch(hipStream_t st) : st_(st) {}
  ~Scratch() { (void)release(); }
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  template <class Tp>
  int get(Tp** p, size_t bytes) {
    void* q = nullptr;
    HIPCHK(hipMallocAsync(&q, bytes > 0 ? bytes : 16, st_));
    held_[n_++] = q;
    *p = static_cast<Tp*>(q);
    return 0;
  }
  // copied: what the call's own copies into the scratch gave (it launches nothing when they failed)
  int done(hipError_t copied = hipSuccess) {
    const hipError_t launched = copied != hipSuccess ? copied : hipGetLastError();
    const hipError_t freed = release();
    HIPCHK(launched);
    HIPCHK(freed);
    return 0;
  }

 private:
  hipError_t release() {
    hipError_t first = hipSuccess;
    for (int i = 0; i < n_; ++i) {
      const hipError_t got = hipFreeAsync(held_[i], st_);
      if (first == hipSuccess) first = got;
    }
    n_ = 0;
    return first;
  }
  hipStream_t st_;
  void* held_[2];  // (no entry allocates more than two)
  int n_ = 0;
};

// The regions of layout L at base into b: the three double regions, then post, lp / ab / bb and lse.
void carve_batch(unsigned char* base, const CtcBatchLayout& L, CtcBatch* b) {
  b->off = reinterpret_cast<double*>(base + L.off);
  b->offb = reinterpret_cast<double*>(base + L.offb);
  b->logz = reinterpret_cast<double*>(base + L.logz);
  b->post = reinterpret_cast<float*>(base + L.post);
  b->lp = reinterpret_cast<float*>(base + L.lp);
  b->ab = reinterpret_cast<float*>(base + L.ab);
  b->bb = reinterpret_cast<float*>(base + L.bb);
  b->lse = reinterpret_cast<float*>(base + L.lse);
}

int ctc_beam_logits_impl(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                         int32_t beam_width, int32_t top_paths, int32_t* hyp, int32_t* hyp_len, float* score, const CtcLm* lm,
                         float* am_score, int label_topk = 0) {
  hipStream_t st = (hipStream_t)stream;
  if (label_topk) {
    if (const char* why = ctc_beam_topk_limits(O, T, U, beam_width, top_paths, label_topk))
      return fail(-1, "CTC beam search (beam_width %d, top_paths %d, label_topk %d, O %d, T %d, U %d): %s", beam_width,
                  top_paths, label_topk, O, T, U, why);
  } else if (const char* why = ctc_beam_limits(O, T, U, beam_width, top_paths)) {
    return fail(-1, "CTC beam search (beam_width %d, top_paths %d, O %d, T %d, U %d): %s", beam_width, top_paths, O, T, U, why);
  }
  if (U == 0) return 0;
  if (!seg || !hyp_len || !score || (T > 0 && (!logits || !hyp))) return fail(-1, "logits / seg / hyp / hyp_len / score is NULL");
  if (ld < O || ld > 0x7fffffff) return fail(-1, "ld = %lld outside [O = %d, 2^31)", (long long)ld, O);
  Scratch sc(st);
  unsigned long long* trie = nullptr;
  uint32_t* pre = nullptr;
  CHK(sc.get(&trie, ctc_beam_scratch_words(T, U, beam_width) * sizeof(unsigned long long)));
  if (label_topk && T > 0) CHK(sc.get(&pre, ctc_beam_topk_scratch_words(T) * sizeof(uint32_t)));
  if (label_topk) ctc_beam_topk_rows(st, logits, (int)ld, O, T, label_topk, pre);
  if (label_topk)
    ctc_beam_topk_search(st, logits, (int)ld, O, T, seg, U, beam_width, top_paths, label_topk, trie, pre, hyp, hyp_len, score,
                         lm, am_score);
  else
    ctc_beam_search(st, logits, (int)ld, O, T, seg, U, beam_width, top_paths, trie, hyp, hyp_len, score, lm, am_score);
  return sc.done();
}

}  // namespace

extern "C" {

int tfk_ctc_beam_topk_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                             int32_t beam_width, int32_t top_paths, int32_t label_topk, const float* lm_dev, int32_t order,
                             float lm_weight, float label_bonus, int flags, int32_t* hyp, int32_t* hyp_len, float* score,
                             float* am_score) {
  if (label_topk < 1) return fail(-1, "tfk_ctc_beam_topk_logits: label_topk outside [1, 63]");
  if (flags & ~TFK_CTC_LM_EOS) return fail(-1, "tfk_ctc_beam_topk_logits: flags %d, it takes 0 or TFK_CTC_LM_EOS", flags);
  if (!lm_dev) {
    if (flags) return fail(-1, "tfk_ctc_beam_topk_logits: TFK_CTC_LM_EOS without a table");
    return ctc_beam_logits_impl(stream, logits, ld, O, T, seg, U, beam_width, top_paths, hyp, hyp_len, score, nullptr, am_score,
                                label_topk);
  }
  if (order < 1 || order > kCtcLmMaxOrder)
    return fail(-1, "tfk_ctc_beam_topk_logits: order %d outside [1, %d]", order, kCtcLmMaxOrder);
  if (O >= 2 && O <= kCtcTopkMaxClasses && ctc_lm_entries(O, order) > kCtcLmMaxEntries)
    return fail(-1, "tfk_ctc_beam_topk_logits: a table of order %d over %d outputs has more than %zu entries", order, O,
                kCtcLmMaxEntries);
  const CtcLm lm = {lm_dev, order, lm_weight, label_bonus, (flags & TFK_CTC_LM_EOS) != 0};
  return ctc_beam_logits_impl(stream, logits, ld, O, T, seg, U, beam_width, top_paths, hyp, hyp_len, score, &lm, am_score,
                              label_topk);
}
int tfk_ctc_beam_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                        int32_t beam_width, int32_t top_paths, int32_t* hyp, int32_t* hyp_len, float* score) {
  return ctc_beam_logits_impl(stream, logits, ld, O, T, seg, U, beam_width, top_paths, hyp, hyp_len, score, nullptr, nullptr);
}
int tfk_ctc_beam_lm_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                           int32_t beam_width, int32_t top_paths, const float* lm_dev, int32_t order, float lm_weight,
                           float label_bonus, int flags, int32_t* hyp, int32_t* hyp_len, float* score, float* am_score) {
  if (order < 1 || order > kCtcLmMaxOrder) return fail(-1, "tfk_ctc_beam_lm_logits: order %d outside [1, %d]", order, kCtcLmMaxOrder);
  if (flags & ~TFK_CTC_LM_EOS) return fail(-1, "tfk_ctc_beam_lm_logits: flags %d, it takes 0 or TFK_CTC_LM_EOS", flags);
  if (!lm_dev) return fail(-1, "tfk_ctc_beam_lm_logits: the table is NULL");
  const CtcLm lm = {lm_dev, order, lm_weight, label_bonus, (flags & TFK_CTC_LM_EOS) != 0};
  return ctc_beam_logits_impl(stream, logits, ld, O, T, seg, U, beam_width, top_paths, hyp, hyp_len, score, &lm, am_score);
}
int tfk_ctc_beam_graph_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg,
                              int32_t U, int32_t beam_width, int32_t top_paths, int32_t label_topk, const float* weight_dev,
                              const int32_t* next_dev, int32_t num_states, int32_t start, float lm_weight, float label_bonus,
                              int flags, int32_t* hyp, int32_t* hyp_len, float* score, float* am_score) {
  if (label_topk < 0) return fail(-1, "tfk_ctc_beam_graph_logits: label_topk outside [0, 63]");
  if (flags & ~TFK_CTC_LM_EOS) return fail(-1, "tfk_ctc_beam_graph_logits: flags %d, it takes 0 or TFK_CTC_LM_EOS", flags);
  if (!weight_dev || !next_dev) return fail(-1, "tfk_ctc_beam_graph_logits: weight / next is NULL");
  if (num_states < 1 || start < 0 || start >= num_states)
    return fail(-1, "tfk_ctc_beam_graph_logits: start %d outside [0, num_states = %d)", start, num_states);
  if (O >= 2 && (size_t)num_states * (size_t)O > kCtcGraphMaxEntries)
    return fail(-1, "tfk_ctc_beam_graph_logits: a graph of %d states over %d outputs has more than %zu entries per table",
                num_states, O, kCtcGraphMaxEntries);
  const CtcLm lm = {weight_dev, 0, lm_weight, label_bonus, (flags & TFK_CTC_LM_EOS) != 0, next_dev, num_states, start};
  return ctc_beam_logits_impl(stream, logits, ld, O, T, seg, U, beam_width, top_paths, hyp, hyp_len, score, &lm, am_score,
                              label_topk);
}

// The register tile of the alignment follows the longest label sequence, which only the device knows: the two offset tables
// come back first (2 (U + 1) words); everything after that is stream-ordered.
int tfk_ctc_align_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                         const int32_t* labels, const int32_t* lab_off, int32_t* ali, float* score) {
  hipStream_t st = (hipStream_t)stream;
  if (U < 0) return fail(-1, "U = %d < 0", U);
  if (U == 0) return 0;
  if (!seg || !lab_off || !score || (T > 0 && (!logits || !ali))) return fail(-1, "logits / seg / lab_off / ali / score is NULL");
  if (ld < O || ld > 0x7fffffff) return fail(-1, "ld = %lld outside [O = %d, 2^31)", (long long)ld, O);
  std::vector<int32_t> h;
  CHK(fetch_tables(st, {{seg, (size_t)U + 1}, {lab_off, (size_t)U + 1}}, &h));
  const int32_t* h_off = h.data() + U + 1;
  int max_labels = 0;
  CHK(seg_check("CTC align", h.data(), U, T));
  CHK(offsets_check("CTC align", "utterance", "", h_off, U, -1, &max_labels));
  if (const char* why = ctc_align_limits(O, T, U, max_labels)) return fail(-1, "CTC align (O %d, T %d, U %d): %s", O, T, U, why);
  if (h_off[U] > h_off[0] && !labels) return fail(-1, "CTC align: labels is NULL");
  Scratch sc(st);
  void* scratch = nullptr;
  CHK(sc.get(&scratch, ctc_align_scratch_bytes(T, max_labels)));
  ctc_viterbi_align(st, logits, (int)ld, O, T, seg, U, labels, lab_off, max_labels, scratch, ali, score);
  return sc.done();
}
int tfk_ctc_align_wild_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg,
                              int32_t U, const int32_t* labels, const int32_t* lab_off, const uint8_t* wild, int32_t* ali,
                              float* score, float* free_score) {
  hipStream_t st = (hipStream_t)stream;
  if (U < 0) return fail(-1, "U = %d < 0", U);
  if (U == 0) return 0;
  if (!seg || !lab_off || !score || !free_score || (T > 0 && (!logits || !ali)))
    return fail(-1, "logits / seg / lab_off / ali / score / free_score is NULL");
  if (ld < O || ld > 0x7fffffff) return fail(-1, "ld = %lld outside [O = %d, 2^31)", (long long)ld, O);
  std::vector<int32_t> h;
  CHK(fetch_tables(st, {{seg, (size_t)U + 1}, {lab_off, (size_t)U + 1}}, &h));
  const int32_t* h_off = h.data() + U + 1;
  int max_labels = 0;
  CHK(seg_check("CTC align", h.data(), U, T));
  CHK(offsets_check("CTC align", "utterance", "", h_off, U, -1, &max_labels));
  if (const char* why = ctc_align_limits(O, T, U, max_labels)) return fail(-1, "CTC align (O %d, T %d, U %d): %s", O, T, U, why);
  if (h_off[U] > h_off[0] && !labels) return fail(-1, "CTC align: labels is NULL");
  Scratch sc(st);
  void* scratch = nullptr;
  CHK(sc.get(&scratch, ctc_align_wild_scratch_bytes(T, max_labels)));
  ctc_viterbi_align_wild(st, logits, (int)ld, O, T, seg, U, labels, lab_off, wild, max_labels, scratch, ali, score, free_score);
  return sc.done();
}

// Rescoring and spotting: the register tile follows the longest hypothesis, so the three small tables come back first
// (U + 2P + 2 words).
int tfk_ctc_score_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                         const int32_t* pair_utt, int32_t P, const int32_t* labels, const int32_t* lab_off, float* score) {
  hipStream_t st = (hipStream_t)stream;
  if (U < 0 || P < 0) return fail(-1, "U = %d / P = %d < 0", U, P);
  if (P > kCtcScoreMaxPairs) return fail(-1, "CTC score: more than %d (utterance, hypothesis) pairs in one call", kCtcScoreMaxPairs);
  if (P == 0) return 0;
  if (U == 0) return fail(-1, "CTC score: %d pairs and no utterance", P);
  if (!seg || !pair_utt || !lab_off || !score || (T > 0 && !logits))
    return fail(-1, "logits / seg / pair_utt / lab_off / score is NULL");
  if (ld < O || ld > 0x7fffffff) return fail(-1, "ld = %lld outside [O = %d, 2^31)", (long long)ld, O);
  std::vector<int32_t> h;
  CHK(fetch_tables(st, {{seg, (size_t)U + 1}, {pair_utt, (size_t)P}, {lab_off, (size_t)P + 1}}, &h));
  const int32_t* h_utt = h.data() + U + 1;
  const int32_t* h_off = h_utt + P;
  int max_labels = 0;
  CHK(seg_check("CTC score", h.data(), U, T));
  CHK(pairs_check("CTC score", h_utt, h_off, P, U, false, &max_labels));
  if (const char* why = ctc_score_limits(O, T, U, P, max_labels))
    return fail(-1, "CTC score (O %d, T %d, U %d, P %d): %s", O, T, U, P, why);
  if (h_off[P] > h_off[0] && !labels) return fail(-1, "CTC score: labels is NULL");
  Scratch sc(st);
  void* scratch = nullptr;
  CHK(sc.get(&scratch, ctc_score_scratch_bytes(T)));
  ctc_score(st, logits, (int)ld, O, T, seg, U, pair_utt, P, labels, lab_off, max_labels, scratch, score);
  return sc.done();
}
int tfk_ctc_spot_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                        const int32_t* pair_utt, int32_t P, const int32_t* labels, const int32_t* lab_off,
                        const uint8_t* wild, float* score, int32_t* start, int32_t* end, float* free_score) {
  hipStream_t st = (hipStream_t)stream;
  if (U < 0 || P < 0) return fail(-1, "U = %d / P = %d < 0", U, P);
  if (P > kCtcScoreMaxPairs) return fail(-1, "CTC spot: more than %d (utterance, pattern) pairs in one call", kCtcScoreMaxPairs);
  if (U == 0) return P == 0 ? 0 : fail(-1, "CTC spot: %d pairs and no utterance", P);
  if (!seg || !free_score || (T > 0 && !logits)) return fail(-1, "logits / seg / free_score is NULL");
  if (P > 0 && (!pair_utt || !lab_off || !score || !start || !end))
    return fail(-1, "pair_utt / lab_off / score / start / end is NULL");
  if (ld < O || ld > 0x7fffffff) return fail(-1, "ld = %lld outside [O = %d, 2^31)", (long long)ld, O);
  std::vector<int32_t> h;  // (no pair: the pair tables may be NULL, and read as zeros)
  CHK(fetch_tables(st, {{seg, (size_t)U + 1}, {P > 0 ? pair_utt : nullptr, (size_t)P}, {P > 0 ? lab_off : nullptr, (size_t)P + 1}},
                   &h));
  const int32_t* h_utt = h.data() + U + 1;
  const int32_t* h_off = h_utt + P;
  int max_labels = 0;
  CHK(seg_check("CTC spot", h.data(), U, T));
  CHK(pairs_check("CTC spot", h_utt, h_off, P, U, false, &max_labels));
  if (const char* why = ctc_score_limits(O, T, U, P, max_labels))
    return fail(-1, "CTC spot (O %d, T %d, U %d, P %d): %s", O, T, U, P, why);
  if (h_off[P] > h_off[0] && !labels) return fail(-1, "CTC spot: labels is NULL");
  Scratch sc(st);
  void* scratch = nullptr;
  CHK(sc.get(&scratch, ctc_spot_scratch_bytes(T)));
  ctc_spot(st, logits, (int)ld, O, T, seg, U, pair_utt, P, labels, lab_off, wild, max_labels, scratch, score, start, end,
           free_score);
  return sc.done();
}

int tfk_ctc_mwer_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                        const int32_t* pair_utt, int32_t P, const int32_t* labels, const int32_t* lab_off,
                        const int32_t* ref_labels, const int32_t* ref_off, float ctc_weight, float* dlogits, int64_t ldd,
                        float* risk, float* score, int32_t* edits) {
  hipStream_t st = (hipStream_t)stream;
  if (U < 0 || P < 0) return fail(-1, "U = %d / P = %d < 0", U, P);
  if (P > kCtcScoreMaxPairs) return fail(-1, "CTC MWER: more than %d (utterance, hypothesis) pairs in one call", kCtcScoreMaxPairs);
  if (!(ctc_weight >= 0.f) || !std::isfinite(ctc_weight))
    return fail(-1, "CTC MWER: ctc_weight %g is negative or not finite", (double)ctc_weight);
  if (U == 0) return P == 0 ? 0 : fail(-1, "CTC MWER: %d pairs and no utterance", P);
  if (!seg || !ref_off || !risk || (T > 0 && !logits)) return fail(-1, "logits / seg / ref_off / risk is NULL");
  if (P > 0 && (!pair_utt || !lab_off || !score || !edits)) return fail(-1, "pair_utt / lab_off / score / edits is NULL");
  if (ld < O || ld > 0x7fffffff) return fail(-1, "ld = %lld outside [O = %d, 2^31)", (long long)ld, O);
  if (dlogits && (ldd < O || ldd > 0x7fffffff)) return fail(-1, "ldd = %lld outside [O = %d, 2^31)", (long long)ldd, O);
  // The shapes live in the small tables, which only the device knows: they come back first
  std::vector<int32_t> h;
  CHK(fetch_tables(st, {{seg, (size_t)U + 1}, {ref_off, (size_t)U + 1}, {P > 0 ? pair_utt : nullptr, (size_t)P},
                        {P > 0 ? lab_off : nullptr, (size_t)P + 1}}, &h));
  const int32_t* h_seg = h.data();
  const int32_t* h_roff = h_seg + U + 1;
  const int32_t* h_utt = h_roff + U + 1;
  const int32_t* h_off = h_utt + P;
  int max_hyp = 0, max_ref = 0;
  CHK(seg_check("CTC MWER", h_seg, U, T));
  if (h_roff[0] < 0 || h_off[0] < 0) return fail(-1, "CTC MWER: lab_off[0] / ref_off[0] < 0");
  CHK(offsets_check("CTC MWER", "utterance", " reference", h_roff, U, -1, &max_ref));
  CHK(pairs_check("CTC MWER", h_utt, h_off, P, U, true, &max_hyp));
  std::vector<int32_t> utt_len(U), ref_len(U), hyp_count(U, 0), hyp_len(P > 0 ? P : 1);
  int64_t PR = 0;
  for (int p = 0; p < P; ++p) {
    hyp_len[p] = h_off[p + 1] - h_off[p];
    ++hyp_count[h_utt[p]];
  }
  for (int u = 0; u < U; ++u) {
    utt_len[u] = h_seg[u + 1] - h_seg[u];
    ref_len[u] = h_roff[u + 1] - h_roff[u];
    PR += (int64_t)(hyp_count[u] + (ctc_weight > 0.f ? 1 : 0)) * utt_len[u];
  }
  const int max_labels = std::max(max_hyp, max_ref);  // (the references' edit distance rides the same limit)
  if (const char* why = ctc_mwer_limits(O, ld, T, U, P, max_labels, PR))
    return fail(-1, "CTC MWER (O %d, T %d, U %d, P %d, longest label sequence %d): %s", O, T, U, P, max_labels, why);
  const int hyp_total = h_off[P] - h_off[0], ref_total = h_roff[U] - h_roff[0];
  if ((hyp_total > 0 && !labels) || (ref_total > 0 && !ref_labels)) return fail(-1, "CTC MWER: labels / ref_labels is NULL");
  const int NP = ctc_weight > 0.f ? P + U : P;
  const int sext = ctc_state_stride(ctc_weight > 0.f ? max_labels : max_hyp);
  const size_t tab_words = ctc_mwer_table_words(U, P, NP), total = (size_t)hyp_total + (size_t)ref_total;
  const size_t ints = ((tab_words + total + 1) * sizeof(int32_t) + 15) & ~(size_t)15;
  std::vector<int32_t> tab(tab_words);
  ctc_mwer_table(utt_len.data(), U, hyp_count.data(), hyp_len.data(), ref_len.data(), NP > P, tab.data());
  Scratch sc(st);
  unsigned char* scratch = nullptr;  // [tables | labels | lattices]
  CHK(sc.get(&scratch, ints + ctc_mwer_scratch_bytes(T, NP, P, PR, sext)));
  int32_t* d_tab = reinterpret_cast<int32_t*>(scratch);
  hipError_t copied = hipMemcpyAsync(d_tab, tab.data(), tab_words * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (copied == hipSuccess && hyp_total > 0)
    copied = hipMemcpyAsync(d_tab + tab_words, labels + h_off[0], (size_t)hyp_total * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
  if (copied == hipSuccess && ref_total > 0)
    copied = hipMemcpyAsync(d_tab + tab_words + hyp_total, ref_labels + h_roff[0], (size_t)ref_total * sizeof(int32_t),
                            hipMemcpyDeviceToDevice, st);
  if (copied == hipSuccess) copied = hipStreamSynchronize(st);  // (the table leaves pageable host memory)
  if (copied == hipSuccess) {
    CtcMwer m = {};
    m.logits = logits; m.ld = (int)ld; m.O = O; m.T = T; m.U = U; m.seg = seg;
    m.P = P; m.NP = NP; m.PR = PR; m.sext = sext; m.max_hyp = max_hyp; m.ctc_weight = ctc_weight;
    m.tab = d_tab; m.labels = d_tab + tab_words;
    ctc_mwer_carve(scratch + ints, &m);
    m.risk = risk; m.score = score; m.edits = edits;
    ctc_mwer(st, m, dlogits, (int)ldd, h_seg[0], h_seg[U] - h_seg[0], Twin());
  }
  return sc.done(copied);
}

int tfk_ctc_mmi_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                       const int32_t* labels, const int32_t* lab_off, const float* weight_dev, const int32_t* next_dev,
                       int32_t num_states, int32_t start, float lm_scale, float ctc_weight, float* utt_loss, float* logz,
                       float* dlogits, int64_t ldd) {
  hipStream_t st = (hipStream_t)stream;
  if (U < 0) return fail(-1, "U = %d < 0", U);
  if (!(lm_scale >= 0.f) || !std::isfinite(lm_scale)) return fail(-1, "CTC MMI: lm_scale %g is negative or not finite", (double)lm_scale);
  if (!(ctc_weight >= 0.f) || !std::isfinite(ctc_weight))
    return fail(-1, "CTC MMI: ctc_weight %g is negative or not finite", (double)ctc_weight);
  if (!weight_dev || !next_dev) return fail(-1, "CTC MMI: no denominator graph (weight / next is NULL)");
  if (num_states < 1) return fail(-1, "CTC MMI: num_states %d < 1", num_states);
  if (const char* why = ctc_den_graph_limits(O, num_states, 0))
    return fail(-1, "CTC MMI (%d states over %d outputs): %s", num_states, O, why);
  if (U == 0) return 0;
  if (T <= 0) return fail(-1, "CTC MMI: empty batch (T = %d)", T);
  if (!seg || !lab_off || !utt_loss || !logz || (T > 0 && !logits)) return fail(-1, "logits / seg / lab_off / utt_loss / logz is NULL");
  if (ld < O || ld > 0x7fffffff) return fail(-1, "ld = %lld outside [O = %d, 2^31)", (long long)ld, O);
  if (dlogits && (ldd < O || ldd > 0x7fffffff)) return fail(-1, "ldd = %lld outside [O = %d, 2^31)", (long long)ldd, O);
  // The shapes and the graph live on the device: they come back first.  The batch is the whole of the logits, and its
  // labels start at 0.
  const size_t ng = (size_t)num_states * (size_t)O;
  std::vector<int32_t> h;
  std::vector<float> h_w(ng);
  CHK(fetch_tables(st, {{seg, (size_t)U + 1}, {lab_off, (size_t)U + 1}, {next_dev, ng}, {weight_dev, ng, h_w.data()}}, &h));
  const int32_t* h_off = h.data() + U + 1;
  const int32_t* h_next = h_off + U + 1;
  int max_labels = 0;
  CHK(seg_check("CTC MMI", h.data(), U, T, /*whole=*/true));
  if (h_off[0] != 0) return fail(-1, "CTC MMI: lab_off[0] = %d is not 0", h_off[0]);
  CHK(offsets_check("CTC MMI", "utterance", " reference", h_off, U, kCtcMaxLabels, &max_labels));
  const int total = h_off[U];
  if (total > 0 && !labels) return fail(-1, "CTC MMI: labels is NULL");
  std::vector<int32_t> h_lab((size_t)(total > 0 ? total : 1));
  if (total > 0) {  // (the second synchronisation: the walk of the graph below reads the labels on the host)
    HIPCHK(hipMemcpyAsync(h_lab.data(), labels, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  for (int i = 0; i < total; ++i)
    if (h_lab[i] < 0 || h_lab[i] >= O - 1) return fail(-1, "CTC MMI: label %d outside [0, %d)", h_lab[i], O - 1);
  CHK(den_tables_check("CTC MMI", h_w.data(), h_next, O, num_states, start, ctc_den_graph_limits, kCtcDenMaxStates));
  CtcDenGraph g;
  ctc_den_compile(h_w.data(), h_next, num_states, O, start, &g);
  if (const char* why = ctc_den_limits(O, T, U, g.N))
    return fail(-1, "CTC MMI (O %d, T %d, U %d, %d composed states): %s", O, T, U, g.N, why);
  std::vector<double> gy((size_t)U);
  for (int u = 0; u < U; ++u) gy[u] = ctc_den_walk(g, h_lab.data() + h_off[u], h_off[u + 1] - h_off[u]);
  const bool train = dlogits != nullptr;
  const int sext = ctc_state_stride(max_labels);
  CtcDen d = {};
  d.O = g.O; d.S = g.S; d.A = g.A; d.K = g.K; d.N = g.N; d.start = g.start;
  d.ld = (int)ld; d.T = T; d.U = U; d.seg = seg; d.lm_scale = lm_scale; d.ctc_weight = ctc_weight;
  // the call's own scratch: the batch with G(y) (U doubles) in front, g (T ld) behind post, the CTC losses (U) and logw behind
  // lse; then tab, and from `head` (a multiple of 16) on the denominator's lattices
  const size_t u = (size_t)U;
  const CtcBatchLayout L = ctc_batch_layout(T, U, ld, sext, u, (size_t)T * (size_t)ld, u + g.logw.size());
  const size_t ints = (g.tab.size() * sizeof(int32_t) + 15) & ~(size_t)15;
  const size_t head = (L.bytes + ints + 15) & ~(size_t)15;
  Scratch sc(st);
  unsigned char* scratch = nullptr;
  CHK(sc.get(&scratch, head + ctc_den_scratch_bytes(d, train)));
  CtcBatch b;
  b.logits = logits; b.ld = (int)ld; b.seg = seg; b.labels = labels; b.lab_off = lab_off;
  b.U = U; b.T = T; b.O = O; b.sext = sext;
  carve_batch(scratch, L, &b);
  double* d_gy = reinterpret_cast<double*>(scratch + L.lead);
  float* gbuf = reinterpret_cast<float*>(scratch + L.mid);
  b.utt_loss = reinterpret_cast<float*>(scratch + L.tail);
  float* d_logw = b.utt_loss + u;
  int32_t* d_tab = reinterpret_cast<int32_t*>(scratch + L.bytes);
  hipError_t copied = hipMemcpyAsync(d_gy, gy.data(), u * sizeof(double), hipMemcpyHostToDevice, st);
  if (copied == hipSuccess)
    copied = hipMemcpyAsync(d_logw, g.logw.data(), g.logw.size() * sizeof(float), hipMemcpyHostToDevice, st);
  if (copied == hipSuccess)
    copied = hipMemcpyAsync(d_tab, g.tab.data(), g.tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (copied == hipSuccess) copied = hipStreamSynchronize(st);  // (the tables leave pageable host memory)
  if (copied == hipSuccess) {
    d.tab = d_tab; d.logw = d_logw; d.post = b.post; d.gy = d_gy; d.utt_loss = utt_loss;
    ctc_den_carve(scratch + head, &d, train);
    ctc_loss_grad(st, b, gbuf, train ? 1 : 0, Twin());
    ctc_den_sweep(st, d, b, train, logz);
    if (train) ctc_den_grad(st, d, gbuf, (int)ld, dlogits, (int)ldd, 0, T, Twin());
  }
  return sc.done(copied);
}

int tfk_ctc_wild_loss_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                             const int32_t* labels, const int32_t* lab_off, const uint8_t* wild, float penalty, float* utt_loss,
                             float* dlogits, int64_t ldd) {
  hipStream_t st = (hipStream_t)stream;
  if (U < 0) return fail(-1, "U = %d < 0", U);
  if (U == 0) return 0;
  if (T <= 0) return fail(-1, "CTC wild: empty batch (T = %d)", T);
  if (!logits || !seg || !lab_off || !utt_loss) return fail(-1, "logits / seg / lab_off / utt_loss is NULL");
  if (O < 1 || ld < O || ld > 0x7fffffff) return fail(-1, "ld = %lld outside [O = %d, 2^31)", (long long)ld, O);
  if (dlogits && (ldd < O || ldd > 0x7fffffff)) return fail(-1, "ldd = %lld outside [O = %d, 2^31)", (long long)ldd, O);
  if (dlogits == logits && dlogits && ldd != ld) return fail(-1, "dlogits in place needs ldd == ld");
  std::vector<int32_t> h;
  CHK(fetch_tables(st, {{seg, (size_t)U + 1}, {lab_off, (size_t)U + 1}}, &h));
  const int32_t* h_off = h.data() + U + 1;
  int max_labels = 0;
  CHK(seg_check("CTC wild", h.data(), U, T));
  CHK(offsets_check("CTC wild", "utterance", "", h_off, U, kCtcMaxLabels, &max_labels));
  if (h_off[U] > h_off[0] && !labels) return fail(-1, "CTC wild: labels is NULL");
  const bool train = dlogits != nullptr;
  const int sext = ctc_state_stride(max_labels);
  const CtcBatchLayout L = ctc_batch_layout(T, U, ld, sext);
  Scratch sc(st);
  unsigned char* scratch = nullptr;
  CHK(sc.get(&scratch, L.bytes));
  CtcBatch b;
  b.logits = logits; b.ld = (int)ld; b.seg = seg; b.labels = labels; b.lab_off = lab_off;
  b.U = U; b.T = T; b.O = O; b.sext = sext;
  carve_batch(scratch, L, &b);
  b.utt_loss = utt_loss;
  b.wild = wild; b.wild_cost = penalty;
  ctc_loss_grad_rows(st, b, dlogits, (int)ldd, h[0], h[U] - h[0], train ? 1 : 0);
  return sc.done();
}

int tfk_label_edit_distance(void* stream, const int32_t* hyp, const int32_t* hyp_off, const int32_t* ref,
                            const int32_t* ref_off, int32_t U, int32_t* dist) {
  if (U < 0) return fail(-1, "U = %d < 0", U);
  if (U == 0) return 0;
  if (!hyp_off || !ref_off || !dist) return fail(-1, "hyp_off / ref_off / dist is NULL");
  label_edit_distance((hipStream_t)stream, hyp, hyp_off, nullptr, ref, ref_off, U, kCtcMaxLabels, dist);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"
