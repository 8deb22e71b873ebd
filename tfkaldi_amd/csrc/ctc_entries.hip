// The stand-alone CTC entries of the C ABI (include/tfkaldi_hip.h): they take a stream and logits in HBM and need no
// tfk_engine.  Host code only -- every kernel is ctc.hip's.  What the entries share is written once here:
//   fetch_tables   the small tables that only the device knows come back first, in one synchronisation
//   ctc_tables.h   the checks of those tables (plain C++, run on the CPU by tools/ctc_tables_check.cpp)
//   Scratch        the call's own stream-ordered scratch, released whatever happened in between
//   carve_batch    a CtcBatch out of one allocation (the arithmetic: ctc_batch_layout in ctc_tables.h)
#include "../../include/tfkaldi_hip.h"
#include "ctc.h"
#include "ctc_stream.h"
#include "ctc_tables.h"
#include "tfk_error.h"

#include <hip/hip_runtime.h>
#include <string.h>

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

constexpr CtcStreamCaps kStreamCaps = {kCtcBeamMaxWidth, kCtcBeamMaxClasses, kCtcBeamMaxFrames, kCtcTopkMaxClasses,
                                       kCtcTopkMaxLabels,  kCtcStreamMaxLanes};

const char* model_name(int kind) {
  return kind == kCtcModelNone ? "no model" : kind == kCtcModelNgram ? "an n-gram table" : kind == kCtcModelGraph ? "a graph" : "nothing";
}
bool same_bits(float a, float b) { return __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b); }
bool same_model(const CtcStreamModel& a, const CtcStreamModel& b) {
  if (a.kind != b.kind || a.owner != b.owner) return false;
  if (a.kind == kCtcModelNone) return true;
  if (a.owner ? a.generation != b.generation : (a.table != b.table || a.next != b.next)) return false;
  return a.order == b.order && a.num_states == b.num_states && a.start == b.start && same_bits(a.weight, b.weight) &&
         same_bits(a.bonus, b.bonus);
}

}  // namespace

namespace tfk {

int ctc_stream_push_checks(const tfk_ctc_stream* s, const char* who, int O, int T, const int32_t* chunk_len,
                           const CtcStreamModel& m) {
  if (O != s->O) return fail(-1, "%s: output_dim %d differs from the stream's O = %d", who, O, s->O);
  CHK(ctc_stream_push_check(who, chunk_len, s->frames.data(), s->lanes, T, s->max_frames));
  for (int l = 0; l < s->lanes; ++l)
    if (s->frames[l] > 0 && !same_model(s->bound[l], m))
      return fail(-1, "%s: lane %d holds %d frames decoded with %s; a push with %s (or other tables, weights or bonus) cannot continue it "
                  "(tfk_ctc_stream_reset first)", who, l, s->frames[l], model_name(s->bound[l].kind), model_name(m.kind));
  return 0;
}

int ctc_stream_push_launch(tfk_ctc_stream* s, hipStream_t st, const float* logits, int64_t ld, int T, const int32_t* chunk_len,
                           const CtcStreamModel& m, const CtcStreamPhase& phase) {
  const CtcStreamState state = s->state();
  int32_t* d_seg = reinterpret_cast<int32_t*>(s->dev + s->L.seg);
  if (s->seg_pending) HIPCHK(hipEventSynchronize(s->seg_copied));  // (the copy of the push before; not its search)
  s->h_seg[0] = 0;
  for (int l = 0; l < s->lanes; ++l) s->h_seg[l + 1] = s->h_seg[l] + chunk_len[l];
  HIPCHK(hipMemcpyAsync(d_seg, s->h_seg, ((size_t)s->lanes + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(s->seg_copied, st));
  s->seg_pending = true;
  // a lane without frames that was bound to another model holds that model's start: it starts again (its table is empty)
  for (int l = 0; l < s->lanes; ++l)
    if (s->bound[l].kind >= 0 && !same_model(s->bound[l], m))
      HIPCHK(hipMemsetAsync(state.hdr + (size_t)l * kCtcStreamHdrWords, 0, kCtcStreamHdrWords * sizeof(int32_t), st));
  const CtcLm lm = {m.table, m.order, m.weight, m.bonus, false, m.next, m.num_states, m.start};
  Scratch sc(st);
  uint32_t* pre = nullptr;
  if (s->label_topk) {
    CHK(sc.get(&pre, ctc_beam_topk_scratch_words(T) * sizeof(uint32_t)));
    if (phase) phase(1);
    ctc_beam_topk_rows(st, logits, (int)ld, s->O, T, s->label_topk, pre);
  }
  if (phase) phase(2);
  ctc_stream_push(st, logits, (int)ld, s->O, T, d_seg, state, s->label_topk, pre, m.kind == kCtcModelNone ? nullptr : &lm);
  if (phase) phase(0);
  CHK(sc.done());
  for (int l = 0; l < s->lanes; ++l) {
    s->frames[l] += chunk_len[l];
    s->bound[l] = m;
  }
  return 0;
}

}  // namespace tfk

namespace {

int stream_push_logits(tfk_ctc_stream* s, void* stream, const float* logits, int64_t ld, int32_t T, const int32_t* chunk_len,
                       const float* lm_dev, int32_t order, const int32_t* next_dev, int32_t num_states, int32_t start,
                       float lm_weight, float label_bonus) {
  const char* who = "tfk_ctc_stream_push_logits";
  if (!s) return fail(-1, "%s: the stream is NULL", who);
  if (T > 0 && !logits) return fail(-1, "%s: logits is NULL", who);
  if (T > 0 && (ld < s->O || ld > 0x7fffffff)) return fail(-1, "%s: ld = %lld outside [O = %d, 2^31)", who, (long long)ld, s->O);
  CtcStreamModel m;
  m.kind = !lm_dev ? kCtcModelNone : next_dev ? kCtcModelGraph : kCtcModelNgram;
  if (next_dev && !lm_dev) return fail(-1, "%s: next without weight", who);
  if (m.kind == kCtcModelNgram) {
    if (order < 1 || order > kCtcLmMaxOrder) return fail(-1, "%s: order %d outside [1, %d]", who, order, kCtcLmMaxOrder);
    if (ctc_lm_entries(s->O, order) > kCtcLmMaxEntries)
      return fail(-1, "%s: a table of order %d over %d outputs has more than %zu entries", who, order, s->O, kCtcLmMaxEntries);
    m.order = order;
  } else if (m.kind == kCtcModelGraph) {
    if (num_states < 1 || start < 0 || start >= num_states)
      return fail(-1, "%s: start %d outside [0, num_states = %d)", who, start, num_states);
    if ((size_t)num_states * (size_t)s->O > kCtcGraphMaxEntries)
      return fail(-1, "%s: a graph of %d states over %d outputs has more than %zu entries per table", who, num_states, s->O,
                  kCtcGraphMaxEntries);
    m.num_states = num_states;
    m.start = start;
  }
  if (m.kind != kCtcModelNone) {
    m.table = lm_dev;
    m.next = next_dev;
    m.weight = lm_weight;
    m.bonus = label_bonus;
  }
  CHK(ctc_stream_push_checks(s, who, s->O, T, chunk_len, m));
  HIPCHK(hipSetDevice(s->device));
  return ctc_stream_push_launch(s, (hipStream_t)stream, logits, ld, T, chunk_len, m, nullptr);
}

}  // namespace

extern "C" {

int tfk_ctc_stream_bytes(int32_t O, int32_t lanes, int32_t beam_width, int32_t max_frames, int32_t label_topk, size_t* bytes) {
  if (!bytes) return fail(-1, "tfk_ctc_stream_bytes: bytes is NULL");
  CHK(ctc_stream_limits("tfk_ctc_stream_bytes", kStreamCaps, O, lanes, beam_width, max_frames, label_topk));
  *bytes = ctc_stream_layout(lanes, beam_width, max_frames, kCtcStreamHdrWords, kCtcStreamArrays).bytes;
  return 0;
}
int tfk_ctc_stream_create(int32_t O, int32_t lanes, int32_t beam_width, int32_t max_frames, int32_t label_topk,
                          tfk_ctc_stream** out) {
  if (!out) return fail(-1, "tfk_ctc_stream_create: out is NULL");
  *out = nullptr;
  CHK(ctc_stream_limits("tfk_ctc_stream_create", kStreamCaps, O, lanes, beam_width, max_frames, label_topk));
  tfk_ctc_stream* s = new tfk_ctc_stream;
  s->O = O; s->lanes = lanes; s->W = beam_width; s->max_frames = max_frames; s->label_topk = label_topk;
  s->L = ctc_stream_layout(lanes, beam_width, max_frames, kCtcStreamHdrWords, kCtcStreamArrays);
  s->frames.assign(lanes, 0);
  s->bound.assign(lanes, CtcStreamModel());
  hipError_t got = hipGetDevice(&s->device);
  if (got == hipSuccess) got = hipMalloc((void**)&s->dev, s->L.bytes);
  if (got == hipSuccess) got = hipHostMalloc((void**)&s->h_seg, ((size_t)lanes + 1) * sizeof(int32_t), hipHostMallocDefault);
  if (got == hipSuccess) got = hipEventCreateWithFlags(&s->seg_copied, hipEventDisableTiming);
  // every lane empty and at the start of a search, before the first call can be enqueued on any stream
  if (got == hipSuccess) got = hipMemset(s->dev + s->L.trie, 0xff, s->L.hdr - s->L.trie);
  if (got == hipSuccess) got = hipMemset(s->dev + s->L.hdr, 0, s->L.bytes - s->L.hdr);
  if (got == hipSuccess) got = hipDeviceSynchronize();
  if (got != hipSuccess) {
    const size_t bytes = s->L.bytes;
    (void)tfk_ctc_stream_destroy(s);
    return fail((int)got, "tfk_ctc_stream_create (%zu bytes): %s", bytes, hipGetErrorString(got));
  }
  *out = s;
  return 0;
}
int tfk_ctc_stream_destroy(tfk_ctc_stream* s) {
  if (!s) return 0;
  hipError_t first = hipSuccess;
  if (s->seg_pending) first = hipEventSynchronize(s->seg_copied);
  for (hipError_t got : {s->dev ? hipFree(s->dev) : hipSuccess, s->h_seg ? hipHostFree(s->h_seg) : hipSuccess,
                         s->seg_copied ? hipEventDestroy(s->seg_copied) : hipSuccess})
    if (first == hipSuccess) first = got;
  delete s;
  HIPCHK(first);
  return 0;
}
int tfk_ctc_stream_reset(tfk_ctc_stream* s, void* stream, int32_t lane) {
  if (!s) return fail(-1, "tfk_ctc_stream_reset: the stream is NULL");
  if (lane < -1 || lane >= s->lanes) return fail(-1, "tfk_ctc_stream_reset: lane %d outside [-1, %d)", lane, s->lanes);
  HIPCHK(hipSetDevice(s->device));
  ctc_stream_reset((hipStream_t)stream, s->state(), lane);
  HIPCHK(hipGetLastError());
  for (int l = lane < 0 ? 0 : lane; l < (lane < 0 ? s->lanes : lane + 1); ++l) {
    s->frames[l] = 0;
    s->bound[l] = CtcStreamModel();
  }
  return 0;
}
int tfk_ctc_stream_frames(tfk_ctc_stream* s, int32_t* frames) {
  if (!s || !frames) return fail(-1, "tfk_ctc_stream_frames: the stream / frames is NULL");
  std::copy(s->frames.begin(), s->frames.end(), frames);
  return 0;
}
int tfk_ctc_stream_push_logits(tfk_ctc_stream* s, void* stream, const float* logits, int64_t ld, int32_t T,
                               const int32_t* chunk_len, const float* lm_dev, int32_t order, const int32_t* next_dev,
                               int32_t num_states, int32_t start, float lm_weight, float label_bonus) {
  return stream_push_logits(s, stream, logits, ld, T, chunk_len, lm_dev, order, next_dev, num_states, start, lm_weight,
                            label_bonus);
}
int tfk_ctc_stream_result(tfk_ctc_stream* s, void* stream, int32_t top_paths, int flags, int32_t* hyp, int32_t hyp_cap,
                          int32_t* hyp_len, float* score, float* am_score) {
  const char* who = "tfk_ctc_stream_result";
  hipStream_t st = (hipStream_t)stream;
  if (!s) return fail(-1, "%s: the stream is NULL", who);
  if (flags & ~TFK_CTC_LM_EOS) return fail(-1, "%s: flags %d, it takes 0 or TFK_CTC_LM_EOS", who, flags);
  CHK(ctc_stream_result_check(who, s->W, top_paths, hyp_cap));
  if (!hyp_len || !score || (hyp_cap > 0 && !hyp)) return fail(-1, "%s: hyp / hyp_len / score is NULL", who);
  int kind = kCtcModelNone;
  for (int l = 0; l < s->lanes; ++l) {
    if (s->bound[l].kind > kCtcModelNone) kind = s->bound[l].kind;
    if ((flags & TFK_CTC_LM_EOS) && s->bound[l].kind <= kCtcModelNone)
      return fail(-1, "%s: TFK_CTC_LM_EOS, and lane %d is %s (the end term is the model's)", who, l,
                  s->bound[l].kind < 0 ? "not bound to a model" : "bound without a model");
  }
  HIPCHK(hipSetDevice(s->device));
  const size_t P = (size_t)top_paths, U = (size_t)s->lanes;
  const int stride = *std::max_element(s->frames.begin(), s->frames.end());
  // [hypotheses P U stride | lengths P U | scores P U | acoustic scores P U]
  const size_t words = P * U * (size_t)stride + 3 * P * U;
  Scratch sc(st);
  int32_t* d_hyp = nullptr;
  CHK(sc.get(&d_hyp, words * sizeof(int32_t)));
  int32_t* d_len = d_hyp + P * U * (size_t)stride;
  float* d_score = reinterpret_cast<float*>(d_len + P * U);
  ctc_stream_result(st, s->state(), kind, (flags & TFK_CTC_LM_EOS) != 0, s->label_topk != 0, top_paths, stride, d_hyp, d_len,
                    d_score, d_score + P * U);
  std::vector<int32_t> h(words);
  hipError_t copied = hipGetLastError();
  if (copied == hipSuccess) copied = hipMemcpyAsync(h.data(), d_hyp, words * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (copied == hipSuccess) copied = hipStreamSynchronize(st);
  CHK(sc.done(copied));
  const int32_t* h_len = h.data() + P * U * (size_t)stride;
  for (size_t p = 0; p < P * U; ++p) {
    const int32_t n = std::min(h_len[p], hyp_cap);
    if (n > 0) memcpy(hyp + p * (size_t)hyp_cap, h.data() + p * (size_t)stride, (size_t)n * sizeof(int32_t));
    for (int32_t j = n > 0 ? n : 0; j < hyp_cap; ++j) hyp[p * (size_t)hyp_cap + j] = -1;
  }
  memcpy(hyp_len, h_len, P * U * sizeof(int32_t));
  memcpy(score, h_len + P * U, P * U * sizeof(float));
  if (am_score) memcpy(am_score, h_len + 2 * P * U, P * U * sizeof(float));
  return 0;
}

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
