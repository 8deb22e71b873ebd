// A CTC decode stream on the host (the contract: tfk_ctc_stream_* in include/tfkaldi_hip.h): what ctc_entries.hip, which owns
// it, and engine.hip, which pushes its own logits into it, share.  The device side is ctc.h's ctc_stream_*; the arithmetic of
// the checks and of the allocation is ctc_tables.h's and runs on the CPU (tools/ctc_stream_check.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "ctc.h"
#include "ctc_tables.h"

struct tfk_ctc_stream;

namespace tfk {

// The model of a push, and what a lane is bound to.  owner: the engine whose model it is (its identity is then `generation`, the
// engine's count of tfk_ctc_lm_set / tfk_ctc_graph_set calls -- an allocator hands a freed pointer out again), NULL: the
// caller's device tables, identified by their pointers.
struct CtcStreamModel {
  int kind = -1;  // -1: unbound; kCtcModelNone / kCtcModelNgram / kCtcModelGraph
  const void* owner = nullptr;
  uint64_t generation = 0;
  const float* table = nullptr;
  const int32_t* next = nullptr;
  int order = 0, num_states = 0, start = 0;
  float weight = 0.f, bonus = 0.f;
};

// phase(1): the row pre-pass follows, phase(2): the search follows, phase(0): the search has been enqueued (the engine books
// its profile rows with it)
typedef std::function<void(int)> CtcStreamPhase;

// Every refusal of a push, before anything is enqueued; nothing of the stream changes.
int ctc_stream_push_checks(const tfk_ctc_stream* s, const char* who, int O, int T, const int32_t* chunk_len,
                           const CtcStreamModel& m);
// The push itself on DEVICE logits [T, ld], stream-ordered on st; the checks have passed.
int ctc_stream_push_launch(tfk_ctc_stream* s, hipStream_t st, const float* logits, int64_t ld, int T, const int32_t* chunk_len,
                           const CtcStreamModel& m, const CtcStreamPhase& phase);

}  // namespace tfk

struct tfk_ctc_stream {
  int device = 0, O = 0, lanes = 0, W = 0, max_frames = 0, label_topk = 0;
  tfk::CtcStreamLayout L = {};
  unsigned char* dev = nullptr;
  // the chunk bounds of a push travel through this pinned table; seg_copied: its last copy has left it
  int32_t* h_seg = nullptr;
  hipEvent_t seg_copied = nullptr;
  bool seg_pending = false;
  std::vector<int32_t> frames;            // [lanes] frames consumed
  std::vector<tfk::CtcStreamModel> bound;  // [lanes]
  tfk::CtcStreamState state() const {
    return {reinterpret_cast<int32_t*>(dev + L.hdr), reinterpret_cast<uint32_t*>(dev + L.arr),
            reinterpret_cast<unsigned long long*>(dev + L.trie), lanes, W, max_frames};
  }
};
