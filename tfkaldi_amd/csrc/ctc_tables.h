// Host-side checks of the small CTC tables, and the layout of a CtcBatch carved out of one allocation: plain C++ over host
// arrays, no HIP and no ctc.h (the limits come in as arguments), so tools/ctc_tables_check.cpp runs all of it on the CPU.
// Every check takes the family name ("CTC align", "CTC wild", "CTC score", "CTC spot", "CTC MWER", "CTC MMI") its messages
// open with, fails through tfk::fail and returns 0 or the error code.
//   offset-table form  what a stand-alone *_logits entry sees once its tables are back from the device
//   length-table form  what an engine entry is handed by its caller
#pragma once
#include "tfk_error.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace tfk {

// ---- offset-table form ----

// Utterance bounds seg[U + 1]: no negative length, and [seg[0], seg[U]] inside [0, T] -- or, with `whole`, exactly [0, T].
inline int seg_check(const char* fam, const int32_t* seg, int U, int T, bool whole = false) {
  for (int u = 0; u < U; ++u)
    if (seg[u + 1] < seg[u]) return fail(-1, "%s: utterance %d has a negative length", fam, u);
  if (whole) {
    if (seg[0] != 0 || seg[U] != T) return fail(-1, "%s: seg = [%d, %d] is not [0, T = %d]", fam, seg[0], seg[U], T);
  } else if (seg[0] < 0 || seg[U] > T) {
    return fail(-1, "%s: seg = [%d, %d] outside [0, T = %d]", fam, seg[0], seg[U], T);
  }
  return 0;
}

// Label offsets off[n + 1] of n sequences: no negative length (the message names `unit` -- "utterance" or "pair" -- and the
// `noun` of the length, "" or " reference"), off[0] >= 0, at most `limit` labels in one (limit < 0: the caller's own limits
// function says it).  Returns the longest sequence.
inline int offsets_check(const char* fam, const char* unit, const char* noun, const int32_t* off, int n, int limit,
                         int* longest) {
  int most = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t len = off[i + 1] - off[i];
    if (len < 0) return fail(-1, "%s: %s %d has a negative%s length", fam, unit, i, noun);
    most = len > most ? len : most;
  }
  if (off[0] < 0) return fail(-1, "%s: lab_off[0] = %d < 0", fam, off[0]);
  if (limit >= 0 && most > limit) return fail(-1, "%s: %d labels in one utterance (limit %d)", fam, most, limit);
  *longest = most;
  return 0;
}

// Pair tables pair_utt[P] / off[P + 1]: the offsets as above, every pair's utterance in [0, U) and, with `ordered`, the pairs
// ordered by utterance.  Returns the longest sequence.
inline int pairs_check(const char* fam, const int32_t* pair_utt, const int32_t* off, int P, int U, bool ordered,
                       int* longest) {
  CHK(offsets_check(fam, "pair", "", off, P, -1, longest));
  for (int p = 0; p < P; ++p) {
    if (pair_utt[p] < 0 || pair_utt[p] >= U)
      return fail(-1, "%s: pair %d names utterance %d outside [0, %d)", fam, p, pair_utt[p], U);
    if (ordered && p > 0 && pair_utt[p] < pair_utt[p - 1])
      return fail(-1, "%s: pair %d: the pairs are not ordered by utterance", fam, p);
  }
  return 0;
}

// ---- length-table form ----

// Utterance lengths utt_len[U]: none negative and, with T >= 0, summing to T.
inline int utt_len_check(const char* fam, const int32_t* utt_len, int U, int T) {
  int64_t frames = 0;
  for (int u = 0; u < U; ++u) {
    if (utt_len[u] < 0) return fail(-1, "%s: utterance %d has a negative length", fam, u);
    frames += utt_len[u];
  }
  if (T >= 0 && frames != T)
    return fail(-1, "%s: utterance lengths sum to %lld, expected T = %d", fam, (long long)frames, T);
  return 0;
}

// How a message names a label sequence: "utterance 1", "utterance 1, hypothesis 0" or "utterance 1, pattern 0 (pair 3)".
// (Formatted only when a check fails: the checks run per pair on the training path.)
struct SeqName {
  int u;
  const char* noun;  // NULL: the utterance alone
  int k, pair;       // pair < 0: not named
  const char* str(char (&buf)[96]) const {
    if (!noun) snprintf(buf, sizeof(buf), "utterance %d", u);
    else if (pair < 0) snprintf(buf, sizeof(buf), "utterance %d, %s %d", u, noun, k);
    else snprintf(buf, sizeof(buf), "utterance %d, %s %d (pair %d)", u, noun, k, pair);
    return buf;
  }
};

// One label sequence of n labels at labels + first, its gap flags at wild + first_flag (NULL: none): at most `limit`
// labels, every label in [0, O - 1) (the blank is the last class), every flag 0 or 1.
inline int sequence_check(const char* fam, const SeqName& who, const int32_t* labels, int64_t first, int32_t n,
                          const uint8_t* wild, int64_t first_flag, int O, int limit) {
  char buf[96];
  if (n > limit) return fail(-1, "%s: %s has %d labels (limit %d)", fam, who.str(buf), n, limit);
  if (n > 0 && !labels) return fail(-1, "%s: labels is NULL", fam);
  for (int32_t i = 0; i < n; ++i)
    if (labels[first + i] < 0 || labels[first + i] >= O - 1)
      return fail(-1, "%s: %s: label %d outside [0, %d)", fam, who.str(buf), labels[first + i], O - 1);
  if (wild)
    for (int32_t g = 0; g <= n; ++g)
      if (wild[first_flag + g] > 1)
        return fail(-1, "%s: %s, gap %d: wild is %d, not 0 or 1", fam, who.str(buf), g, (int)wild[first_flag + g]);
  return 0;
}

// The transcripts of U utterances: utt_len[U] frames, label_len[U] labels back to back in `labels`, label_len[u] + 1 gap
// flags per utterance back to back in `wild` (NULL: none).  No negative length, then sequence_check with the utterance
// named; with T >= 0 the utterance lengths must sum to T.  Returns the number of labels.
inline int transcripts_check(const char* fam, const int32_t* utt_len, const int32_t* label_len, const int32_t* labels,
                             const uint8_t* wild, int U, int O, int limit, int T, int64_t* total) {
  int64_t first = 0;
  for (int u = 0; u < U; ++u) {
    const int32_t n = label_len[u];
    if (utt_len[u] < 0 || n < 0) return fail(-1, "%s: utterance %d has a negative length", fam, u);
    CHK(sequence_check(fam, SeqName{u, nullptr, 0, -1}, labels, first, n, wild, first + u, O, limit));
    first += n;
  }
  *total = first;
  return utt_len_check(fam, utt_len, U, T);
}

// The number of (utterance, `noun`) pairs P = sum of hyp_count[U] -- noun: "hypothesis" or "pattern" -- against max_pairs; no
// negative count, no negative utterance length.
inline int pairs_count(const char* fam, const char* noun, const int32_t* hyp_count, const int32_t* utt_len, int U,
                       int max_pairs, int* P) {
  int64_t pairs = 0;
  for (int u = 0; u < U; ++u) {
    if (hyp_count[u] < 0) return fail(-1, "%s: utterance %d has a negative %s count", fam, u, noun);
    if (utt_len[u] < 0) return fail(-1, "%s: utterance %d has a negative length", fam, u);
    pairs += hyp_count[u];
    if (pairs > max_pairs) return fail(-1, "%s: more than %d (utterance, %s) pairs in one call", fam, max_pairs, noun);
  }
  *P = (int)pairs;
  return 0;
}

// The pair tables of those P pairs from hyp_count[U] and label_len[P] (labels back to back in pair order, label_len[p] + 1
// gap flags per pair in `wild`, NULL: none): fills pair_utt[P] and lab_off[P + 1] (either may be NULL), checks every
// sequence with the utterance and the hypothesis named (name_pair: and the pair, as "utterance 1, pattern 0 (pair 3)").
// Returns the longest sequence and, where asked, the number of labels.
inline int pairs_build(const char* fam, const char* noun, bool name_pair, const int32_t* hyp_count, int U,
                       const int32_t* label_len, const int32_t* labels, const uint8_t* wild, int O, int limit,
                       int32_t* pair_utt, int32_t* lab_off, int* longest, int64_t* total = nullptr) {
  int most = 0, p = 0;
  int64_t first = 0;
  char buf[96];
  if (lab_off) lab_off[0] = 0;
  for (int u = 0; u < U; ++u)
    for (int k = 0; k < hyp_count[u]; ++k, ++p) {
      const int32_t n = label_len[p];
      const SeqName who = {u, noun, k, name_pair ? p : -1};
      if (n < 0) return fail(-1, "%s: %s has a negative length", fam, who.str(buf));
      CHK(sequence_check(fam, who, labels, first, n, wild, first + p, O, limit));
      first += n;
      if (pair_utt) pair_utt[p] = u;
      if (lab_off) lab_off[p + 1] = (int32_t)first;
      most = n > most ? n : most;
    }
  *longest = most;
  if (total) *total = first;
  return 0;
}

// ---- the denominator graph of the MMI criterion ----

// Host tables weight / next [num_states, O] of tfk_ctc_den_set and tfk_ctc_mmi_logits (`who` opens the messages): the rules
// of tfk_ctc_graph_set, then the limits of the composed lattice -- limits(O, num_states, arcs) is ctc_den_graph_limits,
// max_states its kCtcDenMaxStates -- all before anything is allocated.
inline int den_tables_check(const char* who, const float* weight, const int32_t* next, int O, int64_t num_states, int start,
                            const char* (*limits)(int, int64_t, int64_t), int max_states) {
  if (num_states < 1) return fail(-1, "%s: num_states %lld < 1", who, (long long)num_states);
  if (const char* why = limits(O, num_states, 0))
    return fail(-1, "%s (%lld states over %d outputs): %s", who, (long long)num_states, O, why);
  if (start < 0 || start >= num_states) return fail(-1, "%s: start %d outside [0, %lld)", who, start, (long long)num_states);
  const size_t n = (size_t)num_states * (size_t)O;
  int64_t arcs = 0;
  for (size_t i = 0; i < n; ++i) {
    const float w = weight[i];
    if (w != w || w == INFINITY) return fail(-1, "%s: entry %zu of weight is NaN or +inf", who, i);
    if (i % O != (size_t)O - 1 && w > -INFINITY) {
      if (next[i] < 0 || next[i] >= num_states)
        return fail(-1, "%s: entry %zu of next is %d, outside [0, %lld)", who, i, next[i], (long long)num_states);
      ++arcs;
    }
  }
  if (const char* why = limits(O, num_states, arcs))
    return fail(-1, "%s (%lld states + %lld arcs = %lld composed states, limit %d): %s", who, (long long)num_states,
                (long long)arcs, (long long)(num_states + arcs), max_states, why);
  return 0;
}

// ---- a CtcBatch in one allocation ----

// Byte offsets of the regions of a CtcBatch of T frames, U utterances, logits rows of ld floats and lattice rows of sext:
//   [lead doubles | off T, offb T, logz U doubles | post T ld | mid floats | lp, ab, bb T sext each | lse T | tail floats]
// doubles first, so that every region is aligned to its element; lead, mid and tail are the caller's own regions.  `bytes`
// is where the tail ends.
struct CtcBatchLayout {
  size_t lead, off, offb, logz, post, mid, lp, ab, bb, lse, tail, bytes;
};
inline CtcBatchLayout ctc_batch_layout(int T, int U, int64_t ld, int sext, size_t lead_doubles = 0, size_t mid_floats = 0,
                                       size_t tail_floats = 0) {
  const size_t t = (size_t)T, u = (size_t)U, row = (size_t)ld, s = (size_t)sext;
  CtcBatchLayout L;
  size_t at = 0;
  L.lead = at;  at += lead_doubles * sizeof(double);
  L.off = at;   at += t * sizeof(double);
  L.offb = at;  at += t * sizeof(double);
  L.logz = at;  at += u * sizeof(double);
  L.post = at;  at += t * row * sizeof(float);
  L.mid = at;   at += mid_floats * sizeof(float);
  L.lp = at;    at += t * s * sizeof(float);
  L.ab = at;    at += t * s * sizeof(float);
  L.bb = at;    at += t * s * sizeof(float);
  L.lse = at;   at += t * sizeof(float);
  L.tail = at;  at += tail_floats * sizeof(float);
  L.bytes = at;
  return L;
}

// ---- a CTC decode stream (tfk_ctc_stream_*) ----

// The numbers of the search that the checks below need (ctc.h's constants, handed in so that this file stays free of HIP).
struct CtcStreamCaps {
  int max_width, max_classes, max_frames, topk_max_classes, topk_max_labels, max_lanes;
};
constexpr int kCtcStreamMaxLanes = 1024;

// The shape of a stream (`who` opens the messages): NULL-free arithmetic only, nothing is allocated.
inline int ctc_stream_limits(const char* who, const CtcStreamCaps& c, int O, int lanes, int W, int max_frames, int label_topk) {
  if (lanes < 1 || lanes > c.max_lanes) return fail(-1, "%s: lanes %d outside [1, %d]", who, lanes, c.max_lanes);
  if (W < 1 || W > c.max_width) return fail(-1, "%s: beam_width %d outside [1, %d]", who, W, c.max_width);
  if (max_frames < 1 || max_frames > c.max_frames)
    return fail(-1, "%s: max_frames %d outside [1, %d]", who, max_frames, c.max_frames);
  if (label_topk < 0 || label_topk > c.topk_max_labels)
    return fail(-1, "%s: label_topk %d outside [0, %d]", who, label_topk, c.topk_max_labels);
  const int most = label_topk ? c.topk_max_classes : c.max_classes;
  if (O < 2 || O > most)
    return fail(-1, "%s: output_dim %d outside [2, %d]%s", who, O, most, label_topk ? "" : " (63 labels + blank, more with label_topk)");
  return 0;
}

// One push of T rows cut into chunk_len[lanes]: no NULL, no negative length, the lengths sum to T, no lane passes max_frames
// (frames[lanes]: what each lane holds).
inline int ctc_stream_push_check(const char* who, const int32_t* chunk_len, const int32_t* frames, int lanes, int T,
                                 int max_frames) {
  if (!chunk_len) return fail(-1, "%s: chunk_len is NULL", who);
  if (T < 0) return fail(-1, "%s: T = %d < 0", who, T);
  int64_t rows = 0;
  for (int l = 0; l < lanes; ++l) {
    if (chunk_len[l] < 0) return fail(-1, "%s: lane %d has a negative chunk length", who, l);
    rows += chunk_len[l];
  }
  if (rows != T) return fail(-1, "%s: the chunk lengths sum to %lld, expected T = %d", who, (long long)rows, T);
  for (int l = 0; l < lanes; ++l)
    if ((int64_t)frames[l] + chunk_len[l] > max_frames)
      return fail(-1, "%s: lane %d would hold %lld frames (max_frames %d)", who, l, (long long)frames[l] + chunk_len[l],
                  max_frames);
  return 0;
}

// What a result may be asked for.
inline int ctc_stream_result_check(const char* who, int W, int top_paths, int hyp_cap) {
  if (top_paths < 1 || top_paths > W) return fail(-1, "%s: top_paths %d outside [1, beam_width = %d]", who, top_paths, W);
  if (hyp_cap < 0) return fail(-1, "%s: hyp_cap %d < 0", who, hyp_cap);
  return 0;
}

// Byte offsets of the regions of a stream's one allocation:
//   [trie lanes x (2 max_frames W + 64) 64-bit words | hdr lanes x hdr_words | arr lanes x arrays x W | seg lanes + 1], 32-bit
// words behind the 64-bit ones, and hdr_words even (a lane's header holds a double at word 4), so that every region is aligned
// to its element.  `bytes` is where seg ends.
struct CtcStreamLayout {
  size_t trie, hdr, arr, seg, bytes;
  size_t lane_trie_words;
};
inline CtcStreamLayout ctc_stream_layout(int lanes, int W, int max_frames, int hdr_words, int arrays) {
  const size_t n = (size_t)lanes, w = (size_t)W;
  CtcStreamLayout L;
  L.lane_trie_words = 2 * (size_t)max_frames * w + 64;
  size_t at = 0;
  L.trie = at;  at += n * L.lane_trie_words * sizeof(uint64_t);
  L.hdr = at;   at += n * (size_t)hdr_words * sizeof(int32_t);
  L.arr = at;   at += n * (size_t)arrays * w * sizeof(uint32_t);
  L.seg = at;   at += (n + 1) * sizeof(int32_t);
  L.bytes = at;
  return L;
}

}  // namespace tfk
