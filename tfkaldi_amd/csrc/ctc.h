// CTC loss on the device (BASELINE configs[4]): what the reference's CTCTrainer means to build with
// tf.nn.ctc_loss (neuralNetworks/trainer.py:558-570) -- time-major logits, blank = LAST class, repeated labels merged,
// per-utterance loss -log p(labels | logits) -- as a clean-room implementation of the published forward-backward
// recursion (Graves et al. 2006) in log space.  The reference's own method cannot run, so there is no reference
// behaviour to match; the checker is oracle/ctc_oracle.py, itself pinned against torch's CPU ctc_loss.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "kernels.h"

namespace tfk {

struct CtcBatch {
  const float* logits;     // [T, ld] pre-softmax outputs of the flat, utterance-major frames
  int ld;
  float* post;             // [T, ld] scratch: softmax(logits)
  float* lse;              // [T]     scratch: log-sum-exp of every row
  const int32_t* seg;      // [U + 1] first row of every utterance
  const int32_t* labels;   // concatenated label sequences, values in [0, O - 1)
  const int32_t* lab_off;  // [U + 1] first label of every utterance
  int U, T, O;
  int sext;                // row stride of lp / ab: >= 2 * (longest label sequence) + 1, a multiple of 64 * R
  float* lp;               // [T, sext] scratch: log p_t(state s), states = blank, l_0, blank, l_1, ..., blank
  float* ab;               // [T, sext] scratch: forward variables alpha~ (relative to off)
  float* bb;               // [T, sext] scratch: backward variables beta~ (relative to offb); gradient only
  double* off;             // [T]     scratch: per-frame offset of the re-centred forward variables
  double* offb;            // [T]     scratch: the same for the backward variables
  double* logz;            // [U]     scratch: log p(labels) in double
  float* utt_loss;         // [U] out: -log p, +inf for an utterance too short for its labels
  // Wildcard gaps (the contract is the comment at tfk_accumulate_ctc_wild in tfkaldi_hip.h): gap g of utterance u (the even
  // state 2g) whose flag wild[lab_off[u] + u + g] is non-zero emits exp(-wild_cost) instead of p_t(blank).  NULL: no flag
  // set, and every value is the plain loss's bit for bit (MWER's pair-level batches and MMI's numerator leave it so).
  const uint8_t* wild = nullptr;
  float wild_cost = 0.f;
};

// Longest label sequence the wave-per-utterance recursion handles (64 lanes x 16 states).
constexpr int kCtcMaxLabels = (64 * 16 - 1) / 2;
// sext for a batch whose longest label sequence has max_labels entries
int ctc_state_stride(int max_labels);

// with_grad: dlogits [T, ld] <- softmax - state posteriors folded onto the classes (zero rows for utterances with an
// infinite loss); tw: bf16 twin of dlogits (mixed-precision mode).  Without with_grad only utt_loss is produced.
// With b.wild the loss is the value of the lattice with wildcard gaps and dlogits <- softmax * (1 - W_t) - the posteriors of
// the label and blank-gap states folded onto the classes, W_t = the posterior mass of the frame's wildcard states.
void ctc_loss_grad(hipStream_t s, const CtcBatch& b, float* dlogits, int with_grad, Twin tw);
// The same for a batch whose utterances cover only rows [row0, row0 + rows) of the T rows, with dlogits of its own row stride
// ldd >= O: only those rows of dlogits are written, columns [O, ldd) as zero; no twin.  What tfk_ctc_wild_loss_logits calls.
// dlogits may be the logits themselves when ldd == b.ld (the gradient reads post, never the logits).
void ctc_loss_grad_rows(hipStream_t s, const CtcBatch& b, float* dlogits, int ldd, int row0, int rows, int with_grad);

// scalars[0] (+)= sum of the utterance losses, scalars[1] (+)= number of labels (trainer.py:126-133 counts TARGET
// lengths), scalars[2] (+)= 1
void ctc_loss_reduce(hipStream_t s, const float* utt_loss, const int32_t* lab_off, int U, float* scalars, bool overwrite);

// Best-path decoding (tf.nn.ctc_greedy_decoder, merge_repeated=True) of the utterances seg[U + 1] over logits [T, ld]:
// cls[t] = the frame's largest logit (ties: lowest class; a NaN loses to every number); hyp[seg[u] + n] = utterance u's
// n-th label (repeats merged, then the blank O - 1 removed), -1 on its remaining rows; hyp_len[u] = its label count.
void ctc_best_path(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U, int32_t* cls,
                   int32_t* hyp, int32_t* hyp_len);
// Prefix beam search (Graves 2012; Hannun et al. 2014) with the conventions of
// tf.nn.ctc_beam_search_decoder(merge_repeated=False), on the logits [T, ld] of the utterances seg[U + 1]; blank = the
// LAST class; rows are log-softmaxed inside the kernel.  Per utterance a beam of at most W prefixes, each with (pb, pnb) =
// log-probability of its alignments so far that end in a blank / a non-blank, start {(): (0, -inf)}.  Per frame with
// log-probabilities lp, from every beam prefix p with tot = logaddexp(pb, pnb):
//   stay      p gets pb' (+)= tot + lp[blank] and, if p is not empty, pnb' (+)= pnb + lp[last(p)]
//   extend    q = p + (c,), c in [0, O - 1), gets pnb' (+)= (pb if c == last(p) else tot) + lp[c]
// contributions to one label sequence merge by logaddexp (a q that is itself in the beam: its own pnb term, then its
// parent's extension -- a fixed order); the W candidates with the largest logaddexp(pb', pnb') survive -- ties: shorter
// prefix, then the lower (beam slot, label) of the candidate, which is a fixed function of the input, not of scheduling.
// Out: hyp[n * T + seg[u] + k] = k-th label of utterance u's n-th best prefix (-1 on its remaining rows),
// hyp_len[n * U + u], score[n * U + u] = its natural-log probability; n < top_paths, best first; paths beyond the
// surviving prefixes have length 0 and score -inf (a zero-frame utterance: the empty prefix with score 0, then those).
// trie: ctc_beam_scratch_words(T, U, W) 64-bit words of scratch.  ctc_beam_limits: NULL, or the limit a shape breaks.
// lm == NULL: the search above, by acoustic score alone.  With lm -- a dense character n-gram table on the DEVICE, [C, O]
// row-major, C = ctc_lm_contexts(O, order) = O^(order - 1) -- every prefix also carries g and a context id, candidates are
// ranked by logaddexp(pb', pnb') + g, and the final paths by that (+ weight * lm[ctx][O - 1] with eos); `score` is the
// combined value and am_score (NULL: not wanted) the acoustic part.  The contract is the comment at tfk_ctc_beam_lm in
// tfkaldi_hip.h.  weight = bonus = 0 without eos gives the bits of lm == NULL.
// next != NULL: the model is a deterministic graph over the labels instead (the contract: tfk_ctc_graph_set) -- table is
// weight [num_states, O] (-inf: no such arc; column O - 1: the final weight), next [num_states, O] the transitions, the
// context id is the state, the empty prefix has `start`, and an extension without an arc is no candidate.  `order` is not
// read then.  Both tables have at most kCtcGraphMaxEntries entries.
struct CtcLm {
  const float* table;
  int order;  // in [1, kCtcLmMaxOrder]
  float weight, bonus;
  bool eos;
  const int32_t* next = nullptr;
  int num_states = 0, start = 0;
};
constexpr size_t kCtcGraphMaxEntries = (size_t)1 << 25;
constexpr int kCtcLmMaxOrder = 4;
int ctc_lm_contexts(int O, int order);
constexpr int kCtcBeamMaxWidth = 128;
constexpr int kCtcBeamMaxClasses = 64;
constexpr int kCtcBeamMaxFrames = (1 << 19) - 2;
size_t ctc_beam_scratch_words(int T, int U, int W);
const char* ctc_beam_limits(int O, int T, int U, int W, int top_paths);
void ctc_beam_search(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U, int W,
                     int top_paths, unsigned long long* trie, int32_t* hyp, int32_t* hyp_len, float* score,
                     const CtcLm* lm = nullptr, float* am_score = nullptr);
// The same search with PER-FRAME LABEL PRUNING, for any O up to kCtcTopkMaxClasses (the contract is the comment at
// tfk_ctc_beam_topk in tfkaldi_hip.h): at frame t only the K = min(label_topk, O - 1) labels with the largest logits of row t
// (ties: the lower class) may extend a prefix; a stay still uses the true lp[last(p)].  Candidates of slot i are its kept
// labels in ascending class order, then the stay, so with K == O - 1 (O <= 64) every output equals ctc_beam_search's bit for
// bit.  ctc_beam_topk_rows is the row pre-pass (one wave per row, off the sequential chain): row t of `pre`
// (kCtcTopkRowWords words) = [64 kept labels ascending, 0x7fffffff beyond K | 64 values z - lsum | lsum = mx + logf(se) |
// z[blank] - lsum]; ctc_beam_topk_search is the search on those rows.  pre: ctc_beam_topk_scratch_words(T) 32-bit words,
// trie: ctc_beam_scratch_words(T, U, W) 64-bit words.  lm / am_score as ctc_beam_search, except that am_score (if not NULL) is
// also written without a model, where it equals score; the table has at most kCtcLmMaxEntries entries (ctc_lm_entries:
// O^order, or a value above the limit when it would exceed it).
constexpr int kCtcTopkMaxClasses = 65536;
constexpr int kCtcTopkMaxLabels = 63;
constexpr int kCtcTopkRowWords = 2 * 64 + 2;
constexpr size_t kCtcLmMaxEntries = (size_t)1 << 26;
size_t ctc_lm_entries(int O, int order);
size_t ctc_beam_topk_scratch_words(int T);
const char* ctc_beam_topk_limits(int O, int T, int U, int W, int top_paths, int label_topk);
void ctc_beam_topk_rows(hipStream_t s, const float* logits, int ld, int O, int T, int label_topk, uint32_t* pre);
void ctc_beam_topk_search(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U, int W,
                          int top_paths, int label_topk, unsigned long long* trie, const uint32_t* pre, int32_t* hyp,
                          int32_t* hyp_len, float* score, const CtcLm* lm = nullptr, float* am_score = nullptr);
// The RESUMABLE search (the contract is the comment at tfk_ctc_stream_create in tfkaldi_hip.h): `lanes` independent sessions, one
// workgroup each, whose state outlives the launch.  Per lane: trie = ctc_beam_scratch_words(max_frames, 1, W) 64-bit words (its
// capacity follows max_frames, not the chunk), hdr = kCtcStreamHdrWords 32-bit words, arr = kCtcStreamArrays arrays of W 32-bit
// words (the layout: BeamResume in ctc.hip; the arithmetic of the whole allocation: ctc_stream_layout in ctc_tables.h).
//   ctc_stream_reset   lane (-1: every lane) back to the empty table and the start of a search; stream-ordered memsets
//   ctc_stream_push    the frame loop of ctc_beam_search (label_topk == 0) or ctc_beam_topk_search (pre: the rows of
//                      ctc_beam_topk_rows for THIS chunk) over rows [seg[l], seg[l + 1]) of logits [T, ld] for lane l, from the
//                      lane's saved state to its saved state; lm as above (eos is not read: the end terms of the surviving
//                      prefixes are saved with the state, with lm->weight beside them).  A lane with no row still saves.
//   ctc_stream_result  the N-best of every lane from its saved state, which it leaves as it is: hyp[(n * lanes + l) * stride + k],
//                      k < hyp_len[n * lanes + l] only (stride >= every lane's frame count), score / am_score [n * lanes + l]
//                      (am_score may be NULL).  kind: the model kind the lanes were pushed under; pruned: which search.
// Any split of a lane's frames into pushes leaves the state, and so the result, of the one search over all of them, bit for
// bit: the frame step reads nothing else of the past, and node ids, which differ with the table's capacity, order nothing.
constexpr int kCtcStreamHdrWords = 8;
constexpr int kCtcStreamArrays = 11;
constexpr int kCtcModelNone = 0, kCtcModelNgram = 1, kCtcModelGraph = 2;
struct CtcStreamState {
  int32_t* hdr;
  uint32_t* arr;
  unsigned long long* trie;
  int lanes, W, max_frames;
};
void ctc_stream_reset(hipStream_t s, const CtcStreamState& st, int lane);
void ctc_stream_push(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, const CtcStreamState& st,
                     int label_topk, const uint32_t* pre, const CtcLm* lm);
void ctc_stream_result(hipStream_t s, const CtcStreamState& st, int kind, bool eos, bool pruned, int top_paths, int stride,
                       int32_t* hyp, int32_t* hyp_len, float* score, float* am_score);
// Forced alignment: the most probable path through the CTC lattice of every utterance's KNOWN label sequence (the contract
// is the comment at tfk_ctc_align in tfkaldi_hip.h).  States as the loss: n = 2S + 1, blank, l_0, blank, ..., blank;
// transitions as ctc_alpha_beta (stay, +1, +2 into a label that differs from the label two states back); start in state
// 0 or 1, end in n - 1 or n - 2.  The max-plus recursion runs on the RAW logits (a per-row constant does not move the
// argmax), so for logits that are small integers every fp32 value is exact and the tie rule is a fixed function of the
// input: candidates in the order stay, +1, +2, a later one wins only if STRICTLY larger; at the end n - 1 wins unless
// n - 2 is strictly larger.  Out: ali[seg[u] + t] = position j in [0, S) of the label frame t emits, -1 for a blank frame,
// -2 on every row of an utterance without a valid path; score[u] = sum_t (z[t, class] - logsumexp(z[t, :])), -inf without
// a path, for a zero-frame utterance 0 if S == 0 else -inf.  Rows outside every utterance are not written.
// scratch: ctc_align_scratch_bytes(T, max_labels) bytes, 16-byte aligned; max_labels >= every label count (it selects the
// register tile).  ctc_align_limits: NULL, or the limit a shape breaks.
constexpr int kCtcAlignMaxFrames = (1 << 23) - 1;
size_t ctc_align_scratch_bytes(int T, int max_labels);
const char* ctc_align_limits(int O, int T, int U, int max_labels);
void ctc_viterbi_align(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U,
                       const int32_t* labels, const int32_t* lab_off, int max_labels, void* scratch, int32_t* ali,
                       float* score);
// N-best rescoring: score[p] = log p(labels_p | x_u), the natural log of the sum over ALL valid CTC alignments of pair p's
// label sequence labels[lab_off[p], lab_off[p + 1]) on the frames of utterance u = pair_utt[p] (the contract is the comment
// at tfk_ctc_score in tfkaldi_hip.h).  States and transitions as the loss, so score = -(that utterance's CTC loss with those
// labels); -inf for a pair too short for its labels, for a zero-frame utterance 0 if S == 0 else -inf.  The pairs of one
// utterance should be adjacent (they share the rows they read); any order is correct.  fp32 state values relative to a
// running offset kept in double, as the loss.  scratch: ctc_score_scratch_bytes(T) bytes (the rows' log-sum-exps: T floats
// whatever P is); max_labels >= every label count (it selects the register tile).  ctc_score_limits: NULL, or the limit a
// shape breaks.
constexpr int kCtcScoreMaxPairs = 1 << 20;
size_t ctc_score_scratch_bytes(int T);
const char* ctc_score_limits(int O, int T, int U, int P, int max_labels);
void ctc_score(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U,
               const int32_t* pair_utt, int P, const int32_t* labels, const int32_t* lab_off, int max_labels, void* scratch,
               float* score);
// Alignment with WILDCARD GAPS (the contract is the comment at tfk_ctc_align_wild in tfkaldi_hip.h): ctc_viterbi_align's
// lattice, transitions and tie rule; gap g of an utterance (the even state 2g, g in [0, S]) whose flag
// wild[lab_off[u] + u + g] is non-zero emits rowmax[t] = max_c z[t, c] instead of z[t, blank].  wild == NULL: no flag set,
// and ali / score are ctc_viterbi_align's bit for bit.  ali: -1 for a frame in any gap.  free_score[u] =
// sum_t (rowmax[t] - logsumexp(z[t, :])) in double, rounded once (0 for a zero-frame utterance; written for every utterance,
// with or without a path).  scratch: ctc_align_wild_scratch_bytes(T, max_labels) bytes, 16-byte aligned.  Limits:
// ctc_align_limits.
size_t ctc_align_wild_scratch_bytes(int T, int max_labels);
void ctc_viterbi_align_wild(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U,
                            const int32_t* labels, const int32_t* lab_off, const uint8_t* wild, int max_labels,
                            void* scratch, int32_t* ali, float* score, float* free_score);
// Keyword spotting (the contract is the comment at tfk_ctc_spot in tfkaldi_hip.h): for every (utterance, pattern) pair, laid
// out as ctc_score's pairs, the score of ctc_viterbi_align_wild's path of that pattern on that utterance -- the same bits --
// and its span: start[p] = the first frame that emits a label, end[p] = one past the last; S == 0: 0 and 0; no path: -inf, -1,
// -1.  Nothing is stored per frame: the start frame travels with the state values.  The flags of pair p are
// wild[lab_off[p] + p + g].  free_score [U] as above; P == 0 writes only that.  scratch: ctc_spot_scratch_bytes(T) bytes.
// Limits: ctc_score_limits.
size_t ctc_spot_scratch_bytes(int T);
void ctc_spot(hipStream_t s, const float* logits, int ld, int O, int T, const int32_t* seg, int U, const int32_t* pair_utt,
              int P, const int32_t* labels, const int32_t* lab_off, const uint8_t* wild, int max_labels, void* scratch,
              float* score, int32_t* start, int32_t* end, float* free_score);
// Expected label errors over an N-best list (MWER; Prabhavalkar et al. 2018) and their gradient w.r.t. the logits (the contract
// is the comment at tfk_accumulate_ctc_mwer in tfkaldi_hip.h).  Per utterance u with hypotheses y_i (pairs ufirst[u] ..
// ufirst[u + 1]), s_i = log p(y_i | z) as ctc_score defines it, e_i = their Levenshtein distance to the reference:
//   p_i = softmax over the list of s_i (an infeasible pair: 0),  risk[u] = R = sum_i p_i e_i,  w_i = p_i (e_i - R)
//   dlogits[t, c] = sum_i w_i occ_i[t, c] + ctc_weight * (softmax(z_t)[c] - occ_ref[t, c])
// with occ = a label sequence's state posteriors folded onto the classes, what ctc_loss_grad subtracts from the softmax.
// Every pair -- and, with ctc_weight > 0, every reference, as pair P + u -- is one "utterance" of a pair-level CtcBatch: pair p
// owns the scratch rows [prow[p], prow[p + 1]) (as many as its utterance has frames) of lp / ab / bb / off / offb, and
// ctc_alpha_beta_kernel sweeps it as it sweeps an utterance of the loss.  Order of every sum is fixed: see the kernels.
// tab (ctc_mwer_table fills it on the host; ctc_mwer_table_words words):
//   [prow NP + 1 | lab_off NP + 1 | pair_utt NP | ufirst U + 1 | ref_at P | ref_cnt P]
// labels: the hypotheses' labels in pair order, then the references' in utterance order (lab_off / ref_at index it).
// ctc_mwer_limits: NULL, or the limit a shape breaks (PR = the scratch rows of all NP pairs).
struct CtcMwer {
  const float* logits;   // [T, ld]
  int ld, O, T, U;
  const int32_t* seg;    // [U + 1] first row of every utterance
  int P, NP;             // hypothesis pairs; all pairs: P, or P + U with the references appended
  int64_t PR;            // prow[NP]
  int sext;              // ctc_state_stride(longest label sequence of the NP pairs)
  int max_hyp;           // longest hypothesis (selects label_edit_distance's tile)
  float ctc_weight;
  const int32_t* tab;
  const int32_t* labels;
  // scratch (ctc_mwer_carve points these into one block of ctc_mwer_scratch_bytes bytes)
  double *off, *offb, *logz;  // [PR] [PR] [NP]
  float *lp, *ab, *bb;        // [PR, sext]
  float *lse, *utt_loss, *w;  // [T] [NP] [P]
  // out
  float* risk;      // [U]
  float* score;     // [P] log p(y_i | z), -inf for an infeasible pair
  int32_t* edits;   // [P]
};
__host__ __device__ inline const int32_t* ctc_mwer_prow(const CtcMwer& m) { return m.tab; }
__host__ __device__ inline const int32_t* ctc_mwer_lab_off(const CtcMwer& m) { return m.tab + m.NP + 1; }
__host__ __device__ inline const int32_t* ctc_mwer_pair_utt(const CtcMwer& m) { return m.tab + 2 * (m.NP + 1); }
__host__ __device__ inline const int32_t* ctc_mwer_ufirst(const CtcMwer& m) { return m.tab + 2 * (m.NP + 1) + m.NP; }
__host__ __device__ inline const int32_t* ctc_mwer_ref_at(const CtcMwer& m) { return ctc_mwer_ufirst(m) + m.U + 1; }
__host__ __device__ inline const int32_t* ctc_mwer_ref_cnt(const CtcMwer& m) { return ctc_mwer_ref_at(m) + m.P; }
constexpr int64_t kCtcMwerMaxStates = (int64_t)1 << 33;
constexpr int64_t kCtcMwerMaxLds = 64 * 1024;
const char* ctc_mwer_limits(int O, int64_t ld, int T, int U, int P, int max_labels, int64_t PR);
size_t ctc_mwer_table_words(int U, int P, int NP);
// (host arrays; hyp_len[P] in pair order; with_ref appends the references as pairs P .. P + U - 1)
void ctc_mwer_table(const int32_t* utt_len, int U, const int32_t* hyp_count, const int32_t* hyp_len, const int32_t* ref_len,
                    bool with_ref, int32_t* tab);
size_t ctc_mwer_scratch_bytes(int T, int NP, int P, int64_t PR, int sext);
void ctc_mwer_carve(void* scratch, CtcMwer* m);
// risk, score, edits; with dlogits != NULL also rows [row0, row0 + rows) of dlogits [., ldd] (columns beyond O: zero) and
// its twin.  dlogits may be the logits themselves: every read of a row precedes its write.
// stages: the sweeps (row log-sum-exps, emissions, alpha and -- with dlogits -- beta), the weights (edits, risk, score, w), the
// gradient; a caller that times them apart enqueues them one by one, in this order.
constexpr int kCtcMwerSweep = 1, kCtcMwerWeights = 2, kCtcMwerGrad = 4, kCtcMwerAll = 7;
void ctc_mwer(hipStream_t s, const CtcMwer& m, float* dlogits, int ldd, int row0, int rows, Twin tw, int stages = kCtcMwerAll);
// scalars[0] (+)= sum_u risk[u] + ctc_weight * the references' losses, scalars[1] (+)= ref_labels, scalars[2] (+)= 1
void ctc_mwer_loss_reduce(hipStream_t s, const CtcMwer& m, int ref_labels, float* scalars, bool overwrite);
// MMI against a denominator graph (CTC-CRF; the contract is the comment at tfk_accumulate_ctc_mmi in tfkaldi_hip.h): per
// utterance loss = -(log p_ctc(y | z) + lm_scale * G(y)) + log Z, Z = the total likelihood of every label sequence the
// deterministic acceptor G (layout of tfk_ctc_graph_set, final weights always read) accepts, summed exactly by a
// forward-backward sweep over G composed with the CTC topology: one state B_g per graph state (last frame blank or none), one
// state L_a per arc (last frame emitted the arc's label), N = S + A.
// ctc_den_compile (host, once per graph) turns (weight, next) into GATHER-ONLY index tables, so the recursion needs no scatter
// and no atomics.  Arcs are numbered by (label, source), so the composed states of one class are contiguous (the gradient's
// segmented sum reads them in order); K groups = the distinct (target state, label) pairs, numbered by (state, label).
//   tab = [fx A | bx A | g0 S+1 | ffirst S+1 | fterm A | flo K | fhi K | bfirst S+1 | bterm A | blo K | bhi K | cfirst O]
//   fx / bx    per arc: (label << 16) | index into the frame's sums [S + K] that the arc adds to its own value -- forward: the
//              source's group of the arc's own label if it has one (its "all other labels" sum), else the source's total;
//              backward: the target's group of the arc's label
//   g0         per state: its groups;  ffirst / fterm: its incoming arcs ordered by (label, arc), flo / fhi: every group's
//              own run in that list;  bfirst / bterm: its outgoing arcs ordered by label, blo / bhi: the (at most one) arc of
//              the group's label in that list;  cfirst: first arc of every label (cfirst[O - 1] = A)
//   logw       [A arc weights in arc order | S final weights] natural logs, -inf: not final
// A frame of a sweep is two phases with a workgroup barrier between them: (1) one thread per graph state forms
// sums[g] = v[B_g] + all terms and, per group k, sums[S + k] = v[B_g] + the terms OUTSIDE [lo, hi) -- by ADDING a prefix and a
// suffix, never by subtracting from the total; (2) one thread per composed state updates it in place from its own value and
// one entry of sums.  Values are fp32 in the PROBABILITY domain relative to an offset held in double: every frame's vector is
// divided by the previous vector's maximum (known one barrier earlier, so the re-centring costs no barrier of its own; a
// period of one frame, because a grammar that forbids the frame's dominant class loses e^-30 in a single frame of a peaked
// model), the logarithms accumulate in the offset, which is stored per frame.
struct CtcDenGraph {  // host
  int O = 0, S = 0, A = 0, K = 0, N = 0, start = 0;
  std::vector<int32_t> tab;
  std::vector<float> logw;
  // the graph itself for ctc_den_walk: out-arcs of state g are [ofirst[g], ofirst[g + 1]), ordered by label
  std::vector<int32_t> ofirst, olabel, odst;
  std::vector<float> oweight;
};
constexpr int kCtcDenMaxStates = 65536;    // composed states N = S + A
constexpr int kCtcDenMaxClasses = 1024;    // one thread stages one class of the frame's row
constexpr int64_t kCtcDenMaxCells = (int64_t)1 << 31;  // frames x state stride of one direction's scratch (8 GiB)
constexpr size_t kCtcDenMaxLds = 160 * 1024 - 1024;    // of one workgroup's dynamic LDS (the rest: its static arrays)
// NULL, or the limit a graph breaks -- from the two tables alone, before anything is allocated (arcs: the finite entries of
// columns [0, O - 1))
const char* ctc_den_graph_limits(int O, int64_t num_states, int64_t arcs);
// NULL, or the limit a batch breaks on a graph of N composed states
const char* ctc_den_limits(int O, int T, int U, int N);
inline int ctc_den_stride(int N) { return (N + 63) & ~63; }
// weight / next [S, O] as tfk_ctc_graph_set takes them (validated by the caller)
void ctc_den_compile(const float* weight, const int32_t* next, int S, int O, int start, CtcDenGraph* g);
// lm-unscaled G(y) in double: the arc weights along y plus the final weight of the state it reaches; -inf: rejected
double ctc_den_walk(const CtcDenGraph& g, const int32_t* labels, int n);
inline size_t ctc_den_tab_words(int S, int A, int K, int O) { return 4 * (size_t)A + 3 * ((size_t)S + 1) + 4 * (size_t)K + O; }
struct CtcDen {
  const int32_t* tab;  // device copy of CtcDenGraph::tab
  const float* logw;   // device copy of CtcDenGraph::logw
  int O, S, A, K, N, start;
  const float* post;   // [T, ld] softmax rows (ctc_loss_grad leaves them in CtcBatch::post)
  int ld, T, U;
  const int32_t* seg;  // [U + 1]
  float lm_scale, ctc_weight;
  int stride;          // ctc_den_stride(N)
  bool lds;            // residence of the running vector and the sums: LDS, or the workgroup's own global scratch
  bool tab_lds;        // the tables and wexp are copied into LDS too (they fit beside the vector)
  // scratch (ctc_den_carve points these into one block of ctc_den_scratch_bytes bytes)
  double *offa, *offb, *logz;  // [T] [T] [U]
  float *va, *vb;              // [T, stride] every frame's forward / backward vector (vb: gradient only)
  float *wexp;                 // [A + S] exp(lm_scale * logw)
  float *gv, *gs;              // [2U, stride] [2U, S + K] global residence only
  const double* gy;            // [U] lm-unscaled G(reference) (-inf: rejected), filled by the caller
  float* utt_loss;             // [U] out: the MMI loss, +inf for an infeasible / rejected utterance
};
size_t ctc_den_lds_bytes(int O, int N, int S, int K, bool lds);
// where a graph's sweep keeps its data: 0 = the vector and the sums in the workgroup's global scratch, 1 = both in LDS,
// 2 = the index tables and the arc weights in LDS as well -- the one place that decides it (ctc_den_carve follows it)
int ctc_den_residence(int O, int N, int S, int A, int K);
size_t ctc_den_scratch_bytes(const CtcDen& d, bool with_grad);
void ctc_den_carve(void* scratch, CtcDen* d, bool with_grad);  // (sets d->lds, d->tab_lds, d->stride)
// stages, enqueued one by one in this order by a caller that times them apart.  Sweep: wexp, the forward (and, with_grad, the
// backward) sweep, logz, and utt_loss from the numerator's CtcBatch (after ctc_loss_grad on the same stream: logz / utt_loss
// of the references).  Grad: rows [row0, row0 + rows) of dlogits [., ldd] <- occ_den - softmax + (1 + ctc_weight) * g with
// g [., ldg] = softmax - occ_num as ctc_loss_grad wrote it (zero rows for an utterance whose loss is +inf; columns beyond O:
// zero) and the bf16 twin.  dlogits may be g itself: a thread reads an element before it writes it.
// logz_out (NULL: not wanted): [U] floats, log Z per utterance (-inf: no accepted sequence fits)
void ctc_den_sweep(hipStream_t s, const CtcDen& d, const CtcBatch& num, bool with_grad, float* logz_out = nullptr);
void ctc_den_grad(hipStream_t s, const CtcDen& d, const float* g, int ldg, float* dlogits, int ldd, int row0, int rows, Twin tw);
// scalars[0] (+)= sum_u utt_loss (+ ctc_weight * the references' CTC losses), scalars[1] (+)= ref_labels, scalars[2] (+)= 1
void ctc_den_loss_reduce(hipStream_t s, const CtcDen& d, const float* ctc_utt_loss, int ref_labels, float* scalars,
                         bool overwrite);
// tf.edit_distance(normalize=False): dist[u] = Levenshtein distance (unit costs) of hyp[hyp_off[u], + H_u) and
// ref[ref_off[u], ref_off[u + 1]), H_u = hyp_cnt ? hyp_cnt[u] : hyp_off[u + 1] - hyp_off[u].  max_ref >= every reference
// length selects the register tile; a pair with a negative length or a reference longer than min(max_ref rounded up,
// kCtcMaxLabels) gets -1.
void label_edit_distance(hipStream_t s, const int32_t* hyp, const int32_t* hyp_off, const int32_t* hyp_cnt,
                         const int32_t* ref, const int32_t* ref_off, int U, int max_ref, int32_t* dist);

}  // namespace tfk
