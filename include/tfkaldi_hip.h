/*
 * tfkaldi_hip.h -- C ABI of the MI355X (gfx950) DNN acoustic-model training engine.
 *
 * This is the drop-in boundary for the hot path of vrenkens/tfkaldi: everything the reference runs
 * inside `tf.Session.run()` for neuralNetworks/trainer.py (Trainer / CrossEnthropyTrainer),
 * neuralNetworks/decoder.py (Decoder) and neuralNetworks/classifiers/{dnn,layer,activation}.py.
 * The reference has no FFI of its own (its "native layer" is TensorFlow); each entry point below names
 * the TensorFlow graph fetch (reference file:line) it replaces.  A Python host binds it with ctypes
 * (tfkaldi_amd/_lib.py); see INTEGRATION.md.
 *
 * Conventions: plain C, every call returns 0 on success or a non-zero status (tfk_last_error() gives
 * the message, thread-local).  Host buffers are caller-owned and only read/written during the call.
 * One engine per GPU; calls on one engine must be serialised by the caller; all device work is
 * stream-ordered on the engine's HIP stream.  Matrices are dense row-major fp32 unless a leading
 * dimension is given.
 */
#ifndef TFKALDI_HIP_H
#define TFKALDI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFK_ABI_VERSION 21

typedef struct tfk_engine tfk_engine;

/* Arithmetic of the affine / gradient contractions.  TFK_DTYPE_F32 is the reference's (exact-fp32 MFMA).
 * TFK_DTYPE_BF16 is mixed precision (BASELINE cfg3 / cfg4): GEMM operands -- layer inputs, weights, dZ -- are
 * rounded to bfloat16 (round to nearest even), products accumulate in fp32; master parameters, batch-norm
 * statistics, the loss, gradient sums and the Adam update stay fp32. */
/* TFK_DTYPE_F32X3: fp32 arithmetic EMULATED on the bf16 matrix pipe.  Every GEMM operand is split, exactly, into three
 * bfloat16 pieces (8 + 8 + 8 significand bits) and the six piece products of order <= 2^-16 are accumulated in fp32: products of
 * bf16 values are exact in fp32 and the dropped pairs are below 2^-24 of a product, so a contraction differs from the exact
 * fp32 dot product only by fp32 accumulation error -- against float64 it is at least as close as the fp32 MFMA chain of
 * TFK_DTYPE_F32 (tools/bf16x3_probe.py) -- at 6/16 of that mode's matrix-pipe time.  Parameters, statistics, loss, gradient
 * sums and the optimiser are fp32 as in every mode; held to the same parity bounds as TFK_DTYPE_F32. */
enum { TFK_DTYPE_F32 = 0, TFK_DTYPE_BF16 = 1, TFK_DTYPE_F32X3 = 2 };

/* nonlinearity of the hidden layers: neuralNetworks/nnet.py:48-65 */
enum { TFK_NONLIN_RELU = 0, TFK_NONLIN_SIGMOID = 1, TFK_NONLIN_TANH = 2, TFK_NONLIN_LINEAR = 3 };

/*
 * Network + optimiser description: the `[nnet]` hyper-parameters that reach the TF graph
 * (config/config_AURORA4.cfg:102-153 via neuralNetworks/nnet.py:17-78 and trainer.py:13-15).
 * Hidden layer = affine -> Batchnorm -> nonlin -> L2Norm -> Dropout (activation.py:22-42 order).
 */
typedef struct tfk_config {
  int32_t struct_size;         /* = sizeof(tfk_config) */
  int32_t device;              /* HIP device ordinal */
  int32_t input_dim;           /* F: spliced feature dimension (nnet.py:39) */
  int32_t num_layers;          /* L: hidden layers (dnn.py:28) */
  int32_t num_units;           /* H (dnn.py:29) */
  int32_t output_dim;          /* O: pdf-ids (classifier.py:13) */
  int32_t nonlin;              /* TFK_NONLIN_* */
  int32_t batch_norm;          /* activation.py:145-161 */
  int32_t l2_norm;             /* activation.py:87-111 */
  float keep_prob;             /* activation.py:113-143; >= 1 disables dropout */
  int32_t layerwise_init;      /* dnn.py:81-122 */
  float init_learning_rate;    /* trainer.py:110-112 */
  float learning_rate_decay;   /* trainer.py:110-112 */
  int32_t num_steps;           /* trainer.py:88 */
  int32_t max_frames;          /* initial frame capacity of one accumulate call (grows on demand) */
  uint64_t seed;               /* dropout RNG seed */
  /* TF-0.1x defaults that live outside the reference tree; 0 selects the default in brackets */
  float bn_decay;              /* [0.999] tf.contrib.layers.batch_norm decay */
  float bn_epsilon;            /* [1e-3] */
  float adam_beta1;            /* [0.9]   tf.train.AdamOptimizer */
  float adam_beta2;            /* [0.999] */
  float adam_epsilon;          /* [1e-8] */
  int32_t compute_dtype;       /* TFK_DTYPE_*: arithmetic of the three contractions (0 = fp32, the reference's) */
} tfk_config;

/* ---- lifetime -------------------------------------------------------------------------------- */

/* Bytes of persistent state (parameters, gradient sums, Adam moments, BN moving statistics) an
 * engine of this shape keeps in HBM. */
int tfk_state_bytes(const tfk_config* cfg, size_t* bytes);

/* Build the engine: replaces Trainer.__init__ graph construction (trainer.py:37-215) and
 * Decoder.__init__ (decoder.py:11-47).  Parameters start as the reference initialises them EXCEPT the
 * random hidden weights, which the host injects with tfk_tensor_set (layer.py:39-48: hidden W ~
 * N(0, 1/sqrt(d_in)), biases 0; dnn.py:67-68: output W = 0). */
int tfk_create(const tfk_config* cfg, tfk_engine** out);

/* As tfk_create, but the persistent state lives in caller-provided device memory (e.g. a torch
 * tensor, so torch.distributed can all-reduce views of it) and work is enqueued on `stream`
 * (a hipStream_t; NULL = the engine creates its own).  `state` must be 256-byte aligned, hold
 * tfk_state_bytes() bytes, and outlive the engine. */
int tfk_create_ex(const tfk_config* cfg, void* state, size_t state_bytes, void* stream, tfk_engine** out);

int tfk_destroy(tfk_engine* e);

const char* tfk_last_error(void);
int tfk_abi_version(void);
/* Build provenance: the hash of the sources this library was compiled from (tfkaldi_amd/build.py source_id(): every
 * .hip / .h under csrc/, this header, the compiler flags).  The binding refuses a library whose id is not its tree's. */
const char* tfk_build_id(void);

/* ---- state access (checkpointing, weight injection, parity tests) ------------------------------ */

enum { /* tensor kind */
  TFK_WEIGHTS = 0,         /* layer l in [0, L]: [d_in, d_out] row-major (layer.py:42-44) */
  TFK_BIASES = 1,          /* [d_out]                                  (layer.py:46-48) */
  TFK_BN_BETA = 2,         /* layer l in [0, L): [H]   (batch_norm center=True, scale=False) */
  TFK_BN_MOVING_MEAN = 3,  /* [H] init 0 */
  TFK_BN_MOVING_VAR = 4    /* [H] init 1 */
};
enum { /* tensor slot */
  TFK_SLOT_PARAM = 0,
  TFK_SLOT_GRAD = 1,       /* the `gradients/...` accumulators G (trainer.py:118-122) */
  TFK_SLOT_ADAM_M = 2,
  TFK_SLOT_ADAM_V = 3
};
int tfk_tensor_count(tfk_engine* e, int kind, int layer, size_t* count);
int tfk_tensor_get(tfk_engine* e, int kind, int slot, int layer, float* host, size_t count);
int tfk_tensor_set(tfk_engine* e, int kind, int slot, int layer, const float* host, size_t count);

enum { /* scalars */
  TFK_GLOBAL_STEP = 0,          /* trainer.py:98-100 */
  TFK_LEARNING_RATE_FACT = 1,   /* trainer.py:104-106 */
  TFK_INITIALISED_LAYERS = 2,   /* dnn.py:85-89 */
  TFK_ADAM_STEPS = 3,           /* Adam's own step count t (beta powers); NOT checkpointed by the reference */
  TFK_BATCH_LOSS = 4,           /* trainer.py:91-93  (read-only) */
  TFK_NUM_FRAMES = 5,           /* trainer.py:126-128 (read-only) */
  TFK_LEARNING_RATE = 6         /* current decayed rate (read-only) */
};
int tfk_scalar_get(tfk_engine* e, int which, double* value);
int tfk_scalar_set(tfk_engine* e, int which, double value);

/* ---- training: one micro-batch --------------------------------------------------------------- */

enum { /* flags */
  TFK_DEVICE_PTRS = 1,     /* X / y / out are device pointers (already resident in HBM) */
  TFK_LAST_MICROBATCH = 2, /* last accumulate before tfk_apply: fire the bucket callback per layer */
  TFK_LOG_DIV_PRIOR = 4,   /* tfk_posteriors: write log(posterior / prior) (nnet.py:280-286) */
  TFK_RAW_LOGITS = 8,      /* tfk_posteriors: write the logits (Classifier.__call__ output, dnn.py:108) */
  TFK_RAW_DEVICE = 16,     /* the *_raw entry points: `raw` is a device pointer -- features that never left HBM, e.g. the output
                            * of tfk_feat_compute; everything else (y, utt_len, cmvn, out) stays a host pointer.  The producer's
                            * work must be complete, or ordered before the engine's stream (tfk_stream), when the call is made. */
  TFK_CTC_LM_EOS = 32,     /* tfk_ctc_beam_lm*: the final ranking and score add the model's end-of-sequence term */
  TFK_CTC_LM = 64          /* tfk_ctc_beam_topk*: the engine's language model ranks the prefixes */
};

/* Replaces `update_gradients_op.run(feed_dict)` (trainer.py:160-169, 325-332) for ONE micro-batch,
 * already flattened utterance-major as seq2nonseq would (seq_convertors.py:12-39):
 *   X [T, ldx] fp32 spliced frames, y [T] int32 pdf-ids.
 * Forward (train mode) + softmax cross-entropy (trainer.py:526-531) + backward;
 * G += g, batch_loss += loss, num_frames += T, BN moving-average updates (UPDATE_OPS). */
int tfk_accumulate(tfk_engine* e, const float* X, int64_t ldx, const int32_t* y, int32_t T, int flags);

/* The step BEFORE the path, moved onto the device: per-speaker mean/variance normalisation and the
 * +-context splice of processing/feature_reader.py:91-156 (apply_cmvn :109-115, splice :117-156).
 * raw [T, ldraw] = the UNSPLICED frames (raw_dim columns, input_dim = raw_dim * (2*context_width + 1)) of U
 * utterances back to back, utt_len[U] their frame counts (sum = T; 0 is allowed anywhere, also for more utterances
 * than there are frames: an empty utterance contributes no row and its cmvn rows are not read).
 * cmvn = NULL: raw is already normalised.  cmvn = [U, 2, raw_dim] fp32: row 0 of utterance u is its speaker's
 * mean, row 1 the standard deviation sqrt(E[x^2] - mean^2); the device computes (raw - mean) / std with the same
 * IEEE roundings as numpy's float32 subtract and divide, so the result is bit-identical to the host path.
 * Frames beyond an utterance's edges splice in as zeros, exactly like the host splice.  Only the unspliced frames
 * cross PCIe (11x less at context 5) and the spliced matrix is produced in HBM.  Host pointers (raw, y, utt_len,
 * cmvn) -- TFK_DEVICE_PTRS is not accepted; TFK_RAW_DEVICE makes `raw` alone a device pointer. */
int tfk_accumulate_raw(tfk_engine* e, const float* raw, int64_t ldraw, const int32_t* y, int32_t T,
                       const int32_t* utt_len, int32_t U, int32_t context_width, const float* cmvn, int flags);
int tfk_eval_accumulate_raw(tfk_engine* e, const float* raw, int64_t ldraw, const int32_t* y, int32_t T,
                            const int32_t* utt_len, int32_t U, int32_t context_width, const float* cmvn, int flags);

/*
 * Several micro-batches of ONE optimiser step in one call -- the same result as calling tfk_accumulate (tfk_accumulate_raw)
 * once per micro-batch in order, `flags` applying to the last one -- so that the engine can STACK them: the reference runs
 * update_gradients_op once per micro-batch (trainer.py:310-332), and at a thousand frames per micro-batch the contractions
 * leave the matrix pipes half idle and re-read every weight matrix k times per step.  A stacked pass multiplies all k
 * micro-batches at once (rows are independent in the affine maps; dW over the stacked rows IS G += g) and keeps per
 * micro-batch whatever couples the rows of one: the batch-norm statistics and their moving-average updates (in order),
 * batch-norm's backward, the dropout stream.  Equal to the sequential calls up to fp32 summation order inside the weight
 * gradients and the loss sum.  Chains the stacked pass does not cover (no batch norm, a nonlinearity other than ReLU,
 * L2Norm, layer-wise growth), micro-batches of more than 2048 frames and env TFK_STACK=0 run one after the other.
 *   tfk_accumulate_stacked      X[T, ldx] (host, or device with TFK_DEVICE_PTRS) = the micro-batches back to back,
 *                               seg_rows[k] frames each
 *   tfk_accumulate_stacked_raw  unspliced frames of U utterances back to back (as tfk_accumulate_raw), seg_utts[k]
 *                               utterances per micro-batch
 */
int tfk_accumulate_stacked(tfk_engine* e, const float* X, int64_t ldx, const int32_t* y, int32_t T, const int32_t* seg_rows,
                           int32_t k, int flags);
int tfk_accumulate_stacked_raw(tfk_engine* e, const float* raw, int64_t ldraw, const int32_t* y, int32_t T,
                               const int32_t* utt_len, int32_t U, int32_t context_width, const float* cmvn,
                               const int32_t* seg_utts, int32_t k, int flags);
/* Trainer.evaluate (reference neuralNetworks/trainer.py:356-441: one update_valid_loss run per micro-batch) over k micro-batches
 * in ONE call.  In evaluation mode the rows of a micro-batch are independent (batch norm normalises with the moving statistics,
 * dropout is the identity, L2Norm is row-wise), so the k runs are one pass of the GEMMs over the concatenated rows -- every
 * activation chain, no padding between segments; passes are cut at micro-batch boundaries once they hold TFK_EVAL_PASS_ROWS rows
 * (default 4096: the host-fed input of the next pass crosses PCIe under the kernels of this one).  batch_loss / num_frames end
 * up as k tfk_eval_accumulate[_raw] calls leave them, up to the fp32 order of the loss sum.  Arguments as the training entry
 * points above. */
int tfk_eval_accumulate_stacked(tfk_engine* e, const float* X, int64_t ldx, const int32_t* y, int32_t T, const int32_t* seg_rows,
                                int32_t k, int flags);
int tfk_eval_accumulate_stacked_raw(tfk_engine* e, const float* raw, int64_t ldraw, const int32_t* y, int32_t T,
                                    const int32_t* utt_len, int32_t U, int32_t context_width, const float* cmvn,
                                    const int32_t* seg_utts, int32_t k, int flags);

/* CTC loss instead of the frame-level cross-entropy (BASELINE configs[4]): what the reference's
 * CTCTrainer.compute_loss means to build with tf.nn.ctc_loss (trainer.py:533-570; its code cannot run, so this is a
 * clean-room implementation of the published forward-backward algorithm with that op's conventions: the blank is
 * the LAST class, repeated labels are merged).  X [T, ldx] = the flat utterance-major frames of U utterances,
 * utt_len[U] their frame counts (sum = T), labels = their label sequences back to back (values in [0, output_dim-1)),
 * label_len[U] the sequence lengths (at most 511 labels per utterance).  batch_loss += sum_u -log p(labels_u | X_u),
 * num_frames += number of labels (the reference counts TARGET lengths, trainer.py:126-133), then backward as
 * tfk_accumulate.  An utterance too short for its labels contributes +inf to the loss and a zero gradient.
 * Host pointers for utt_len / labels / label_len; X as tfk_accumulate (TFK_DEVICE_PTRS allowed). */
int tfk_accumulate_ctc(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                       const int32_t* labels, const int32_t* label_len, int flags);
int tfk_eval_accumulate_ctc(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                            const int32_t* labels, const int32_t* label_len, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_accumulate_raw; the utterance boundaries are
 * shared): 11x less PCIe traffic, which is what bounds a host-fed CTC step on long utterances. */
int tfk_accumulate_ctc_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                           int32_t context_width, const float* cmvn, const int32_t* labels, const int32_t* label_len,
                           int flags);
int tfk_eval_accumulate_ctc_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len,
                                int32_t U, int32_t context_width, const float* cmvn, const int32_t* labels,
                                const int32_t* label_len, int flags);

/* Replaces `[average_loss, apply_gradients_op]` + the three re-initialisations (trainer.py:336-352):
 * g = clip(G / num_frames, -1, 1); Adam; global_step += 1; returns batch_loss / num_frames (the
 * pre-update, train-mode loss); zeroes G, batch_loss, num_frames.  With data parallelism the host
 * all-reduces the reduce region (below) between the last tfk_accumulate and tfk_apply. */
int tfk_apply(tfk_engine* e, float* average_loss);
/* tfk_apply in two halves: tfk_apply_enqueue puts the whole optimiser step on the engine's streams without waiting for it,
 * tfk_apply_end (below) waits for the step's loss.  Between the two the host is free (the dispenser's prefetch). */
int tfk_apply_enqueue(tfk_engine* e);

/* Replaces `update_valid_loss.run(feed_dict)` (trainer.py:188-195, 433): eval-mode forward + loss. */
int tfk_eval_accumulate(tfk_engine* e, const float* X, int64_t ldx, const int32_t* y, int32_t T, int flags);
/* Replaces `average_loss.eval()` + re-initialisation (trainer.py:436-441).
 * Evaluation INSIDE a training step (between the tfk_accumulate* calls of a step and its tfk_apply): the reference keeps one
 * batch_loss / num_frames pair for both, so its validation would cost the step its loss and its gradient scale.  Here the
 * step's sums are set aside when the first tfk_eval_accumulate* of such an evaluation runs and tfk_eval_finish, after
 * reporting the evaluation's own average, puts them back: the step finishes as if nothing had been evaluated.  (Without an
 * evaluation pass in front of it tfk_eval_finish re-initialises whatever the sums hold, as before.) */
int tfk_eval_finish(tfk_engine* e, float* average_loss);

int tfk_halve_learning_rate(tfk_engine* e); /* trainer.py:141-142 */
int tfk_add_layer(tfk_engine* e);           /* control_ops['add']  (dnn.py:92) */
int tfk_init_last_layer(tfk_engine* e);     /* control_ops['init'] (dnn.py:114-120) */

/* ---- decoding -------------------------------------------------------------------------------- */

/* Replaces `Decoder.outputs.eval` (decoder.py:41-44, 70-71): eval-mode forward + softmax.
 * X [N, ldx] -> out [N, ldo] posteriors (or log(posterior/prior) with TFK_LOG_DIV_PRIOR). */
int tfk_posteriors(tfk_engine* e, const float* X, int64_t ldx, int32_t N, float* out, int64_t ldo, int flags);
int tfk_set_prior(tfk_engine* e, const float* prior, size_t count); /* prior.npy (nnet.py:241-244) */
/* As tfk_posteriors on unspliced frames of U utterances (device-side CMVN + splice as tfk_accumulate_raw;
 * several utterances per call = the batched decode of SURVEY 8f-2). */
int tfk_posteriors_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t N, const int32_t* utt_len, int32_t U,
                       int32_t context_width, const float* cmvn, float* out, int64_t ldo, int flags);

/* (ABI 9) Best-path CTC decoding -- tf.nn.ctc_greedy_decoder(merge_repeated=True), the standard evaluation of a model
 * trained with tfk_accumulate_ctc -- and its label errors, tf.edit_distance(normalize=False).  Eval-mode forward of the
 * flat utterance-major frames X [T, ldx] of U utterances (utt_len[U], sum = T), per-frame argmax of the LOGITS (ties: the
 * lowest class; a NaN loses to every number), repeats merged (a blank between two equal classes keeps both), blanks (the
 * LAST class) removed.  hyp[T]: utterance u's labels start at row sum_{v<u} utt_len[v], the rest of its rows are -1;
 * hyp_len[U]: their counts.  With ref_labels / ref_len (back to back, as tfk_accumulate_ctc takes labels: values in
 * [0, output_dim - 1), at most 511 per utterance) and edits[U] non-NULL: edits[u] = Levenshtein distance (unit costs) of
 * hypothesis and reference.  Host pointers.  Evaluation mode; parameters, accumulators and statistics are not touched
 * (same rules as tfk_posteriors).  flags: 0. */
int tfk_ctc_greedy(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                   const int32_t* ref_labels, const int32_t* ref_len, int32_t* hyp, int32_t* hyp_len,
                   int32_t* edits, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_posteriors_raw; flags 0 or TFK_RAW_DEVICE). */
int tfk_ctc_greedy_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                       int32_t context_width, const float* cmvn, const int32_t* ref_labels, const int32_t* ref_len,
                       int32_t* hyp, int32_t* hyp_len, int32_t* edits, int flags);
/* (ABI 10) CTC prefix beam search by acoustic score alone (Graves 2012; Hannun et al. 2014) with the conventions of
 * tf.nn.ctc_beam_search_decoder(merge_repeated=False), and the label errors of its best path.  Eval-mode forward of the flat
 * utterance-major frames X [T, ldx] of U utterances (utt_len[U], sum = T); the LOGITS are log-softmaxed per row; blank = the
 * LAST class; utterances are independent.  The algorithm (this comment is the contract):
 *   Per utterance a beam of at most beam_width prefixes; every prefix p carries (pb, pnb) = the log-probability of all
 *   alignments of p so far that end in a blank / in a non-blank.  Start: {(): (0, -inf)}.  For frame t with
 *   log-probabilities lp, from every beam prefix p with tot = logaddexp(pb, pnb):
 *     stay:    p receives pb' (+)= tot + lp[blank] and, if p is not empty, pnb' (+)= pnb + lp[last(p)];
 *     extend:  for every label c in [0, output_dim - 1), q = p + (c,) receives pnb' (+)= (pb if c == last(p) else tot) + lp[c];
 *     contributions to the same label sequence merge by logaddexp (a q that is itself in the beam collects its own stay terms
 *     and its parent's extension: at most three terms, summed in a fixed order);
 *     the beam_width candidates with the largest logaddexp(pb', pnb') are kept.  Ties: the shorter prefix, then the candidate
 *     with the lower (beam slot of p, label) pair -- a fixed function of the input, so two calls agree bit for bit; it is
 *     NOT the lexicographic order of the label sequences, and nothing should rest on how an exact tie falls.
 *   After the last frame: the top_paths <= beam_width best prefixes by total score, best first.
 * hyp[n * T + row]: path n of utterance u starts at row sum_{v<u} utt_len[v] of plane n, the rest of its rows are -1 (a
 * hypothesis never has more labels than frames); hyp_len[n * U + u]: its label count; score[n * U + u]: its natural-log
 * probability (float; summed in fp32 relative to a running offset kept in double).  A zero-frame utterance has one hypothesis,
 * the empty one with score 0; paths beyond the surviving prefixes have length 0 and score -inf.  With ref_labels / ref_len
 * (as tfk_ctc_greedy) and edits[U] non-NULL: edits[u] = Levenshtein distance of the BEST path to the reference.  NaN logits:
 * the result is unspecified, the call returns.  Limits: 1 <= top_paths <= beam_width <= 128, output_dim <= 64 (63 labels +
 * blank), T <= 524286; a shape outside them returns non-zero and tfk_last_error names the limit.  Host pointers.  Evaluation
 * mode; parameters, accumulators and statistics are not touched (same rules as tfk_ctc_greedy).  flags: 0. */
int tfk_ctc_beam(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                 int32_t beam_width, int32_t top_paths, const int32_t* ref_labels, const int32_t* ref_len, int32_t* hyp,
                 int32_t* hyp_len, float* score, int32_t* edits, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_posteriors_raw; flags 0 or TFK_RAW_DEVICE). */
int tfk_ctc_beam_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                     int32_t context_width, const float* cmvn, int32_t beam_width, int32_t top_paths,
                     const int32_t* ref_labels, const int32_t* ref_len, int32_t* hyp, int32_t* hyp_len, float* score,
                     int32_t* edits, int flags);
/* (ABI 10) Tests / tools: the beam search alone on logits [T, ld] of O classes, stream-ordered on `stream`, DEVICE pointers:
 * seg[U + 1] = first row of every utterance (seg[U] = T); hyp [top_paths * T], hyp_len / score [top_paths * U] as above. */
int tfk_ctc_beam_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                        int32_t beam_width, int32_t top_paths, int32_t* hyp, int32_t* hyp_len, float* score);
/* (ABI 12) The character n-gram language model of tfk_ctc_beam_lm: a DENSE table over the label alphabet.  With O =
 * output_dim (O - 1 labels + the blank index O - 1), order n in [1, 4] and C = O^(n - 1):
 *   table[C][O] float32, row-major, O^n values, all finite (smoothing and back-off are the caller's business: every lookup
 *   is one load).  A context id holds a prefix's last n - 1 labels as base-O digits, the most recent label the least
 *   significant; a position before the utterance's start is the digit O - 1, so the empty prefix has id C - 1 and order 1 the
 *   single row 0; ctx(p + c) = (ctx(p) * O + c) mod C.  table[ctx][c], c < O - 1: the natural-log probability of label c
 *   after that context.  Column O - 1: the log-probability that the sequence ENDS after it (read only under TFK_CTC_LM_EOS).
 * `table` is a HOST pointer to O^order floats; the call copies them to the device (64 MB at O = 64, order 4) and replaces any
 * model the engine holds; table == NULL drops it.  (ABI 13) output_dim <= 65536 and O^order <= 2^26 entries (256 MB: O = 8192
 * at order 2, O = 400 at order 3); a larger table is refused with the limit in the message, before anything is read or
 * allocated.  An order outside [1, 4] or a non-finite entry (tfk_last_error names its index) is rejected too; in every such
 * case the engine keeps the model it had.  A model over more than 64 outputs serves tfk_ctc_beam_topk only.  Parameters, accumulators and statistics are not touched;
 * tfk_ctc_beam / tfk_ctc_beam_raw ignore the model. */
int tfk_ctc_lm_set(tfk_engine* e, const float* table, int32_t order);
/* (ABI 12) CTC prefix beam search with that model (Hannun et al. 2014: prefixes ranked by p_ctc * p_lm^alpha * |prefix|^beta;
 * here in log space, with a per-label bonus for beta).  Everything of tfk_ctc_beam holds unchanged -- states (pb, pnb), stay /
 * extend, merging by logaddexp in the fixed order, log-softmax of the logits.  In addition (this comment is the contract):
 *   every prefix carries a language-model score g and a context id.  The empty prefix has g = 0.  An extension has
 *   g(p + c) = (g(p) + lm_weight * table[ctx(p)][c]) + label_bonus, evaluated in fp32 in exactly that order: g is a function
 *   of the label sequence alone, every route to a prefix computes the same bits (a prefix that is re-created included).  A
 *   prefix that stays keeps its g; an extension that merges into a prefix already in the beam takes that prefix's g.
 *   A candidate's rank key is logaddexp(pb', pnb') + g; the beam keeps the beam_width largest keys.  Ties as tfk_ctc_beam:
 *   the shorter prefix, then the lower (slot, label) pair.  The running offset and the per-frame re-centring stay on the
 *   acoustic part.
 *   After the last frame: the top_paths best prefixes by key; with flag TFK_CTC_LM_EOS the ranking and the reported score add
 *   lm_weight * table[ctx(p)][O - 1].
 * Two scores per path: score[n * U + u] is the combined value (fp32 relative to the double offset, as tfk_ctc_beam's);
 * am_score[n * U + u] (may be NULL) the acoustic part alone, the log-probability of the prefix's surviving alignments --
 * what tfk_ctc_beam calls score.  With lm_weight = label_bonus = 0 and no end flag, hyp, hyp_len and score equal
 * tfk_ctc_beam's bit for bit and am_score == score.  A zero-frame utterance: the empty hypothesis, am_score 0, score 0 or
 * lm_weight * table[C - 1][O - 1] under the end flag; padding paths as tfk_ctc_beam (both scores -inf).  edits[u]: the
 * Levenshtein distance of the best path BY COMBINED SCORE.  Limits: those of tfk_ctc_beam; a model must have been set
 * (tfk_ctc_lm_set), else the call returns non-zero.  flags: 0 or TFK_CTC_LM_EOS. */
int tfk_ctc_beam_lm(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                    int32_t beam_width, int32_t top_paths, float lm_weight, float label_bonus, const int32_t* ref_labels,
                    const int32_t* ref_len, int32_t* hyp, int32_t* hyp_len, float* score, float* am_score, int32_t* edits,
                    int flags);
/* The same on UNSPLICED frames (as tfk_ctc_beam_raw; flags: TFK_RAW_DEVICE and / or TFK_CTC_LM_EOS). */
int tfk_ctc_beam_lm_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                        int32_t context_width, const float* cmvn, int32_t beam_width, int32_t top_paths, float lm_weight,
                        float label_bonus, const int32_t* ref_labels, const int32_t* ref_len, int32_t* hyp,
                        int32_t* hyp_len, float* score, float* am_score, int32_t* edits, int flags);
/* (ABI 12) Tests / tools: that search alone on logits, as tfk_ctc_beam_logits; DEVICE pointers, lm_dev [O^order] included
 * (not checked for finiteness); am_score may be NULL; flags: 0 or TFK_CTC_LM_EOS. */
int tfk_ctc_beam_lm_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                           int32_t beam_width, int32_t top_paths, const float* lm_dev, int32_t order, float lm_weight,
                           float label_bonus, int flags, int32_t* hyp, int32_t* hyp_len, float* score, float* am_score);
/* (ABI 13) CTC prefix beam search with PER-FRAME LABEL PRUNING, for any output_dim up to 65536: per frame only the label_topk
 * most probable labels may start a new label (`cutoff_top_n` elsewhere), which bounds a frame's candidates by
 * beam_width * (K + 1) whatever output_dim is.  Everything of tfk_ctc_beam and tfk_ctc_beam_lm holds unless stated otherwise:
 * the states (pb, pnb), stay and extend, merging by logaddexp in the fixed order, the rank key logaddexp(pb', pnb') + g, ties
 * (the shorter prefix, then the lower candidate index), re-centring on the acoustic part with the offset kept in double, the
 * final ranking, TFK_CTC_LM_EOS, and the layout of hyp, hyp_len, score, am_score, edits.  The differences (this comment is the
 * contract):
 *   K = min(label_topk, O - 1), 1 <= label_topk <= 63.
 *   keep(t), for frame t, is the set of the K labels (never the blank) with the largest logits in row t; among equal logits
 *   the lower class wins.
 *   Extend sees only kept labels: for c not in keep(t) there is no candidate (p, c), and its term does not merge into a beam
 *   prefix that equals p + c either -- the extension behaves as if lp[c] = -inf.
 *   Stay is unchanged: it uses the true lp[blank] and the true lp[last(p)], whether or not last(p) is in keep(t).
 *   Candidates of beam slot i are its kept labels in ascending class order, then the stay candidate; the candidate index (the
 *   last tie-break) is i * (K + 1) + q.  With K = O - 1 this is tfk_ctc_beam's order.
 *   So the search sums exactly the alignments in which every frame that BEGINS a label occurrence -- its class is a label and
 *   differs from the previous frame's class -- has that label in its keep(t); `score` (am_score with a model) stays a lower
 *   bound of the hypothesis' full CTC probability.
 * flags: TFK_CTC_LM -- the engine's model (tfk_ctc_lm_set) ranks the prefixes with lm_weight and label_bonus, as
 * tfk_ctc_beam_lm; non-zero return if none is set.  Without it the search is acoustic, lm_weight / label_bonus are ignored
 * and am_score (may be NULL) equals score.  TFK_CTC_LM_EOS requires TFK_CTC_LM; alone it returns non-zero.
 * Limits: 2 <= output_dim <= 65536, 1 <= top_paths <= beam_width <= 128, T <= 524286, 1 <= label_topk <= 63; a shape outside
 * them returns non-zero and tfk_last_error names the limit.
 * With output_dim <= 64 and label_topk >= output_dim - 1, hyp, hyp_len, score and am_score equal tfk_ctc_beam's /
 * tfk_ctc_beam_lm's bit for bit: the row's log-sum-exp is formed as there (lp = z - (mx + logf(se)), se summed by the same
 * wave butterfly), and the extension by a label and the stay on it use the same fp32 value z - (mx + logf(se)). */
int tfk_ctc_beam_topk(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                      int32_t beam_width, int32_t top_paths, int32_t label_topk, float lm_weight, float label_bonus,
                      const int32_t* ref_labels, const int32_t* ref_len, int32_t* hyp, int32_t* hyp_len, float* score,
                      float* am_score, int32_t* edits, int flags);
/* The same on UNSPLICED frames (as tfk_ctc_beam_raw; flags: those and TFK_RAW_DEVICE). */
int tfk_ctc_beam_topk_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                          int32_t context_width, const float* cmvn, int32_t beam_width, int32_t top_paths, int32_t label_topk,
                          float lm_weight, float label_bonus, const int32_t* ref_labels, const int32_t* ref_len, int32_t* hyp,
                          int32_t* hyp_len, float* score, float* am_score, int32_t* edits, int flags);
/* (ABI 13) Tests / tools: that search alone on logits, as tfk_ctc_beam_lm_logits; DEVICE pointers.  lm_dev == NULL: no model
 * (order, lm_weight, label_bonus ignored, flags must be 0); else lm_dev [O^order <= 2^26]; flags: 0 or TFK_CTC_LM_EOS.
 * am_score may be NULL.  The scratch of the call comes from the stream's memory pool. */
int tfk_ctc_beam_topk_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                             int32_t beam_width, int32_t top_paths, int32_t label_topk, const float* lm_dev, int32_t order,
                             float lm_weight, float label_bonus, int flags, int32_t* hyp, int32_t* hyp_len, float* score,
                             float* am_score);
/* (ABI 16) A FINITE-STATE GRAMMAR in place of the n-gram table: a DETERMINISTIC weighted acceptor over the labels (a lexicon
 * trie, a closed grammar, a backed-off n-gram expanded on the host).  With O = output_dim and S = num_states >= 1:
 *   weight[S][O] float32, row-major.  weight[s][c], c < O - 1: the natural-log weight of the arc that leaves state s with
 *   label c; -inf means THERE IS NO SUCH ARC.  Column O - 1: the final weight of s, -inf = not final; read only under
 *   TFK_CTC_LM_EOS, like the end column of the table.  NaN and +inf are rejected anywhere.
 *   next[S][O] int32: next[s][c] in [0, S) wherever the arc exists; ignored where it does not, and in column O - 1.
 *   start in [0, S).
 * weight alone says whether an arc exists.  Host pointers, copied to the device; S * O <= 2^25 entries per table (128 MB each),
 * a larger model is refused with the limit in the message before anything is read or allocated.  The call replaces whatever
 * model the engine holds, table or graph (tfk_ctc_lm_set likewise replaces a graph); weight == NULL drops it.  A bad start, a
 * NaN / +inf weight or a next out of range on an existing arc (tfk_last_error names the first offending index) is rejected; on
 * any failure the engine keeps the model it had.  A graph over more than 64 outputs serves tfk_ctc_beam_topk only.
 * tfk_ctc_beam_lm[_raw] and tfk_ctc_beam_topk[_raw] under TFK_CTC_LM rank by whichever model is set; signatures, limits and
 * errors are unchanged.  Everything of tfk_ctc_beam_lm (under TFK_CTC_LM: of tfk_ctc_beam_topk) holds; the differences (this
 * comment is the contract):
 *   a prefix carries g and a STATE; the empty prefix has g = 0 and state `start`.
 *   The extension of p by c exists only if weight[state(p)][c] > -inf; otherwise there is no candidate (p, c), as if
 *   lp[c] = -inf (the wording of the pruned search for labels outside keep(t)).  Where it exists,
 *   g(p + c) = (g(p) + lm_weight * weight[state(p)][c]) + label_bonus in the same three roundings, and
 *   state(p + c) = next[state(p)][c].  Stay is unchanged.  The graph is deterministic, so the state, like g, is a function of
 *   the label sequence alone: every route to a prefix computes the same bits, an extension that merges into a beam prefix
 *   takes that prefix's values, and a missing extension can never be one that merges.
 *   The constraint does not depend on lm_weight: with lm_weight = 0 a missing arc is still missing (existence is decided
 *   before any arithmetic on the weight).
 *   Candidate indices, tie-breaks, re-centring on the acoustic part and the double offset are unchanged.  A frame may have
 *   far fewer live candidates than beam_width; the stay candidates are always live, so the beam never empties.
 *   Final ranking by tot + g; under TFK_CTC_LM_EOS + lm_weight * weight[state][O - 1], and a prefix whose state is not final
 *   has the combined value -inf whatever lm_weight is.  It is still listed (labels, hyp_len, finite am_score, score = -inf)
 *   behind every finite one; among themselves such prefixes are ordered like any tie: shorter, then lower slot.
 *   A zero-frame utterance: the empty hypothesis, am_score 0, score 0 or lm_weight * weight[start][O - 1] under the end flag
 *   (-inf if start is not final).
 * Two identities, bit for bit in hyp, hyp_len, score and am_score: (a) the graph next[s][c] = (s * O + c) mod C, weight = table,
 * start = C - 1 reproduces tfk_ctc_beam_lm / tfk_ctc_beam_topk with that table; (b) a one-state graph with every arc, zero
 * weights and lm_weight = label_bonus = 0 reproduces tfk_ctc_beam. */
int tfk_ctc_graph_set(tfk_engine* e, const float* weight, const int32_t* next, int32_t num_states, int32_t start);
/* (ABI 16) Tests / tools: the search with a graph alone on logits, as tfk_ctc_beam_topk_logits; DEVICE pointers, the tables
 * in the layout above and NOT validated.  label_topk == 0: the unpruned search (O <= 64), else the pruned one.  flags: 0 or
 * TFK_CTC_LM_EOS.  am_score may be NULL. */
int tfk_ctc_beam_graph_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                              int32_t beam_width, int32_t top_paths, int32_t label_topk, const float* weight_dev,
                              const int32_t* next_dev, int32_t num_states, int32_t start, float lm_weight, float label_bonus,
                              int flags, int32_t* hyp, int32_t* hyp_len, float* score, float* am_score);
/* (ABI 11) CTC forced alignment: the most probable alignment of every utterance's KNOWN label sequence -- which frames emit
 * which label, and with what probability (time stamps and segments, corpus cleaning by alignment score, frame-level targets).
 * Eval-mode forward of the flat utterance-major frames X [T, ldx] of U utterances (utt_len[U], sum = T); labels / label_len as
 * tfk_accumulate_ctc takes them (back to back, values in [0, output_dim - 1), at most 511 per utterance); blank = the LAST
 * class; utterances are independent.  The algorithm (this comment is the contract), for an utterance of Tn frames with logits
 * z [Tn, O] and labels l_0 ... l_{S-1}:
 *   States as the loss: n = 2S + 1, ordered blank, l_0, blank, l_1, ..., blank; class(s) = the blank for even s, l_{s>>1} for
 *   odd s.  A valid path s_0 ... s_{Tn-1} starts in state 0 or 1, ends in state n - 1 or n - 2, and every step stays, advances
 *   by 1, or advances by 2 -- by 2 only INTO a label state whose label differs from the label two states back.  The result is
 *   the valid path that maximises sum_t z[t, class(s_t)].
 *   The max-plus recursion runs on the RAW LOGITS, not on their log-softmax: a per-row constant does not move the argmax, and
 *   for logits that are small integers every fp32 intermediate is then exact (the state vector is re-centred on its maximum,
 *   which keeps that exactness; the sum of the shifts is kept in double) -- which makes the tie rule a testable, fixed function
 *   of the input.  Ties: at a state the candidates are taken in the order stay, advance by 1, advance by 2, and a later
 *   candidate replaces an earlier one only if it is STRICTLY larger; at the end n - 1 wins unless n - 2 is strictly larger.
 *   In words: of equal predecessors the higher-numbered one wins.
 * ali[T] (on the utterance's rows): for a frame that emits a label the POSITION j of that label, 0 <= j < S (its class is
 * labels[j]; the position, not the class, separates repeated labels); -1 for a blank frame.  score[U]: the natural-log
 * probability of that alignment, sum_t (z[t, class(s_t)] - logsumexp(z[t, :])) (float; fp32 values relative to a running
 * offset kept in double, the rows' log-sum-exps summed in double, as the loss forms log Z).  An utterance too short for its
 * labels (no valid path): score -inf and -2 on all its rows.  A zero-frame utterance: score 0 if S == 0, else -inf.  NaN
 * logits: the result is unspecified, the call returns.  Errors (non-zero, tfk_last_error names the cause): NULL pointers,
 * T <= 0, more than 511 labels, a negative length, a label outside [0, output_dim - 1) (the utterance is named).  Host
 * pointers.  Evaluation mode; parameters, accumulators and statistics are not touched (same rules as tfk_ctc_greedy).
 * flags: 0. */
int tfk_ctc_align(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                  const int32_t* labels, const int32_t* label_len, int32_t* ali, float* score, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_posteriors_raw; flags 0 or TFK_RAW_DEVICE). */
int tfk_ctc_align_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                      int32_t context_width, const float* cmvn, const int32_t* labels, const int32_t* label_len,
                      int32_t* ali, float* score, int flags);
/* (ABI 11) Tests / tools: the alignment alone on logits [T, ld] of O classes, DEVICE pointers: seg[U + 1] = first row of every
 * utterance, lab_off[U + 1] = first label of every utterance in labels; ali [T] (rows outside [seg[0], seg[U]) are not
 * written), score [U] as above.  The two offset tables are read back first (the longest label sequence selects the kernel:
 * one synchronisation of `stream`); the kernels and the call's own scratch are stream-ordered.  Labels are not validated
 * (a value outside [0, O) is clamped). */
int tfk_ctc_align_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                         const int32_t* labels, const int32_t* lab_off, int32_t* ali, float* score);
/* (ABI 14) CTC N-best rescoring: the EXACT log-probability log p(labels | x) of label sequences the caller names -- the
 * hypotheses of a beam search (whose own scores are lower bounds: only the alignments that survived pruning), or any other
 * list -- and their label errors against a reference.  Eval-mode forward of the flat utterance-major frames X [T, ldx] of U
 * utterances (utt_len[U], sum = T).  hyp_count[U] = the number of hypotheses of utterance u, >= 0 (0 is allowed anywhere);
 * P = their sum, at most 2^20 = 1048576.  The (utterance, hypothesis) pairs are ordered by utterance, then by hypothesis;
 * label_len[P] and labels lie back to back in pair order, values in [0, output_dim - 1), at most 511 per hypothesis; blank =
 * the LAST class; pairs are independent.
 * score[P]: the natural log of the sum, over ALL valid CTC alignments of the pair's label sequence on its utterance's frames,
 * of prod_t softmax(z[t, :])[class(s_t)]: states and transitions are the loss's (n = 2S + 1 states blank, l_0, blank, ...,
 * blank; start in state 0 or 1, end in n - 1 or n - 2; a step stays, advances by 1, or advances by 2 into a label that
 * differs from the label two states back), so score = -(the utterance's CTC loss with those labels).  A pair too short for
 * its labels: -inf.  A zero-frame utterance: 0 if S == 0, else -inf.  The emission is z[t, class] - logsumexp(z[t, :]) in
 * fp32; the state values are fp32 relative to a running offset kept in double, and the result is rounded to float once.
 * edits[P] (may be NULL; needs ref_len, and ref_labels where a reference is not empty -- per UTTERANCE, as tfk_ctc_greedy
 * takes them, at most 511 labels each): the Levenshtein distance (unit costs) of every hypothesis to its utterance's reference.
 * P == 0 is valid and writes nothing.  Errors (non-zero, tfk_last_error names the cause; the engine stays usable): NULL
 * pointers, T <= 0, a negative count or length, a hypothesis of more than 511 labels (utterance and hypothesis are named), a
 * label outside [0, output_dim - 1) (named), P > 1048576, edits without ref_len.  Host pointers.  Evaluation mode;
 * parameters, accumulators, moments and statistics are not touched (same rules as tfk_ctc_greedy).  flags: 0. */
int tfk_ctc_score(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                  const int32_t* hyp_count, const int32_t* labels, const int32_t* label_len, const int32_t* ref_labels,
                  const int32_t* ref_len, float* score, int32_t* edits, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_posteriors_raw; flags 0 or TFK_RAW_DEVICE). */
int tfk_ctc_score_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                      int32_t context_width, const float* cmvn, const int32_t* hyp_count, const int32_t* labels,
                      const int32_t* label_len, const int32_t* ref_labels, const int32_t* ref_len, float* score,
                      int32_t* edits, int flags);
/* (ABI 14) Tests / tools: the scores alone on logits [T, ld] of O classes, DEVICE pointers: seg[U + 1] = first row of every
 * utterance, pair_utt[P] = the utterance of pair p (in [0, U); pairs of one utterance should be adjacent), lab_off[P + 1] =
 * first label of every pair in labels; score [P] as above.  Rows outside [seg[0], seg[U]) do not matter.  The three small
 * tables are read back first (the longest hypothesis selects the kernel: one synchronisation of `stream`); the kernels and
 * the call's own scratch (T floats, from the stream's memory pool) are stream-ordered.  Labels are not validated (a value
 * outside [0, O) is clamped). */
int tfk_ctc_score_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                         const int32_t* pair_utt, int32_t P, const int32_t* labels, const int32_t* lab_off, float* score);
/* (ABI 19) CTC ALIGNMENT WITH WILDCARD GAPS, and KEYWORD SPOTTING: a transcript that covers only part of a recording
 * (untranscribed speech, music or noise before and after it, a missing stretch in the middle), a known phrase to be found in a
 * long file, a list of keywords searched in a set of utterances.  torchaudio's forced_align has its "star" token for this; CTC
 * segmentation (Kuerzinger et al. 2020) and CTC keyword spotting are the same lattice with free stretches.  This comment is the
 * contract.
 * Lattice.  For an utterance of Tn frames with logits z [Tn, O], labels l_0 ... l_{S-1} and gap flags w_0 ... w_S:
 *   - States, classes and transitions are those of tfk_ctc_align: n = 2S + 1 states, start in state 0 or 1, end in n - 1 or
 *     n - 2, steps of 0, 1 or 2; a step of 2 goes only into a label state whose label differs from the label two states back.
 *   - Gap g is the even state 2g.  Gap 0 lies before the first label, gap S after the last.
 * Emissions.
 *   - Every label state emits z[t, class], as tfk_ctc_align does.
 *   - A gap with w_g = 0 emits z[t, blank], as tfk_ctc_align does.
 *   - A gap with w_g = 1 is a wildcard: it emits rowmax[t] = max_c z[t, c], the best class of the frame, blank included.
 *   - A wildcard gap may therefore hold anything, including nothing where CTC lets the blank be skipped.  Between two equal
 *     labels it still takes at least one frame.
 * Result and tie rule.
 *   - The result is the valid path that maximises the sum of emissions.
 *   - The tie rule is word for word that of tfk_ctc_align: stay before +1 before +2, a later candidate wins only if it is
 *     strictly larger, and at the end n - 1 wins unless n - 2 is strictly larger.
 *   - The recursion runs on raw logits, re-centred on its maximum, with the sum of the shifts kept in double.
 *   - The wildcard emission is the row maximum and not the row log-sum-exp.  Integer logits therefore still make every fp32
 *     intermediate exact, the tie rule stays a testable function of the input, and the score is the log-probability of one
 *     real frame labelling.
 * Outputs.
 *   - ali[T]: the position j of the label a frame emits; -1 for a frame in any gap, blank or wildcard; -2 on every row of an
 *     utterance without a valid path.
 *   - score[U]: sum_t (emission_t - logsumexp(z[t, :])); sums are kept in double and rounded to float once.  -inf without a path.
 *   - free_score[U]: sum_t (rowmax[t] - logsumexp(z[t, :])), the log-probability of the unconstrained best path,
 *     tfk_ctc_greedy's path (written for every utterance, with or without a path).  score <= free always; score - free is what
 *     the pattern costs against saying whatever fits best; score - free = 0 means the pattern lies on the best path.
 *   - No flag set (or wild == NULL): ali and score equal tfk_ctc_align's bit for bit.
 *   - Zero-frame utterance: free 0, and score 0 if S == 0, else -inf.
 *   - Errors are the same as tfk_ctc_align's, plus a NULL free_score and a wild value other than 0 or 1: the message names the
 *     utterance and the gap.
 * Layout of wild: uint8, S_u + 1 flags per utterance, back to back; utterance u's flags start at lab_off[u] + u (lab_off = the
 * running sum of label_len).  NULL means all zero.
 * Host pointers.  Evaluation mode; parameters, accumulators and statistics are not touched (same rules as tfk_ctc_greedy); the
 * engine stays usable after every refused call.  flags: 0. */
int tfk_ctc_align_wild(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                       const int32_t* labels, const int32_t* label_len, const uint8_t* wild, int32_t* ali, float* score,
                       float* free_score, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_posteriors_raw; flags 0 or TFK_RAW_DEVICE). */
int tfk_ctc_align_wild_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                           int32_t context_width, const float* cmvn, const int32_t* labels, const int32_t* label_len,
                           const uint8_t* wild, int32_t* ali, float* score, float* free_score, int flags);
/* (ABI 19) Tests / tools: the alignment alone on logits [T, ld] of O classes, DEVICE pointers (wild included), tables as
 * tfk_ctc_align_logits takes them; ali [T] (rows outside [seg[0], seg[U]) are not written), score [U], free_score [U].  Labels
 * and flags are not validated (a label outside [0, O) is clamped, any non-zero flag is a wildcard). */
int tfk_ctc_align_wild_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg,
                              int32_t U, const int32_t* labels, const int32_t* lab_off, const uint8_t* wild, int32_t* ali,
                              float* score, float* free_score);
/* (ABI 19) KEYWORD SPOTTING: many patterns per utterance in ONE forward pass, in the pair layout of tfk_ctc_score: hyp_count[U]
 * patterns of utterance u (>= 0, 0 allowed anywhere), P = their sum <= 2^20 = 1048576, pairs ordered by utterance, then by
 * pattern; label_len[P] and labels back to back in pair order, at most 511 labels per pattern.  wild holds S_p + 1 flags per
 * PAIR; pair p's flags start at lab_off[p] + p (NULL: all zero).
 * score[P], start[P], end[P]: for every pair exactly what tfk_ctc_align_wild returns for that utterance and pattern -- score
 * bit for bit, start = the first frame (counted inside the utterance) that emits a label and end = one past the last frame that
 * emits a label, on the same path under the same tie rule.  S == 0: start = end = 0.  No path: score -inf, start = end = -1.
 * free_score[U] as tfk_ctc_align_wild.  No back-pointers are stored (with 2^20 pairs they cannot be): the start frame travels
 * with the state value through the recursion -- set when a path enters state 1 from state 0 or starts in state 1, otherwise
 * inherited from the predecessor the tie rule picked -- and the end frame is read at state n - 1 (the frame at which it was
 * entered from n - 2; Tn if the path ends in n - 2).  P == 0 is valid and writes only free_score.
 * Errors (the engine stays usable): NULL pointers, T <= 0, a negative count or length, a pattern of more than 511 labels, a label
 * outside [0, output_dim - 1), a wild value other than 0 or 1 (utterance, pattern, pair and gap are named), P > 1048576.  Host
 * pointers.  Evaluation mode, as tfk_ctc_greedy.  flags: 0. */
int tfk_ctc_spot(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                 const int32_t* hyp_count, const int32_t* labels, const int32_t* label_len, const uint8_t* wild, float* score,
                 int32_t* start, int32_t* end, float* free_score, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_posteriors_raw; flags 0 or TFK_RAW_DEVICE). */
int tfk_ctc_spot_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                     int32_t context_width, const float* cmvn, const int32_t* hyp_count, const int32_t* labels,
                     const int32_t* label_len, const uint8_t* wild, float* score, int32_t* start, int32_t* end,
                     float* free_score, int flags);
/* (ABI 19) Tests / tools: the search alone on logits [T, ld] of O classes, DEVICE pointers (wild included), tables as
 * tfk_ctc_score_logits takes them (pair_utt[P], lab_off[P + 1]); score / start / end [P], free_score [U].  Labels and flags are
 * not validated (a label outside [0, O) is clamped, any non-zero flag is a wildcard). */
int tfk_ctc_spot_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                        const int32_t* pair_utt, int32_t P, const int32_t* labels, const int32_t* lab_off,
                        const uint8_t* wild, float* score, int32_t* start, int32_t* end, float* free_score);
/* (ABI 20) CTC TRAINING ON PARTIAL TRANSCRIPTS: the CTC loss over the lattice of tfk_ctc_align_wild, under the sum instead of
 * the max.  A flagged gap of the label sequence absorbs any frames at no cost, or at a chosen cost per frame: W-CTC (Cai et
 * al. 2022) and the star token of STC (Pratap et al. 2022).  tfk_accumulate_ctc on a transcript with untranscribed audio
 * before, after or inside it forces those frames onto blanks or the neighbouring labels and teaches deletions; this does not.
 * This comment is the contract.
 * Lattice.  For an utterance of Tn frames with logits z [Tn, O], labels l_0 ... l_{S-1} and gap flags w_0 ... w_S:
 *   - States, start, end and transitions are exactly those of tfk_accumulate_ctc and tfk_ctc_align_wild: n = 2S + 1 states,
 *     start in state 0 or 1, end in n - 1 or n - 2, steps of 0, 1 or 2; a step of 2 goes only into a label state whose label
 *     differs from the label two states back.
 *   - Gap g is the even state 2g, g in [0, S].  Two equal labels with a wildcard gap between them still need one frame in it.
 * Emissions, in the probability domain, with p_t = softmax(z_t):
 *   - a label state emits p_t(label);
 *   - a gap with w_g = 0 emits p_t(blank);
 *   - a gap with w_g = 1 emits exp(-penalty).  penalty is finite and >= 0; at 0 the emission is sum_c p_t(c) = 1, "any
 *     class".  (The STC recipe anneals it.)
 * Loss.  loss_u = -log of the sum, over all paths through the lattice, of the product of the path's emissions.
 *   - This is the VALUE OF THE LATTICE, not a probability: a frame labelling that several lattice paths reach through a
 *     wildcard (a frame of class l_0 may sit in the wildcard gap before l_0 or in l_0's own state) is counted once per PATH,
 *     as W-CTC and STC count it.  The loss can therefore be NEGATIVE: [wild, a, wild] on T frames that put all mass on `a`
 *     has T (T + 1) / 2 paths of value 1 and a loss of -log(T (T + 1) / 2).
 *   - Feasibility is that of the plain loss (the transitions are the same): an utterance too short for its labels gives +inf
 *     and a zero gradient; a zero-frame utterance gives 0 if S == 0, else +inf.
 * Gradient.  dL/dz[t, c] = softmax(z_t)[c] * (1 - W_t) - occ[t, c], with W_t = the posterior mass of the wildcard states at
 * frame t and occ = the posteriors of the other states folded onto their classes (a wildcard's emission does not depend on
 * z).  Every row sums to zero.  The per-frame division of the posteriors by their sum -- applied, as in the plain loss, where
 * that sum is within 1e-2 of one -- is over ALL states, wildcards included.  W_t is summed in a fixed order: two calls give
 * the same bits.
 * Bookkeeping.  batch_loss += sum_u loss_u, num_frames += number of reference labels (as every CTC criterion here), then
 * backward as tfk_accumulate.  TFK_LAST_MICROBATCH, TFK_DEVICE_PTRS, the bf16 twin and the set-aside of an open step's sums
 * during evaluation as for tfk_accumulate_ctc.
 * Layout of wild: that of tfk_ctc_align_wild -- uint8, S_u + 1 flags per utterance, utterance u's flags start at
 * lab_off[u] + u, host pointer, NULL means all zero.  With NULL or all-zero flags batch_loss, num_frames and dLogits are
 * tfk_accumulate_ctc's bit for bit, at any penalty.
 * Errors (non-zero; the accumulators are untouched and the engine stays usable; all checked before the pass starts):
 * everything tfk_accumulate_ctc refuses; a flag other than 0 or 1 (the message names the utterance and the gap); a negative
 * or non-finite penalty (the message names `penalty`). */
int tfk_accumulate_ctc_wild(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                            const int32_t* labels, const int32_t* label_len, const uint8_t* wild, float penalty, int flags);
int tfk_eval_accumulate_ctc_wild(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                                 const int32_t* labels, const int32_t* label_len, const uint8_t* wild, float penalty, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_accumulate_ctc_raw; TFK_RAW_DEVICE allowed). */
int tfk_accumulate_ctc_wild_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                                int32_t context_width, const float* cmvn, const int32_t* labels, const int32_t* label_len,
                                const uint8_t* wild, float penalty, int flags);
int tfk_eval_accumulate_ctc_wild_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len,
                                     int32_t U, int32_t context_width, const float* cmvn, const int32_t* labels,
                                     const int32_t* label_len, const uint8_t* wild, float penalty, int flags);
/* (ABI 20) Tests / tools: the criterion alone on logits [T, ld] of O classes (T > 0), DEVICE pointers (wild included), tables
 * as tfk_ctc_align_wild_logits takes them.  Out: utt_loss [U] and -- unless dlogits is NULL, which asks for utt_loss only --
 * rows [seg[0], seg[U]) of dlogits [T, ldd] = dL/dz as above, columns [O, ldd) written as zero; rows outside are not written.
 * dlogits may be the logits themselves (then ldd == ld).  Stream-ordered on `stream` after the two offset tables have come
 * back (one synchronisation), with the call's own scratch from the stream's memory pool.  Labels, flags and penalty are not
 * validated (any non-zero flag is a wildcard). */
int tfk_ctc_wild_loss_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                             const int32_t* labels, const int32_t* lab_off, const uint8_t* wild, float penalty, float* utt_loss,
                             float* dlogits, int64_t ldd);
/* (ABI 15) Training on the EXPECTED NUMBER OF LABEL ERRORS over an N-best list (MWER; Prabhavalkar et al. 2018, Shannon 2017)
 * instead of -- or on top of -- the CTC likelihood.  Train-mode forward of the flat utterance-major frames X [T, ldx] of U
 * utterances (utt_len[U], sum = T) as tfk_accumulate_ctc; ref_labels / ref_len[U] = the references, laid out as
 * tfk_accumulate_ctc takes its labels; hyp_count[U] / hyp_labels / hyp_len[P] = the hypotheses y_1 .. y_N of every utterance,
 * laid out as tfk_ctc_score takes them (N = hyp_count[u] >= 0, 0 allowed anywhere; pairs ordered by utterance, then by
 * hypothesis; labels and hyp_len back to back in pair order; at most 511 labels each, values in [0, output_dim - 1); blank =
 * the LAST class; P <= 1048576).  A hypothesis listed twice counts twice.  Per utterance, on the logits z of THIS pass
 * (train mode: batch statistics, dropout -- not the evaluation-mode logits the list may have been decoded from):
 *   s_i = log p(y_i | z), tfk_ctc_score's quantity (-inf for a pair too short for its labels; a zero-frame utterance: 0 if
 *         the hypothesis is empty, else -inf);   e_i = Levenshtein(y_i, reference), unit costs
 *   p_i = exp(s_i - m) / sum_j exp(s_j - m), m = the largest s_j (an infeasible pair: p_i = 0)
 *   R_u = sum_i p_i e_i (0 when N = 0 or no pair is feasible),   w_i = p_i (e_i - R_u)
 * formed in double, in pair order, from the pairs' log-probabilities in double; every w_i is rounded to float once.
 *   batch_loss += sum_u R_u + ctc_weight * sum_u -log p(reference_u | z_u)     (the second term only when ctc_weight > 0)
 *   num_frames += the number of REFERENCE labels (as the CTC loss counts), so tfk_apply returns the expected label error rate
 *   (errors per reference label) plus ctc_weight times the CTC loss per label
 *   dL/dz[t, c] = sum_i w_i occ_i[t, c] + ctc_weight * (softmax(z_t)[c] - occ_ref[t, c])
 * with occ_i[t, c] = the state posteriors of y_i at frame t folded onto the classes, what the CTC loss subtracts from the
 * softmax (sum_i w_i = 0, so the softmax terms of the first part cancel); then backward as tfk_accumulate.  Per frame the
 * posteriors of a pair are divided by their sum where that is within 1e-2 of one, as in the CTC loss.  Sums run in a fixed
 * order (pairs in pair order; within a pair the labels in label order) without floating-point atomics: two calls on the same
 * input give the same bits.  A single feasible hypothesis, or hypotheses that all have the same e_i, give a zero gradient
 * (R_u is still reported); hyp_count[u] = 0 leaves only the ctc_weight term; a reference too short for its frames under
 * ctc_weight > 0 adds +inf to the loss and no gradient from that term, as in tfk_accumulate_ctc.
 * Scratch: every (utterance, hypothesis) pair -- and every reference under ctc_weight > 0 -- owns a lattice of its
 * utterance's frames x sext states (sext = 2 * the longest label sequence + 1 rounded up to 128, 256, 512 or 1024): 12 bytes
 * per state.  Limits, refused with a message before anything is launched: more than 2^33 such states in one call; a class row
 * plus a state row, (ldO + sext) * 4 bytes with ldO = output_dim rounded up to the engine's row stride, beyond 64 KiB of LDS.
 * Errors (non-zero, tfk_last_error names the cause -- with the utterance and the hypothesis where there is one; the engine
 * stays usable and its accumulators are untouched): NULL pointers, T <= 0, a negative count or length, a label outside
 * [0, output_dim - 1), a hypothesis or reference of more than 511 labels, ctc_weight negative or not finite, P > 1048576, a
 * shape beyond the limits.  Host pointers for the tables; X as tfk_accumulate_ctc (TFK_DEVICE_PTRS allowed);
 * TFK_LAST_MICROBATCH as everywhere.  The eval variant: evaluation-mode forward, loss only (a validation figure); inside an
 * open step the step's sums are set aside and restored as for every other evaluation. */
int tfk_accumulate_ctc_mwer(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                            const int32_t* ref_labels, const int32_t* ref_len, const int32_t* hyp_count,
                            const int32_t* hyp_labels, const int32_t* hyp_len, float ctc_weight, int flags);
int tfk_eval_accumulate_ctc_mwer(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                                 const int32_t* ref_labels, const int32_t* ref_len, const int32_t* hyp_count,
                                 const int32_t* hyp_labels, const int32_t* hyp_len, float ctc_weight, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_accumulate_ctc_raw; TFK_RAW_DEVICE allowed). */
int tfk_accumulate_ctc_mwer_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                                int32_t context_width, const float* cmvn, const int32_t* ref_labels, const int32_t* ref_len,
                                const int32_t* hyp_count, const int32_t* hyp_labels, const int32_t* hyp_len, float ctc_weight,
                                int flags);
int tfk_eval_accumulate_ctc_mwer_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len,
                                     int32_t U, int32_t context_width, const float* cmvn, const int32_t* ref_labels,
                                     const int32_t* ref_len, const int32_t* hyp_count, const int32_t* hyp_labels,
                                     const int32_t* hyp_len, float ctc_weight, int flags);
/* (ABI 15) Tests / tools: the criterion alone on logits [T, ld] of O classes, DEVICE pointers: seg[U + 1] = first row of every
 * utterance, pair_utt[P] = the utterance of pair p (in [0, U), NON-DECREASING: the pairs of an utterance are adjacent),
 * lab_off[P + 1] = first label of every pair in labels, ref_off[U + 1] = first label of every reference in ref_labels.  Out:
 * risk [U] = R_u, score [P] = s_i, edits [P] = e_i, and -- unless dlogits is NULL, which asks for those three only -- rows
 * [seg[0], seg[U]) of dlogits [., ldd] = dL/dz as above (columns [O, ldd) zero; other rows are not written; the logits are
 * not overwritten).  The loss of the call is sum_u risk[u] plus ctc_weight times the references' CTC losses, which this entry
 * does not return.  The small tables are read back first and the derived tables uploaded (two synchronisations of `stream`);
 * the kernels and the call's own scratch (from the stream's memory pool) are stream-ordered.  Labels are not validated (a
 * value outside [0, O) is clamped where it addresses the logits).  Limits as above with ldO = ld. */
int tfk_ctc_mwer_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                        const int32_t* pair_utt, int32_t P, const int32_t* labels, const int32_t* lab_off,
                        const int32_t* ref_labels, const int32_t* ref_off, float ctc_weight, float* dlogits, int64_t ldd,
                        float* risk, float* score, int32_t* edits);
/* (ABI 17) MAXIMUM MUTUAL INFORMATION against a denominator graph (CTC-CRF; lattice-free MMI with the CTC topology).  The
 * numerator is the CTC likelihood of the reference; the denominator is the total likelihood of EVERY label sequence the graph
 * accepts, summed exactly by a forward-backward sweep over the graph composed with the CTC topology -- nothing is sampled, no
 * beam prunes the sum, and no decode precedes the step.
 * The graph G is a deterministic weighted acceptor in exactly the layout of tfk_ctc_graph_set: weight[S][O], next[S][O],
 * start.  Column O - 1 of weight is the final weight and is ALWAYS read here; a graph in which every state is final at weight
 * 0 expresses "no end constraint".  lm_scale (lambda >= 0, finite) multiplies every graph weight, final weights included.
 * Composed lattice of an utterance with log-softmax rows lp_t: one state B_g per graph state g (we are in g, and the last
 * frame was a blank or there was none), one state L_a per existing arc a = (src, c, dst) (the last frame emitted c while
 * taking a); N = S + A states, A the number of arcs.  In the probability domain, with w_a = exp(lambda weight[src][c]) and
 * f_g = exp(lambda weight[g][O - 1]):
 *   alpha_0[B_start] = p_0(blank);  alpha_0[L_a] = w_a p_0(c_a) for arcs leaving start;  everything else 0
 *   alpha_t[B_g] = p_t(blank) (alpha_{t-1}[B_g] + sum_{a: dst(a) = g} alpha_{t-1}[L_a])
 *   alpha_t[L_a] = p_t(c_a) (alpha_{t-1}[L_a]
 *                            + w_a (alpha_{t-1}[B_src(a)] + sum_{a': dst(a') = src(a), c_a' != c_a} alpha_{t-1}[L_a']))
 *   Z = sum_g f_g (alpha_{T-1}[B_g] + sum_{a: dst(a) = g} alpha_{T-1}[L_a])
 * (c_a' != c_a is CTC's rule that a repeated label needs a blank in between).  The backward variables mirror this, with the
 * emission of frame t included, as the CTC loss has it:
 *   beta_{T-1}[B_g] = f_g p(blank);  beta_{T-1}[L_a] = f_dst(a) p(c_a)
 *   beta_t[B_g] = p_t(blank) (beta_{t+1}[B_g] + sum_{a: src = g} w_a beta_{t+1}[L_a])
 *   beta_t[L_a] = p_t(c_a) (beta_{t+1}[L_a] + beta_{t+1}[B_dst(a)] + sum_{a': src(a') = dst(a), c_a' != c_a} w_a' beta_{t+1}[L_a'])
 * Per utterance u with reference y_u, G(y) = the arc weights along y plus the final weight of the state it reaches:
 *   loss_u      = -(log p_ctc(y_u | z) + lambda G(y_u)) + log Z_u          (>= 0 whenever y_u is accepted)
 *   dL/dz[t, c] = occ_den[t, c] - occ_num[t, c] + ctc_weight (softmax(z_t)[c] - occ_num[t, c])
 *   batch_loss += sum_u loss_u + ctc_weight sum_u -log p_ctc(y_u | z)     (the second term only when ctc_weight > 0)
 *   num_frames += the number of reference labels                         (as every CTC criterion here)
 * occ_num is what the CTC loss subtracts from the softmax; occ_den[t, c] = the posterior of the composed states whose class is
 * c, alpha_t beta_t / (p_t(c) Z), folded onto the classes (the softmax terms of numerator and denominator cancel).  Per frame
 * occ_den is divided by its sum where that sum is within 1e-2 of one, as the loss does for occ_num.
 * If no accepted label sequence fits an utterance's frames (Z = 0), or G does not accept its reference, or the utterance is too
 * short for its labels, the utterance contributes +inf to the loss and a zero gradient.  A zero-frame utterance: loss 0 if the
 * reference is empty and start is final, +inf otherwise.  Sums run in a fixed order with no floating-point atomics: two calls
 * on the same input give the same bits.  A sum "over the other labels" (c_a' != c_a) is formed by ADDING the other terms, never
 * by subtracting one from a total (which cancels catastrophically when one label dominates).
 * Numerics: fp32 values relative to an offset held in double, re-centred every frame by an exact power of two on the
 * previous frame's maximum, offsets stored per frame; log Z, G(y) and the loss in double, rounded once.
 * tfk_ctc_den_set: the denominator is a model of its own, separate from the decoding model of tfk_ctc_graph_set /
 * tfk_ctc_lm_set -- neither call disturbs the other.  Validation as tfk_ctc_graph_set, and the same failure rule: a refused
 * call leaves the old model in force.  weight == NULL drops the model.  Limits, named in the message before anything is
 * allocated: output_dim in [2, 1024]; S x O <= 2^25 entries per table; N = S + A <= 65536 composed states (an order-3 n-gram
 * over 35 characters plus the blank is N = 46656).  The tables are compiled on the host, once per call, into gather-only
 * index lists (incoming arcs of a state grouped by label), so the sweeps need no scatter and no atomics.
 * tfk_accumulate_ctc_mmi and its variants: arguments as tfk_accumulate_ctc, plus lm_scale, ctc_weight.  One workgroup per
 * (utterance, direction); the running vector lives in LDS while [O | N | S + groups] floats fit 159 KiB, in the workgroup's
 * own global scratch beyond.  Scratch: 8 bytes per frame and composed state (rounded up to 64).  Errors (non-zero; the
 * accumulators are untouched and the engine stays usable): those of tfk_accumulate_ctc, checked before the pass starts; no
 * denominator set; lm_scale or ctc_weight negative or not finite; more than 2^31 lattice cells (T x N rounded up to 64).
 * TFK_LAST_MICROBATCH, TFK_DEVICE_PTRS and the set-aside of an open step's sums during evaluation as everywhere else. */
int tfk_ctc_den_set(tfk_engine* e, const float* weight, const int32_t* next, int32_t num_states, int32_t start);
/* What the compile of the denominator graph in force found (any pointer may be NULL): its states S, arcs A, groups K (the
 * distinct (target state, label) pairs; N = S + A) and where its sweeps keep their data -- residence 0: the vector and the
 * sums in the workgroup's global scratch; 1: both in LDS; 2: the index tables and arc weights in LDS as well.  An error when
 * no denominator is set. */
int tfk_ctc_den_info(tfk_engine* e, int32_t* num_states, int32_t* num_arcs, int32_t* num_groups, int32_t* residence);
int tfk_accumulate_ctc_mmi(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                           const int32_t* labels, const int32_t* label_len, float lm_scale, float ctc_weight, int flags);
int tfk_eval_accumulate_ctc_mmi(tfk_engine* e, const float* X, int64_t ldx, int32_t T, const int32_t* utt_len, int32_t U,
                                const int32_t* labels, const int32_t* label_len, float lm_scale, float ctc_weight, int flags);
/* The same on UNSPLICED frames (device-side CMVN + splice as tfk_accumulate_ctc_raw; TFK_RAW_DEVICE allowed). */
int tfk_accumulate_ctc_mmi_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len, int32_t U,
                               int32_t context_width, const float* cmvn, const int32_t* labels, const int32_t* label_len,
                               float lm_scale, float ctc_weight, int flags);
int tfk_eval_accumulate_ctc_mmi_raw(tfk_engine* e, const float* raw, int64_t ldraw, int32_t T, const int32_t* utt_len,
                                    int32_t U, int32_t context_width, const float* cmvn, const int32_t* labels,
                                    const int32_t* label_len, float lm_scale, float ctc_weight, int flags);
/* (ABI 17) Tests / tools: the criterion alone on logits [T, ld] of O classes, DEVICE pointers: seg[U + 1] = first row of every
 * utterance (seg[0] = 0, seg[U] = T > 0), lab_off[U + 1] = first label of every reference in labels (lab_off[0] = 0),
 * weight_dev / next_dev [num_states, O] the graph.  Out: utt_loss [U] = loss_u, logz [U] = log Z_u (-inf: Z = 0) and -- unless
 * dlogits is NULL, which asks for those two only -- dlogits [T, ldd] = dL/dz as above (columns [O, ldd) zero).  dlogits may be
 * the logits themselves.  The tables are read back, compiled and uploaded first (synchronisations of `stream`); the kernels
 * and the call's own scratch (from the stream's memory pool) are stream-ordered. */
int tfk_ctc_mmi_logits(void* stream, const float* logits, int64_t ld, int32_t O, int32_t T, const int32_t* seg, int32_t U,
                       const int32_t* labels, const int32_t* lab_off, const float* weight_dev, const int32_t* next_dev,
                       int32_t num_states, int32_t start, float lm_scale, float ctc_weight, float* utt_loss, float* logz,
                       float* dlogits, int64_t ldd);
/* (ABI 9) Tests / tools: tf.edit_distance(normalize=False) of U pairs of int32 sequences, stream-ordered on `stream`,
 * DEVICE pointers: dist[u] = Levenshtein distance of hyp[hyp_off[u], hyp_off[u + 1]) and ref[ref_off[u], ref_off[u + 1]);
 * hyp_off / ref_off [U + 1]; every reference at most 511 long (a longer one, or a negative length, gives dist[u] = -1). */
int tfk_label_edit_distance(void* stream, const int32_t* hyp, const int32_t* hyp_off, const int32_t* ref,
                            const int32_t* ref_off, int32_t U, int32_t* dist);

/* ---- (ABI 21) streaming CTC decode: the prefix beam search, resumable across chunks --------------
 *
 * A stream holds `lanes` independent sessions (one workgroup each, as the batch search has one per utterance).  A lane owns, in
 * device memory that lives as long as the stream: its trie of 2 * max_frames * beam_width + 64 64-bit words (sized by
 * max_frames, not by a chunk), and the beam after its last frame -- per prefix pb, pnb, tot, node, parent, last, len, src, with
 * a model g and ctx, and the model's END TERM table[ctx][O - 1] (graph: weight[state][O - 1]) gathered when the state is
 * saved, lm_weight beside it -- plus the beam's size, its dead count and the score offset (a double).  A push runs the frame
 * loop of tfk_ctc_beam* over the chunk's rows from that state to that state; a result ranks and traces back from it and needs
 * no model.
 *   IDENTITY.  After pushes whose chunks, concatenated per lane, are z[0:t], tfk_ctc_stream_result gives for that lane what
 *   the one-shot entry (tfk_ctc_beam_logits / _lm_logits / _graph_logits / _topk_logits with the same beam_width, label_topk,
 *   model, lm_weight, label_bonus and flags) gives on z[0:t]: labels, lengths, score and am_score bit for bit, for every t
 *   and every chunking, empty chunks and idle lanes included.  (Node ids differ with the table's capacity; nothing is ordered
 *   by them.)
 *   ZERO FRAMES.  A lane without frames gives the empty hypothesis with am_score 0 (score: 0, or the end term of the start
 *   context under TFK_CTC_LM_EOS), as the one-shot search gives for a zero-frame utterance; padding paths have length 0 and
 *   both scores -inf.
 *   A RESULT READS ONLY.  Asking never changes what later pushes produce.
 *   BINDING.  A lane binds to the model of its first push after a reset; a push that gives it 0 frames counts.  The binding is
 *   the kind (none, table, graph), the identity of the tables, order / num_states / start, lm_weight and label_bonus (bits).
 *   The identity of the engine's model is a counter that every tfk_ctc_lm_set / tfk_ctc_graph_set advances, not its address.
 *   A push under any other model while a lane holds frames returns non-zero and names the lane; a lane without frames binds
 *   anew.  TFK_CTC_LM_EOS on a stream with a lane that is unbound, or bound without a model, returns non-zero.  Reset unbinds.
 *   The model must stay alive during a push (as for the one-shot entries), not after it.
 *   REFUSALS come before anything is enqueued and leave every lane as it was: a NULL pointer, a negative chunk length, lengths
 *   that do not sum to T, a lane that would pass max_frames (the message names the lane and the limit), an output_dim other
 *   than the stream's O, lanes outside [1, 1024], max_frames outside [1, 524286], beam_width / output_dim / label_topk outside
 *   the limits of tfk_ctc_beam (label_topk == 0) or tfk_ctc_beam_topk, top_paths outside [1, beam_width], hyp_cap < 0.
 *   ORDER.  A stream is used from one HIP stream at a time; its calls are stream-ordered.  Only tfk_ctc_stream_result waits.
 * Not here: entries on raw (unspliced) frames -- the device splice pads with zeros at the edges of what it is given, which is
 * wrong in mid-stream (splice on the host: StreamSplicer in the Python package) --, streaming greedy decoding, endpointing,
 * and capture into a hipGraph (a push and a result allocate stream-ordered scratch). */
typedef struct tfk_ctc_stream tfk_ctc_stream;
/* bytes of device memory a stream of this shape holds (16 * max_frames * beam_width per lane dominate) */
int tfk_ctc_stream_bytes(int32_t O, int32_t lanes, int32_t beam_width, int32_t max_frames, int32_t label_topk, size_t* bytes);
/* label_topk == 0: the unpruned search (O <= 64); else the pruned one, limits as tfk_ctc_beam_topk.  On the current device;
 * every lane empty, unbound, at 0 frames. */
int tfk_ctc_stream_create(int32_t O, int32_t lanes, int32_t beam_width, int32_t max_frames, int32_t label_topk,
                          tfk_ctc_stream** out);
int tfk_ctc_stream_destroy(tfk_ctc_stream* s); /* after the work enqueued on it is over */
/* lane (-1: every lane) back to an empty trie, 0 frames, unbound: two stream-ordered memsets */
int tfk_ctc_stream_reset(tfk_ctc_stream* s, void* stream, int32_t lane);
int tfk_ctc_stream_frames(tfk_ctc_stream* s, int32_t* frames /* host [lanes] */);
/* Tests / tools, and callers with their own logits: DEVICE logits [T, ld], chunk_len[lanes] HOST (>= 0, sum = T, lane l's rows
 * follow lane l - 1's).  Model as tfk_ctc_beam_lm_logits / tfk_ctc_beam_graph_logits take it (device tables, not validated):
 * lm_dev == NULL acoustic (the arguments after it are not read); next_dev == NULL the n-gram table of `order`; else the graph
 * lm_dev = weight, next_dev, num_states, start. */
int tfk_ctc_stream_push_logits(tfk_ctc_stream* s, void* stream, const float* logits, int64_t ld, int32_t T,
                               const int32_t* chunk_len, const float* lm_dev, int32_t order, const int32_t* next_dev,
                               int32_t num_states, int32_t start, float lm_weight, float label_bonus);
/* Evaluation-mode forward of X [T, ldx] (already SPLICED rows, host pointer, as tfk_ctc_beam takes X; T == 0: no forward) and
 * the same push on the engine's logits and stream; parameters, accumulators and statistics are untouched.  flags: 0 or
 * TFK_CTC_LM (the engine's model, table or graph, ranks with lm_weight / label_bonus; non-zero if none is set). */
int tfk_ctc_stream_push(tfk_engine* e, tfk_ctc_stream* s, const float* X, int64_t ldx, int32_t T, const int32_t* chunk_len,
                        float lm_weight, float label_bonus, int flags);
/* The N-best of every lane over the frames pushed so far.  HOST outputs; synchronises `stream`.  flags: 0 or TFK_CTC_LM_EOS.
 * hyp[(n * lanes + l) * hyp_cap + j], j < min(hyp_len, hyp_cap), the rest -1; hyp_len[n * lanes + l] is the TRUE length (it
 * may exceed hyp_cap: truncated); score / am_score [n * lanes + l] (am_score may be NULL; without a model it equals score). */
int tfk_ctc_stream_result(tfk_ctc_stream* s, void* stream, int32_t top_paths, int flags, int32_t* hyp, int32_t hyp_cap,
                          int32_t* hyp_len, float* score, float* am_score);

/* ---- data parallelism (one engine per rank; the host owns the collective) --------------------- */

/* The reduce region is one contiguous fp32 span of the state: [ G (all layers) | batch_loss,
 * num_frames, num_microbatches, pad | BN moving-average increments ].  A SUM all-reduce of it across
 * ranks before tfk_apply makes B/U serial micro-batches on one GPU (trainer.py:310-332) and
 * one micro-batch on each of B/U GPUs the same computation.  Buckets: b in [0, L] is the weight-gradient span of
 * layer L - b (the order backward produces them), L + 1 every bias / beta gradient, L + 2 the scalars + the BN
 * increments.  With TFK_LAST_MICROBATCH they are announced in the order L + 2 (right after the loss, before
 * backward), 0 .. L, L + 1 -- also during layer-wise growth, when the layers above the active depth have a zero
 * gradient (they are announced right after bucket 0). */
int tfk_reduce_region(tfk_engine* e, void** device_ptr, size_t* num_floats);
/* `init_grads` / `init_loss` / `init_num_frames` (trainer.py:350-352) done eagerly: writes zeros over the whole
 * reduce region.  tfk_apply re-initialises lazily (the next step's first micro-batch overwrites G), so a rank
 * that contributes NO micro-batch to a step must call this before the all-reduce. */
int tfk_zero_accumulators(tfk_engine* e);
int tfk_reduce_bucket(tfk_engine* e, int bucket, size_t* offset_floats, size_t* num_floats);
int tfk_num_buckets(tfk_engine* e, int* n);

/* Called on the host from tfk_accumulate(TFK_LAST_MICROBATCH) right after the kernels that finish a
 * bucket have been enqueued, so the host can launch that bucket's all-reduce behind them while the
 * remaining backward keeps the GPU busy. */
typedef void (*tfk_bucket_fn)(void* user, int bucket);
int tfk_set_bucket_callback(tfk_engine* e, tfk_bucket_fn fn, void* user);

/* tfk_apply in three parts, for a host that overlaps the optimiser with its collectives: tfk_apply_begin needs
 * bucket L + 2 reduced (learning rate, BN moving averages, loss hand-over); tfk_apply_span runs mean -> clip ->
 * Adam on the parameters [offset, offset + n) of the arena (same offsets as the reduce region), callable as soon as
 * THAT span of G is reduced; tfk_apply_end returns the average loss and re-initialises the accumulators.
 * tfk_apply == begin, span(0, P), end. */
int tfk_apply_begin(tfk_engine* e);
int tfk_apply_span(tfk_engine* e, size_t offset_floats, size_t num_floats);
int tfk_apply_end(tfk_engine* e, float* average_loss);

/* Called on the host right before the kernels that READ the parameters of hidden layer `layer` (0 .. L - 1), of the
 * output layer (L) or of every layer (-1: tensor get / set, the bf16 shadow rebuild) are enqueued.  A host that writes
 * parameters asynchronously -- the all-gather of the sharded exchange step, still in flight when the next step's
 * forward pass starts -- makes the engine stream wait for exactly that write here. */
typedef void (*tfk_layer_fn)(void* user, int layer);
int tfk_set_layer_callback(tfk_engine* e, tfk_layer_fn fn, void* user);

/* Sharded exchange step (reduce-scatter -> tfk_apply_span on this rank's share -> all-gather of the updated
 * parameters written straight into the arena by the collective): tells the engine that parameters changed behind
 * the optimiser's back, so the bf16 weight shadow of the mixed-precision mode is rebuilt before its next use.
 * Call between the last tfk_apply_span and tfk_apply_end (or at any other time). */
int tfk_params_touched(tfk_engine* e);

/* Mixed precision + sharded exchange: the bf16 shadow of the weight matrices.  When every weight matrix has a leading
 * dimension that is a multiple of 8, the shadow mirrors the fp32 parameter arena element for element (`mirrors_arena` = 1,
 * `num_elems` = the length of the weight part of the arena) and lives at the tail of the state arena (tfk_state_bytes
 * counts it), so the host can all-gather each rank's freshly updated shard of the SHADOW (tfk_apply_span writes it with
 * the update) instead of the fp32 parameters: half the bytes, and the next forward pass -- which reads only the shadow --
 * waits for it layer by layer through tfk_set_layer_callback.  The fp32 masters then stay valid only on the rank that
 * owns the span until the host gathers them (checkpoints, tensor get / set).  Otherwise num_elems = 0. */
int tfk_shadow_region(tfk_engine* e, void** device_ptr, size_t* num_elems, int* mirrors_arena);
/* (ABI 8) Emulated fp32 + sharded exchange: the tiled three-plane twin of weight matrix `layer` (0 .. L) -- what the
 * contractions read and what tfk_apply_span writes with the update.  Rows come in pairs (csrc/x3_layout.h), so rank r's rows
 * [r * rows / world, (r + 1) * rows / world) are the r-th of `world` equal, contiguous pieces of the region whenever rows is a
 * multiple of 2 * world: the exchange may then all-gather the owner-written PLANES of the matrix (6 B per weight) in place of
 * its fp32 parameters (4 B) + a local rebuild (tfk_twins_from_params); the fp32 masters of the matrix then stay valid on their
 * owner only, as with the bf16 shadow.  bytes = 0 when the arithmetic has no such twins or the optimiser does not write them.
 * tfk_param_checksum(e, 3, ..) sums every twin. */
int tfk_twin_region(tfk_engine* e, int layer, void** device_ptr, size_t* bytes, int* rows);
/* (ABI 7) The fp32 parameters [offset, offset + n) -- whole weight matrices -- were written behind the optimiser's back (a
 * sharded exchange all-gathered them) and what the contractions READ is derived from them: under TFK_DTYPE_F32X3 the tiled
 * three-plane twins (csrc/x3_layout.h).  Rebuilds the twins of those matrices on `stream` (NULL: the engine's) -- the exchange
 * calls it on the stream the gather ran on, right behind it, so that the rebuild of layer l hides under the forward pass of
 * the layers below instead of the whole set being rebuilt, all gathers awaited, in front of the next pass.  *current = 1: what
 * the contractions read is current for that span (exact fp32: always; emulated fp32: rebuilt); 0: nothing was done (mixed
 * precision without this path, or twins that were stale anyway) and the caller falls back to tfk_params_touched. */
int tfk_twins_from_params(tfk_engine* e, size_t offset, size_t n, void* stream, int* current);
/* Between tfk_apply_begin and tfk_apply_end: does tfk_apply_span write the bf16 shadow along with the parameters
 * (mixed precision, arena-mirroring shadow that was current when the step began)? */
int tfk_apply_writes_shadow(tfk_engine* e, int* direct);
/* Position-weighted 64-bit integer checksum of the fp32 parameter arena (which = 0), of the arena-mirroring bf16
 * shadow (which = 1) or of the fp32 bias / beta vectors alone (which = 2), taken in engine-stream order; synchronises.  Replicas of a data-parallel job compare it after
 * the first optimiser steps: a mis-ordered collective would otherwise train on stale weights silently. */
int tfk_param_checksum(tfk_engine* e, int which, uint64_t* value);

/* Number of micro-batches of this optimiser step that ranks AFTER this one process: weights this
 * rank's BN moving-average increment by bn_decay^later so the all-reduced result equals the
 * reference's sequential per-micro-batch EMA updates. */
int tfk_set_later_microbatches(tfk_engine* e, int32_t later);
/* The fp32 parameter arena [P] (same float offsets as the gradient part of the reduce region): what a sharded exchange
 * step all-gathers into. */
int tfk_param_region(tfk_engine* e, void** device_ptr, size_t* num_floats);
/* (ABI 8) Adam's first and second moments [P] each, same float offsets as the parameter arena.  Under a sharded exchange every
 * rank updates the moments of its OWN shards only -- the optimiser state is sharded with the optimiser -- so whatever changes
 * the assignment of shards to ranks (tfk_comm_set_bucket_bytes, tfk_comm_set_gather) gathers them first. */
int tfk_moment_regions(tfk_engine* e, void** adam_m, void** adam_v, size_t* num_floats);

/* ---- the exchange step inside the library: RCCL over xGMI, no host language in the step ------------------------
 *
 * Replaces, for N > 1 GPUs, what a single reference process does between `update_gradients_op` and
 * `apply_gradients_op` (trainer.py:165-184): the micro-batches of a step run on different GPUs, so G, batch_loss,
 * num_frames and the BN moving-average increments are SUMMED over the ranks before mean -> clip -> Adam.  A tfk_comm
 * attaches to one engine, installs itself behind the engine's bucket / layer hooks (tfk_set_bucket_callback /
 * tfk_set_layer_callback: do not set your own while one is attached) and from then on
 *     tfk_accumulate*(..., TFK_LAST_MICROBATCH)  launches the collectives while backward is still being enqueued,
 *     tfk_comm_apply                             replaces tfk_apply          (Adam per reduced span, parameter gathers),
 *     tfk_comm_eval_finish                       replaces tfk_eval_finish    (scalar tail summed over the ranks),
 *     tfk_comm_idle                              a rank without a micro-batch in this step contributes zeros.
 * Every rank makes the same calls in the same order.  Exchange modes as tfkaldi_amd/dataparallel.py (which drives the
 * same protocol through torch.distributed for backends without RCCL):
 *   TFK_EXCHANGE_SHARDED    in-place reduce-scatter of every coalesced span of weight gradients, Adam on this rank's
 *                           1/world of it, in-place all-gather of the updated parameters -- in mixed precision of the
 *                           bf16 shadow (2 B per parameter; the fp32 masters of a span then live on its owner until
 *                           tfk_comm_gather_masters) -- consumed layer by layer by the next forward pass;
 *   TFK_EXCHANGE_ALLREDUCE  SUM all-reduce of every span, full Adam on every rank.
 * Streams: collectives launched while backward still runs, and the parameter gathers the next forward pass consumes layer
 * by layer, go to a comm stream the tfk_comm owns (ordered against the engine stream by events); the collectives launched
 * behind the LAST backward kernel and the gather the next forward pass reads first go to the engine stream itself
 * (nothing is left to overlap with, and a round trip through another stream costs ~26 us; env TFK_DP_INLINE_TAIL=0:
 * everything on the comm stream).  RCCL orders the operations of one communicator itself.
 * bucket_bytes: adjacent gradient buckets are coalesced until a collective carries at least this much (0: default,
 * 32 MiB -- each collective under backward costs the step a fixed 6-10 us, but the next forward pass cannot start a layer before
 * the whole gather covering it has arrived and the span still coalescing when backward ends is exposed: csrc/exchange.hip).
 * Bootstrap: EVERY rank first calls tfk_comm_available (local, no collective: RCCL loadable, engine and mode acceptable) and
 * the host agrees on the answers (one MIN all-reduce over whatever process group it already has) -- tfk_comm_create is
 * collective (ncclCommInitRank), so a rank that could not even load RCCL must be known BEFORE the others enter it and
 * block.  Then rank 0 calls tfk_comm_unique_id, the host distributes the bytes any way it likes (torch.distributed, MPI, a
 * file), and every rank calls tfk_comm_create with them. */
enum { TFK_EXCHANGE_SHARDED = 0, TFK_EXCHANGE_ALLREDUCE = 1 };
typedef struct tfk_comm tfk_comm;
int tfk_comm_available(tfk_engine* e, int mode);
int tfk_comm_unique_id(void* id, size_t capacity, size_t* size);  /* 128 bytes */
int tfk_comm_create(tfk_engine* e, const void* id, size_t id_size, int rank, int world, int mode, size_t bucket_bytes,
                    tfk_comm** out);
int tfk_comm_destroy(tfk_comm* c);  /* before tfk_destroy of its engine */
int tfk_comm_info(tfk_comm* c, int* rank, int* world, int* mode, int* gathers_shadow);
const char* tfk_comm_backend(tfk_comm* c);  /* "rccl" | "loopback" */
int tfk_comm_apply(tfk_comm* c, float* average_loss);
/* the same in two halves (as tfk_apply_enqueue / tfk_apply_end): _enqueue launches the tail collectives, Adam on this rank's
 * spans and the parameter gathers; _end waits for the loss (and runs the replica check of the first sharded steps). */
int tfk_comm_apply_enqueue(tfk_comm* c);
int tfk_comm_apply_end(tfk_comm* c, float* average_loss);
int tfk_comm_eval_finish(tfk_comm* c, float* average_loss);
/* (tests / diagnostics) launch what is still coalescing and make the engine stream wait for every collective of the step,
 * WITHOUT the optimiser: the reduce region then holds the summed gradients -- of a reduce-scattered span only this rank's
 * 1/world.  tfk_comm_apply may follow. */
int tfk_comm_finish_reduce(tfk_comm* c);
int tfk_comm_idle(tfk_comm* c);
/* make the engine stream wait for parameter gathers still in flight (before the state is read behind the engine's back) */
int tfk_comm_drain(tfk_comm* c);
/* mixed-precision sharded exchange: are the fp32 masters currently valid on their owners only? / COLLECTIVE: bring them
 * home (all-gather of every sharded span) before a checkpoint or a tensor get / set */
int tfk_comm_masters_stale(tfk_comm* c, int* stale);
int tfk_comm_gather_masters(tfk_comm* c);
/* collectives of the last completed step: counts by kind and, in launch order, the gradient spans as triples
 * (offset in floats, floats, 1 = reduce-scattered / 0 = all-reduced); spans holds 3 * capacity values */
int tfk_comm_last_step(tfk_comm* c, int* reduce_scatters, int* all_gathers, int* all_reduces, size_t* spans, int capacity,
                       int* num_spans);
/* (ABI 8) HOW a reduce-scattered span and a parameter gather travel (sharded mode; reference seam trainer.py:165-184 -- the sum
 * `G += g` over the micro-batches of a step, here over ranks):
 *   TFK_ALGO_RCCL    ncclReduceScatter / ncclAllGather: RCCL picks the algorithm (ring / tree over its channels) and with it the
 *                    order the ranks' contributions are added in;
 *   TFK_ALGO_DIRECT  the collective spelled out for a full mesh of point-to-point xGMI links: one grouped ncclSend / ncclRecv
 *                    per peer -- sub-span q of every rank goes straight to rank q over the link between them, all world - 1
 *                    links busy at once -- and the OWNER adds the world contributions in fp32 in RANK ORDER, i.e. in the order a
 *                    single process adds its micro-batches: the reduced shard equals the serial run's G bit for bit.  The
 *                    gather is the same movement backwards (own shard to every peer, in place).
 * Wire format of the reduce-scatter: TFK_WIRE_FP32, or TFK_WIRE_BF16 (direct movement at half the bytes; the owner's own
 * contribution stays exact).  Environment at attach: TFK_DP_ALGO = rccl (default) | direct | auto, TFK_DP_WIRE = fp32 | bf16.
 * `auto` (more than one RCCL rank): tfk_comm_create times both algorithms on scratch memory of a span's size (tfk_comm_tune,
 * collective) and keeps the faster one per operation -- the slowest rank's time decides, identically on every rank.  It is
 * opt-in until a multi-GPU node has run it: bench.py --gpus N runs the same tuning pass and an algorithm x wire A/B BEHIND its
 * timed region and reports both, so the first scaling line shows what `auto` would have chosen and gained.
 * tfk_comm_set_exchange (-1 = keep): between steps only, every rank with the same arguments.
 * tfk_comm_get_exchange: what is in force; chosen_by 0 default / 1 environment / 2 tuned / 3 set; tune_us[4] = microseconds of
 * reduce-scatter rccl, direct, all-gather rccl, direct as tuned (0: never tuned). */
enum { TFK_ALGO_RCCL = 0, TFK_ALGO_DIRECT = 1 };
enum { TFK_WIRE_FP32 = 0, TFK_WIRE_BF16 = 1 };
int tfk_comm_set_exchange(tfk_comm* c, int algo, int wire);
int tfk_comm_get_exchange(tfk_comm* c, int* algo_reduce_scatter, int* algo_all_gather, int* wire, int* chosen_by, double* tune_us);
int tfk_comm_tune(tfk_comm* c, size_t floats, int iters); /* COLLECTIVE */
/* (ABI 8) WHAT is gathered under the emulated fp32 arithmetic (sharded mode).  Default (`params`): the fp32 parameters of every
 * span, and every rank rebuilds the three-plane twins of what it received (tfk_twins_from_params behind each gather).  `planes`
 * (env TFK_DP_GATHER=planes at attach, or this call -- COLLECTIVE, between steps): the sharding unit becomes the weight matrix --
 * rank r owns rows [r R / world, (r + 1) R / world) of every matrix of a span, the span's collectives are launched as one group
 * -- and for every matrix whose rows divide by 2 * world the twin rows the owner's Adam wrote are gathered (tfk_twin_region: 6 B
 * per weight on the wire, nothing rebuilt); the fp32 masters of those matrices stay with their owners until
 * tfk_comm_gather_masters (tfk_comm_masters_stale says so; tfk_comm_info: gathers_shadow = 2).  Switching back gathers them.
 * dataparallel.exchange_model prices both; bench.py --gpus N measures both (`exchange_ab`). */
int tfk_comm_set_gather(tfk_comm* c, int planes);
/* (ABI 8) the coalescing threshold of tfk_comm_create's `bucket_bytes`, changed between steps (every rank alike; 0 = the 32 MiB
 * default): how many weight matrices one collective carries is the first thing to tune on real links -- bench.py sweeps it.
 * COLLECTIVE: another span cut assigns shards to other ranks, so masters left with their owners are gathered first. */
int tfk_comm_set_bucket_bytes(tfk_comm* c, size_t bucket_bytes);
/* (ABI 8) Device time per phase of the exchange step, for diagnosis (bench.py --gpus N: `exchange_phases`): between
 * tfk_comm_timing(c, 1) and tfk_comm_timing_read every phase is bracketed by timing events on the stream it runs on (each
 * record costs that stream a few microseconds: a diagnostic pass, not the one a rate is quoted from).  ms_per_step[k], averaged
 * over the steps completed in between: 0 reduce-scatters (pack / exchange / owner's sum included), 1 all-reduces (vectors, scalar
 * tail), 2 engine-stream time from the last backward kernel to the first optimiser kernel (what the exchange leaves exposed in
 * front of Adam), 3 Adam on this rank's spans, 4 parameter gathers, 5 three-plane twin rebuilds behind them, 6 engine-stream
 * time the next forward pass spends waiting for gathers (the first span's gather + rebuild run on that stream and count in
 * full).  tfk_comm_timing_read synchronises both streams and switches the timing off. */
int tfk_comm_timing(tfk_comm* c, int on);
int tfk_comm_timing_read(tfk_comm* c, double* ms_per_step, int capacity, long* steps);
/* Tests: a group of `world` engines of ONE process on ONE device; each rank is driven by its own host thread and the
 * collectives are a rendezvous + plain kernels.  This is how the protocol above runs at world 2 / 4 / 8 on a single-GPU
 * box (RCCL refuses two ranks on one device). */
typedef struct tfk_loopback tfk_loopback;
int tfk_loopback_create(int world, tfk_loopback** out);
int tfk_loopback_destroy(tfk_loopback* group);
int tfk_comm_create_loopback(tfk_engine* e, tfk_loopback* group, int rank, int mode, size_t bucket_bytes, tfk_comm** out);

/* ---- streams, profiling, debugging ------------------------------------------------------------- */

int tfk_synchronize(tfk_engine* e);
int tfk_stream(tfk_engine* e, void** hip_stream);

typedef struct tfk_kernel_stat {
  char name[48];
  int64_t launches;
  double total_ms;  /* HIP-event time on the engine stream */
  double flops;     /* algorithmic FLOPs of those launches */
  double bytes;     /* algorithmic bytes of those launches */
} tfk_kernel_stat;
/* Bracket every kernel launch with HIP events (on the engine stream) until tfk_profile_end. */
int tfk_profile_begin(tfk_engine* e);
int tfk_profile_end(tfk_engine* e, tfk_kernel_stat* stats, int capacity, int* count);

enum { /* debug tensors of the LAST accumulate / eval / posteriors call */
  TFK_DBG_LOGITS = 0,      /* [T, O] logits; after tfk_accumulate: dLogits = softmax - onehot */
  TFK_DBG_HIDDEN = 1,      /* [T, H] output of hidden layer `layer` */
  TFK_DBG_DROPOUT_MASK = 2,/* [T, H] 0/1 keep mask of hidden layer `layer` (regenerated) */
  TFK_DBG_PREACT = 3,      /* [T, H] affine output z of hidden layer `layer` (what batch norm normalises) */
  TFK_DBG_BN_MEAN = 4,     /* row 0 of [T, H]: batch mean of z's columns as the backward pass reads it (training calls) */
  TFK_DBG_BN_RSTD = 5,     /* row 0 of [T, H]: 1 / sqrt(batch variance + eps) */
  TFK_DBG_DPREACT = 6,     /* [T, H] dz of hidden layer `layer`, the gradient with respect to its affine output, as hidden_backward
                            * leaves it.  Mixed precision stores dz as its bf16 twin ALONE (rounded from the kernel's registers;
                            * both contractions that consume dz read the twin), so these are the twin's values, widened.  Kept only
                            * under tfk_debug_capture; without it the call fails by name. */
  TFK_DBG_TRAIN_LOGITS = 7 /* [T, O] the logits of a training call, which the loss then overwrites with dLogits in place; under
                            * tfk_debug_capture only (one more device-to-device copy, behind the forward pass) */
};
int tfk_debug_fetch(tfk_engine* e, int what, int layer, float* host, size_t count);

/* ABI 18: the bf16 operand twins as the contractions read them (tests and tools; TFK_DTYPE_BF16 only -- TFK_DTYPE_F32 keeps no
 * twins, and the three-plane twins of TFK_DTYPE_F32X3 are refused by name).  `host` receives the raw bfloat16 bit patterns,
 * unpadded (the twins' padding columns are not part of the fetch); `count` = rows x columns.  The call waits for everything the
 * engine has in flight.
 *   TFK_TWIN_INPUT    [T, F]  the twin of the input slot the last call read
 *   TFK_TWIN_HIDDEN   [T, H]  the twin of the output of hidden layer `layer` (evaluated by the last call)
 *   TFK_TWIN_DLOGITS  [T, O]  the twin of d loss / d logits; after a training call only
 *   TFK_TWIN_WEIGHTS  [d_in, d_out] the shadow of the weight matrix of layer `layer` (0 .. L).  Refused while the shadow is not
 *                     current (parameters written from outside, or an optimiser step that does not write it): the next pass
 *                     rebuilds it.
 *   TFK_TWIN_DPREACT  [T, H]  the twin of dz of hidden layer `layer`; under tfk_debug_capture only */
enum { TFK_TWIN_INPUT = 0, TFK_TWIN_HIDDEN = 1, TFK_TWIN_DLOGITS = 2, TFK_TWIN_WEIGHTS = 3, TFK_TWIN_DPREACT = 4 };
int tfk_debug_fetch_twin(tfk_engine* e, int what, int layer, uint16_t* host, size_t count);
/* The backward pass keeps dz only in its two ping-pong twin buffers.  on != 0: every later NON-STACKED training pass enqueues
 * device-to-device copies on the engine stream -- one behind the forward pass (the logits, which the loss overwrites in place:
 * TFK_DBG_TRAIN_LOGITS) and one right behind each hidden layer's hidden_backward (the bf16 twin of dz, the only form in which
 * mixed precision stores it: TFK_DBG_DPREACT / TFK_TWIN_DPREACT) -- into buffers allocated with the activations and released by
 * tfk_destroy or by on == 0.  A stacked pass captures nothing.  TFK_DTYPE_BF16 only: TFK_DTYPE_F32X3 is refused by name (its
 * fused dual launch never stores du or dz in fp32).  With capture off (the default) a pass enqueues exactly what it did
 * before ABI 18. */
int tfk_debug_capture(tfk_engine* e, int on);

/* Stand-alone fp32 GEMM on device pointers (tests / tools): layout 0 NN, 1 NT, 2 TN (gemm_f32.h). */
int tfk_gemm_f32(void* stream, int layout, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                 int M, int N, int K, const float* bias, int epi, int tile_config);
/* Stand-alone bf16 GEMM (fp32 accumulate / result) on device pointers: A, B hold bfloat16 bit patterns with
 * leading dimensions (in elements) that are multiples of 8 and zero padding (gemm_bf16.h). */
int tfk_gemm_bf16(void* stream, int layout, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc,
                  int M, int N, int K, const float* bias, int epi);
/* Stand-alone fp32-emulating GEMM (TFK_DTYPE_F32X3's contraction; gemm_bf16.h: gemm_bf16x3) on device pointers: A and B are given
 * as three bf16 planes each in the TILED layout of csrc/x3_layout.h (ld a multiple of 32; 2-row x 32-column units of three 128-byte
 * lines, one per plane: element (r, c) of plane q at ((r / 2) * (ld / 32) + c / 32) * 192 + 64 q + 32 (r % 2) + c % 32;
 * ceil(rows / 2) * (ld / 32) * 192 elements in all); tfk_split3 makes such a twin from an fp32 matrix [rows, lds]:
 * src == plane 0 + plane 1 + plane 2 exactly, padding columns zero.  tfk_gemm_bf16x3_dual: the backward pair of a layer in one
 * launch (as tfk_gemm_bf16_dual).  Tests and tools.  (ABI 7: the separate-plane form of ABI 6 -- `a_plane` / `b_plane`
 * arguments -- is gone.) */
int tfk_split3(void* stream, const float* src, int lds, uint16_t* dst, int ldd, int rows, int cols);
/* tests: mark a ticket of the engine's split-K workspace as taken, as an interrupted launch would leave it.  The next step whose
 * contractions split their K must then FAIL (tfk_apply / tfk_eval_finish / tfk_posteriors return non-zero, tfk_last_error names
 * the timeout) -- a block that waits ~1 s for its partner's partial sums reports it through mapped memory -- and the step after
 * that must work again. */
int tfk_debug_poison_splitk(tfk_engine* e);
int tfk_gemm_bf16x3(void* stream, int layout, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc, int M,
                    int N, int K, const float* bias, int epi);
int tfk_gemm_bf16x3_dual(void* stream, const uint16_t* A_nt, int lda_nt, const uint16_t* B_nt, int ldb_nt, float* C_nt,
                         int ldc_nt, int M_nt, int N_nt, int K_nt, const uint16_t* A_tn, int lda_tn, const uint16_t* B_tn,
                         int ldb_tn, float* C_tn, int ldc_tn, int M_tn, int N_tn, int K_tn, int epi_tn);
/* The backward pair of one layer in ONE launch (gemm_bf16.h: gemm_bf16_dual): C_nt[M_nt, N_nt] = A_nt . B_nt^T and
 * C_tn[M_tn, N_tn] (+)= A_tn^T . B_tn (epi_tn: 0 or 2 = accumulate).  Fails when the pair of shapes is not eligible
 * (tfk_gemm_bf16_dual_config == 0).  Block geometry: env TFK_BF16_DUAL_CFG (3: 128x64, 4: 128x128, 5: 256x128,
 * 8: 256x128 for the NT half + 256x256 for the TN half, 0: off). */
int tfk_gemm_bf16_dual(void* stream, const uint16_t* A_nt, int lda_nt, const uint16_t* B_nt, int ldb_nt, float* C_nt,
                       int ldc_nt, int M_nt, int N_nt, int K_nt, const uint16_t* A_tn, int lda_tn, const uint16_t* B_tn,
                       int ldb_tn, float* C_tn, int ldc_tn, int M_tn, int N_tn, int K_tn, int epi_tn);
int tfk_gemm_bf16_dual_config(int M_nt, int N_nt, int M_tn, int N_tn);
/* Tile configuration of the bf16 GEMM (gemm_bf16.h: 0-2 register-staged, 3-8 LDS-DMA staged): force one for every
 * later call (cfg < 0 restores the heuristic) / ask which one the heuristic gives an [M, N] result.  Tools and
 * tests only. */
int tfk_gemm_bf16_force_config(int cfg);
int tfk_gemm_bf16_config(int M, int N);

/* ---- feature computation: wav samples -> fbank / mfcc / ssc (+ deltas), CMVN statistics ------------ */
/*
 * The step in FRONT of the feature reader: processing/feat.py:7-69 (FeatureComputer),
 * processing/base.py:39-284 (mfcc, fbank, logfbank, ssc, lifter, deriv, delta, ddelta), processing/sigproc.py:33-191
 * (preemphasis, framesig, magspec, powspec) and processing/prepare_data.py:80-118 (compute_cmvn), computed in
 * float64 as the reference does (numpy's default), for a whole BATCH of utterances per call.
 *
 * All pointers of the compute calls are DEVICE pointers; work is ordered on `stream` (a hipStream_t; NULL = the
 * default stream).  A plan may be used from one thread at a time.
 *
 * Signals of the batch are concatenated: utterance u owns samples [sig_off[u], sig_off[u+1]) and frames
 * [frame_off[u], frame_off[u+1]) -- the caller counts frames as sigproc.py:49-55 does (1 if len <= frame_len, else
 * 1 + ceil((len - frame_len) / frame_step)) -- and frame t of an utterance covers its samples
 * [t*frame_step, t*frame_step + frame_len), zero-padded past the end of the utterance (sigproc.py:57-66), after the
 * pre-emphasis y[0] = x[0], y[i] = x[i] - preemph * x[i-1] (sigproc.py:180-191).  Frames longer than nfft are
 * truncated and shorter ones zero-padded by the transform (numpy.fft.rfft(frames, nfft): sigproc.py:138).
 */
typedef struct tfk_feat tfk_feat;

enum { TFK_FEAT_FBANK = 0, TFK_FEAT_MFCC = 1, TFK_FEAT_SSC = 2,        /* feat.py:21-28: log-fbank, mfcc, ssc */
       TFK_FEAT_FBANK_RAW = 3 };  /* base.fbank (base.py:59-98): filterbank energies and frame energy WITHOUT the log */
enum { TFK_DYN_NODELTA = 0, TFK_DYN_DELTA = 1, TFK_DYN_DDELTA = 2 };   /* feat.py:30-37 */
enum { TFK_SAMPLE_I16 = 0, TFK_SAMPLE_F64 = 1,  /* scipy.io.wavfile's int16 / any other integer type promoted to float64 */
       TFK_SAMPLE_F32 = 2 };  /* float32 wav files: numpy keeps `signal[1:] - coeff * signal[:-1]` in float32 for them (the Python
                               * float is cast down), so the pre-emphasis is done in float32 and only then widened */
enum { TFK_STAGE_FRAMES = 1, TFK_STAGE_MAGSPEC = 2, TFK_STAGE_POWSPEC = 3 };

typedef struct tfk_feat_config {
  int32_t struct_size;     /* sizeof(tfk_feat_config) */
  int32_t device;          /* HIP device ordinal */
  int32_t kind;            /* TFK_FEAT_* */
  int32_t dynamic;         /* TFK_DYN_* */
  int32_t frame_len;       /* samples per frame:  round(winlen * rate)  (sigproc.py:50) */
  int32_t frame_step;      /* samples per step:   round(winstep * rate) (sigproc.py:51) */
  int32_t nfft;            /* transform length: a power of two in [32, 4096] */
  int32_t nfilt;           /* mel filters (<= nfft / 2) */
  int32_t numcep;          /* TFK_FEAT_MFCC: cepstra kept (<= nfilt) */
  int32_t include_energy;  /* append log(frame energy) as the last static column (feat.py:61-62) */
  double preemph;          /* pre-emphasis coefficient */
} tfk_feat_config;

/* Tables are HOST pointers, copied: filterbank[nfilt][nfft/2+1] (base.get_filterbanks), bin_weight[nfft/2+1]
 * (TFK_FEAT_SSC: numpy.linspace(1, rate/2, nfft/2+1), base.py:151), dct[nfilt][numcep] and lifter[numcep]
 * (TFK_FEAT_MFCC: the orthonormal DCT-II matrix and the lifter weights, base.py:55-56,226-246). */
int tfk_feat_create(const tfk_feat_config* cfg, const double* filterbank, const double* bin_weight, const double* dct,
                    const double* lifter, tfk_feat** out);
int tfk_feat_destroy(tfk_feat* f);
/* columns of the feature matrix: (nfilt or numcep, + 1 with the energy) * (1, 2 or 3) */
int tfk_feat_dim(const tfk_feat* f, int32_t* dim);
/* FeatureComputer.__call__ (feat.py:42-69) for a batch: out[n_frames][ld_out] as float32 (what ArkWriter stores,
 * ark.py:202) or float64 (what the reference's functions return). */
int tfk_feat_compute(tfk_feat* f, void* stream, const void* signal, int sample_type, const int64_t* sig_off,
                     const int64_t* frame_off, int32_t n_utts, int64_t n_frames, void* out, int64_t ld_out, int out_f64);
/* Intermediate results of the same pipeline as float64: TFK_STAGE_FRAMES [n_frames][frame_len] (sigproc.framesig of
 * the pre-emphasised signal), TFK_STAGE_MAGSPEC / TFK_STAGE_POWSPEC [n_frames][nfft/2+1] (sigproc.py:125-153). */
int tfk_feat_stage(tfk_feat* f, void* stream, int stage, const void* signal, int sample_type, const int64_t* sig_off,
                   const int64_t* frame_off, int32_t n_utts, int64_t n_frames, double* out, int64_t ld_out);
/* base.deriv / delta / ddelta (base.py:248-284) on a float64 matrix x[n_rows][ld_x] of `dim` columns whose rows
 * [row_off[u], row_off[u+1]) are one utterance each (scipy.ndimage.convolve1d's 'reflect' boundary applies per
 * utterance): out[n_rows][ld_out] = [x | d x | d d x] limited to 1 + dynamic blocks.  deriv_only: out = d x. */
int tfk_feat_dynamic(void* stream, const double* x, int64_t ld_x, int32_t dim, const int64_t* row_off, int32_t n_utts,
                     int64_t n_rows, int dynamic, int deriv_only, void* out, int64_t ld_out, int out_f64);
/* sigproc.deframesig (sigproc.py:69-123): overlap-add of frames[n_frames][ld] (frame_len columns used) back into a signal
 * of (n_frames - 1) * frame_step + frame_len samples; every sample is divided by the sum of the window values (+ 1e-15 per
 * frame, as there) of the frames that cover it, both sums taken in frame order.  win[frame_len] = NULL: rectangular. */
int tfk_deframesig(void* stream, const double* frames, int64_t ld, int64_t n_frames, int32_t frame_len, int32_t frame_step,
                   const double* win, double* out);
/* The tail of sigproc.logpowspec (sigproc.py:170-178), in place on n power-spectrum values: 10 log10(max(p, 1e-30)),
 * minus the maximum over all of them when norm != 0.  scratch: device memory for 1024 doubles. */
int tfk_logpow(void* stream, double* p, int64_t n, int norm, double* scratch);
/* compute_cmvn (prepare_data.py:80-118): speaker s owns the utterances [spk_off[s], spk_off[s+1]) of the list
 * (utt_row[q], utt_len[q]) = first row and row count in feats[.][ld] (float32, `dim` columns);
 * stats[s] = [[sum x | count], [sum x^2 | 0]] as [2][dim+1] doubles, the sums accumulated row after row in float32
 * exactly as numpy reduces the reference's float32 matrix. */
int tfk_cmvn_stats(void* stream, const float* feats, int64_t ld, int32_t dim, const int64_t* spk_off,
                   const int64_t* utt_row, const int64_t* utt_len, int32_t n_spk, double* stats);

#ifdef __cplusplus
}
#endif
#endif /* TFKALDI_HIP_H */
