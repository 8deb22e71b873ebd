"""Training environment with the reference's interface (neuralNetworks/trainer.py): Trainer,
CrossEnthropyTrainer, CTCTrainer.

The reference builds a TensorFlow graph (trainer.py:37-215) and drives it with session runs; here the
"graph + session" is one HIP engine (include/tfkaldi_hip.h).  What each reference fetch became:

    update_gradients_op.run(feed_dict)          -> engine.accumulate(X, y)      per micro-batch
    [average_loss, apply_gradients_op] + re-init -> engine.apply()
    update_valid_loss.run / average_loss.eval()  -> engine.eval_accumulate / eval_finish
    modelsaver / saver                           -> ModelSaver (.npz) / <prefix>_trainvars (.npz)

The host never pads: the reference zero-pads every utterance to max_input_length in float64 and the graph
immediately strips the padding again (trainer.py:298-307, seq_convertors.py:12-39); the engine takes the
flat utterance-major [T, F] matrix that seq2nonseq would have produced.
"""
import json
import os
from abc import ABCMeta, abstractmethod

import numpy as np

from .. import _lib
from ..dataparallel import (CtcMicroBatch, CtcMmiMicroBatch, CtcMwerMicroBatch, CtcWildMicroBatch, DataParallel,
                            RawMicroBatch, StackedRawMicroBatches, _beam_settings, local_device, partition, rank_seed)
from ..engine import _finite_nonneg
from ..processing.feature_reader import Unspliced, cmvn_table
from .classifiers.dnn import ModelSaver


def _spliced(utt):
    """host matrix [N, F] of one utterance (an Unspliced one is spliced on the host when it shares a
    micro-batch with already-spliced utterances)"""
    if isinstance(utt, Unspliced):
        return utt.spliced()
    return np.asarray(utt, dtype=np.float32)


class _Graph(object):
    """placeholder for the `.graph` attribute (reference callers pass it to tf.Session, nnet.py:134)"""

    def finalize(self):
        pass


class _StepVariable(object):
    """`.global_step` with the .eval() of a tf Variable (trainer.py:98-100, 342)"""

    def __init__(self, engine):
        self._engine = engine

    def eval(self, session=None):
        return self._engine.global_step


def microbatch_indices(num_utt, per_minibatch):
    """Utterance indices of the micro-batches the reference feeds (trainer.py:280-332).  It appends
    `num_utt % U` zero-length dummy utterances (sic -- not U - num_utt % U) and runs floor(len / U)
    micro-batches, so with num_utt % U != 0 the tail can be truncated; the dummies contribute nothing."""
    U = per_minibatch
    total = num_utt + (num_utt % U)
    return [[i for i in range(k * U, (k + 1) * U) if i < num_utt] for k in range(total // U)]


class MicrobatchSelector(object):
    """Which utterances of a batch does data-parallel rank `rank` need?  The selector the trainer hands to
    BatchDispenser.next_packed: the batch is cut into the reference's micro-batches (microbatch_indices), the
    micro-batches are dealt to the ranks in contiguous blocks (dataparallel.partition: rank order = the reference's
    serial order) and only this rank's come back -- the dispenser never reads the other ranks' frames."""

    def __init__(self, per_minibatch, rank=0, world=1):
        self.per_minibatch, self.rank, self.world = int(per_minibatch), int(rank), int(world)

    def __call__(self, frames):
        """frames: frame count of every usable utterance of the batch, in order -> (this rank's micro-batches as
        lists of positions, (micro-batches in the whole step, this rank's first, this rank's end))"""
        plan = microbatch_indices(len(frames), self.per_minibatch)
        if sum(len(idx) for idx in plan) < len(frames):
            Trainer._warn_truncation(len(frames), self.per_minibatch, sum(len(idx) for idx in plan))
        groups = [idx for idx in plan if idx and any(frames[i] for i in idx)]
        start, end = partition(len(groups), self.world)[self.rank]
        return groups[start:end], (len(groups), start, end)


class Trainer(object, metaclass=ABCMeta):
    """General class for the training environment of a neural-net classifier"""

    def __init__(self, classifier, input_dim, max_input_length, max_target_length, init_learning_rate,
                 learning_rate_decay, num_steps, numutterances_per_minibatch, seed=None, device=None):
        """
        Args (as reference trainer.py:13-31):
            classifier: the neural net classifier that will be trained
            input_dim: the input dimension to the nnnetgraph
            max_input_length: the maximal length of the input sequences
            max_target_length: the maximal length of the target sequences
            init_learning_rate: the initial learning rate
            learning_rate_decay: the parameter for exponential learning rate decay
            num_steps: the total number of steps that will be taken
            numutterances_per_minibatch: how many utterances are processed at a time
        Extra (optional): seed for weight initialisation / dropout, HIP device ordinal
        """
        self.numutterances_per_minibatch = numutterances_per_minibatch
        self.max_input_length = max_input_length
        self.max_target_length = max_target_length
        self.classifier = classifier
        self.input_dim = input_dim
        self._seed = seed if seed is not None else int.from_bytes(os.urandom(4), "little")
        self.dp = DataParallel()
        if self.dp.enabled:
            # every rank adopts rank 0's seed BEFORE the engine is built: the per-rank dropout keys are derived from it
            # (rank_seed), so a multi-rank run is reproducible from the one logged seed (round-2 advisor finding: ranks
            # > 0 keyed their dropout from a private os.urandom value that nothing recorded)
            import torch
            import torch.distributed as dist
            seed_t = torch.tensor([self._seed], dtype=torch.int64)
            if dist.get_backend(self.dp.group) == "nccl":
                seed_t = seed_t.cuda(device if device is not None else local_device())
            dist.broadcast(seed_t, src=0, group=self.dp.group)
            self._seed = int(seed_t.item())
        if device is None:
            device = local_device() if self.dp.enabled else 0
        self.graph = _Graph()
        # the loss is part of the graph: abstract in the base class (trainer.py:219-242)
        self.loss_kind = self.compute_loss(None, None, None, None)
        if self.loss_kind not in ("cross_enthropy", "ctc"):
            raise NotImplementedError("the HIP engine implements the cross-enthropy and CTC losses")
        max_frames = max(1, int(numutterances_per_minibatch)) * max(1, int(max_input_length))
        self.engine = classifier.create_engine(
            input_dim, torch_state=self.dp.enabled, init_learning_rate=init_learning_rate,
            learning_rate_decay=learning_rate_decay, num_steps=num_steps, max_frames=min(max_frames, 1 << 16),
            seed=rank_seed(self._seed, self.dp.rank), device=device)  # per-rank dropout stream from the SHARED seed
        self.modelsaver = ModelSaver(self.engine)
        self.control_ops = classifier.control_ops(self.engine)
        self.global_step = _StepVariable(self.engine)
        self.summarywriter = None
        self.graph.finalize()

    @abstractmethod
    def compute_loss(self, targets, logits, logit_seq_length, target_seq_length):
        """the loss of the training graph; subclasses name the loss the engine runs"""
        raise NotImplementedError("Abstract method")

    def initialize(self):
        """Initialize all the variables (reference trainer.py:244-247): random hidden weights, zero output
        layer, step counters, Adam state.  Every data-parallel rank draws the same weights."""
        self.dp.gather_parameters(self.engine)
        self.classifier.initialize(self.engine, np.random.default_rng(self._seed))
        for l in range(self.engine.L + 1):
            for kind in (_lib.WEIGHTS, _lib.BIASES) + ((_lib.BN_BETA,) if self.engine.batch_norm and l < self.engine.L else ()):
                zeros = np.zeros(self.engine._shape(kind, l), dtype=np.float32)
                for slot in (_lib.SLOT_GRAD, _lib.SLOT_ADAM_M, _lib.SLOT_ADAM_V):
                    self.engine.set(kind, l, zeros, slot)
        self.engine.set_scalar(_lib.GLOBAL_STEP, 0)
        self.engine.set_scalar(_lib.LEARNING_RATE_FACT, 1.0)
        self.engine.set_scalar(_lib.ADAM_STEPS, 0)

    def start_visualization(self, logdir):
        """open a summary log (the reference writes TensorBoard events: trainer.py:249-258); one JSON line
        per update with step, loss and learning rate is appended to <logdir>/summaries.jsonl"""
        os.makedirs(logdir, exist_ok=True)
        self.summarywriter = open(os.path.join(logdir, "summaries.jsonl"), "a")

    # ---- batching ----
    _warned_truncation = False

    @staticmethod
    def _warn_truncation(num_utt, per_minibatch, used):
        # the reference's padding arithmetic (trainer.py:280-294) silently drops the tail of a batch whose size
        # is not a multiple of numutterances_per_minibatch; kept for parity, but said once
        if not Trainer._warned_truncation:
            print("WARNING batch of %d utterances with numutterances_per_minibatch = %d: the last %d utterance(s) of "
                  "every such batch are not used (reference behaviour: trainer.py:280-294)"
                  % (num_utt, per_minibatch, num_utt - used))
            Trainer._warned_truncation = True

    def _groups(self, inputs, targets):
        """(utterance indices, micro-batch) of every micro-batch the batch yields: a group without frames yields none.  A
        generator: the truncation warning and the per-group checks of frames against targets run as it is consumed, so
        consume it to its end before the first micro-batch reaches the engine (as _microbatches does)"""
        plan = microbatch_indices(len(inputs), self.numutterances_per_minibatch)
        used = sum(len(idx) for idx in plan)
        if used < len(inputs):
            self._warn_truncation(len(inputs), self.numutterances_per_minibatch, used)
        for idx in plan:
            if not idx:
                continue
            if self.loss_kind == "ctc":  # label sequences of their own length
                deferred = all(isinstance(inputs[i], Unspliced) for i in idx)  # CMVN / splice on the device
                frames = [np.asarray(inputs[i]) if deferred else _spliced(inputs[i]) for i in idx]
                X = np.concatenate(frames, axis=0)
                if X.shape[0] == 0:
                    continue
                yield idx, CtcMicroBatch(
                    X, np.array([f.shape[0] for f in frames], dtype=np.int32),
                    np.concatenate([np.asarray(targets[i]).astype(np.int32).reshape(-1) for i in idx]),
                    np.array([np.asarray(targets[i]).size for i in idx], dtype=np.int32),
                    context_width=inputs[idx[0]].context_width if deferred else None,
                    cmvn=cmvn_table([inputs[i] for i in idx]) if deferred else None)
                continue
            for i in idx:
                if inputs[i].shape[0] != targets[i].shape[0]:
                    raise ValueError("utterance %d: %d input frames but %d targets (the cross-enthropy trainer "
                                     "needs equal lengths)" % (i, inputs[i].shape[0], targets[i].shape[0]))
            y = np.concatenate([np.asarray(targets[i]).astype(np.int32) for i in idx], axis=0)
            if y.shape[0] == 0:
                continue
            if all(isinstance(inputs[i], Unspliced) for i in idx):
                # splice on the device: ship the unspliced frames + utterance lengths
                raw = np.concatenate([np.asarray(inputs[i]) for i in idx], axis=0)
                lens = np.array([inputs[i].shape[0] for i in idx], dtype=np.int32)
                yield idx, RawMicroBatch(raw, y, lens, inputs[idx[0]].context_width, cmvn_table([inputs[i] for i in idx]))
            else:
                X = np.concatenate([_spliced(inputs[i]) for i in idx], axis=0)
                yield idx, (X, y)

    def _microbatches(self, inputs, targets):
        return [mb for _, mb in self._groups(inputs, targets)]

    def _step(self, microbatches, name, num_utts):
        """one optimiser step over the micro-batches of the method `name`: the loss before the update"""
        if not microbatches:
            raise ValueError("%s: the batch holds no frames (no micro-batch could be built from %d utterance(s))"
                             % (name, num_utts))
        loss = self.dp.train_step(self.engine, microbatches)
        self._summarise(loss)
        return loss

    def _evaluation(self, inputs, targets, build, *settings):
        """the loss of the micro-batches build(inputs, targets, *settings) in evaluation mode; None when there is no data
        (trainer.py:372-373)"""
        if inputs is None or targets is None:
            return None
        microbatches = build(inputs, targets, *settings)  # (what it refuses, it refuses before the engine is touched)
        return self.dp.eval_step(self.engine, microbatches)

    def update(self, inputs, targets):
        """
        update the neural model with a batch of training data

        Args:
            inputs: a list containing an NxF matrix for each utterance in the batch
            targets: a list containing an N-dimensional vector for each utterance
        Returns:
            the loss at this step (batch_loss / num_frames, evaluated before the parameter update)
        """
        return self._step(self._microbatches(inputs, targets), "Trainer.update", len(inputs))

    def _summarise(self, loss):
        if self.summarywriter is not None:
            self.summarywriter.write(json.dumps({"step": self.engine.global_step, "loss": loss,
                                                 "learning_rate": self.engine.scalar(_lib.LEARNING_RATE)}) + "\n")
            self.summarywriter.flush()

    def evaluate(self, inputs, targets):
        """the loss of the batch in evaluation mode; None when there is no data (trainer.py:372-373)"""
        return self._evaluation(inputs, targets, self._microbatches)

    # ---- the packed feed (BatchDispenser.next_packed): this rank's utterances only, CMVN + splice in HBM ----
    def selector(self):
        """the selector to hand to BatchDispenser.next_packed for batches meant for update_packed / evaluate_packed"""
        if getattr(self, "_selector", None) is None:
            self._selector = MicrobatchSelector(self.numutterances_per_minibatch, self.dp.rank, self.dp.world)
        return self._selector

    def _packed_microbatches(self, batch, stack=False, train=True):
        """the micro-batches of a PackedBatch as the engine takes them; stack: ONE object for all of them (training with
        the cross-enthropy loss: the engine runs consecutive micro-batches as one pass of the GEMMs when it can)"""
        out = []
        ce = self.loss_kind != "ctc"
        if ce and not np.array_equal(batch.lens, batch.target_lens):
            bad = int(np.flatnonzero(batch.lens != batch.target_lens)[0])
            raise ValueError("utterance %s: %d input frames but %d targets (the cross-enthropy trainer needs equal "
                             "lengths)" % (batch.utt_ids[bad], batch.lens[bad], batch.target_lens[bad]))
        entry = "accumulate_stacked_raw" if train else "eval_accumulate_stacked_raw"
        if stack and ce and len(batch.groups) > 1 and hasattr(self.engine, entry) and (
                train or os.environ.get("TFK_STACK", "1") != "0"):
            return [StackedRawMicroBatches(batch.frames, batch.targets, batch.lens, batch.context_width, batch.cmvn,
                                           [u1 - u0 for u0, u1, _, _, _, _ in batch.groups])]
        for u0, u1, r0, r1, t0, t1 in batch.groups:
            cmvn = None if batch.cmvn is None else batch.cmvn[u0:u1]
            if ce:
                out.append(RawMicroBatch(batch.frames[r0:r1], batch.targets[t0:t1], batch.lens[u0:u1],
                                         batch.context_width, cmvn))
            else:
                out.append(CtcMicroBatch(batch.frames[r0:r1], batch.lens[u0:u1], batch.targets[t0:t1],
                                         batch.target_lens[u0:u1], context_width=batch.context_width, cmvn=cmvn))
        return out

    def update_packed(self, batch, overlap=None):
        """Trainer.update for a PackedBatch selected with self.selector(): the same optimiser step from this rank's
        utterances alone.  `overlap()` runs once the step is enqueued and before the host waits for its loss."""
        total, _, end = batch.info
        if total == 0:
            raise ValueError("Trainer.update: the batch holds no frames (no micro-batch could be built from %d "
                             "utterance(s))" % batch.batch_utts)
        loss = self.dp.train_own(self.engine, self._packed_microbatches(batch, stack=True), total - end, overlap)
        self._summarise(loss)
        return loss

    def evaluate_packed(self, batch):
        """Trainer.evaluate for a PackedBatch selected with self.selector(); None when there is no data"""
        if batch is None:
            return None
        # (one stacked pass over all of this rank's micro-batches: rows are independent in evaluation mode)
        return self.dp.eval_own(self.engine, self._packed_microbatches(batch, stack=True, train=False))

    def halve_learning_rate(self):
        self.engine.halve_learning_rate()

    # ---- persistence (path prefixes chosen by the caller: nnet.py:140, 148, 206, 233, 238) ----
    def gather_parameters(self):
        """COLLECTIVE under data parallelism: make the fp32 parameters whole on this rank (the mixed-precision sharded
        exchange keeps each span's masters on its owner).  Every rank calls it before any rank saves."""
        self.dp.gather_parameters(self.engine)

    # Collective contract under data parallelism (one process per GPU):
    #   __init__ (seed broadcast), initialize, restore_model, restore_trainer, gather_parameters, update*, evaluate*
    #       are COLLECTIVE: every rank calls them at the same point of the program (a rank that restores or initialises
    #       alone deadlocks the others -- the reference is single-process and has no such rule).
    #   save_model / save_trainer are LOCAL (rank 0 alone writes) but read the fp32 parameters: every rank must have
    #       called gather_parameters() since the last update (Nnet's schedule does); otherwise they raise on the caller.
    def save_model(self, filename):
        """LOCAL; needs gather_parameters() on every rank first when the fp32 masters are sharded"""
        self.modelsaver.save(None, filename)

    def restore_model(self, filename):
        """COLLECTIVE under data parallelism: every rank restores"""
        self.dp.gather_parameters(self.engine)
        self.modelsaver.restore(None, filename)

    def save_trainer(self, filename):
        """model + the `train_variables` scope: global_step and learning_rate_fact.  As in the reference
        (trainer.py:204-205) the Adam moments and beta powers are NOT part of a checkpoint.  LOCAL (see save_model)."""
        self.modelsaver.save(None, filename)
        tmp = filename + "_trainvars.tmp%d" % os.getpid()
        with open(tmp, "wb") as fid:
            np.savez(fid, global_step=np.array(self.engine.global_step, dtype=np.int64),
                     learning_rate_fact=np.array(self.engine.scalar(_lib.LEARNING_RATE_FACT), dtype=np.float64))
        os.replace(tmp, filename + "_trainvars")

    def restore_trainer(self, filename):
        """COLLECTIVE under data parallelism: every rank restores"""
        self.dp.gather_parameters(self.engine)
        self.modelsaver.restore(None, filename)
        with np.load(filename + "_trainvars") as data:
            self.engine.set_scalar(_lib.GLOBAL_STEP, int(data["global_step"]))
            self.engine.set_scalar(_lib.LEARNING_RATE_FACT, float(data["learning_rate_fact"]))

    def close(self):
        if self.summarywriter is not None:
            self.summarywriter.close()
            self.summarywriter = None
        self.dp.drain(self.engine)
        self.engine.synchronize()
        self.engine.close()


class CrossEnthropyTrainer(Trainer):
    """A trainer that minimises the cross-enthropy loss; the output sequences must be of the same length as
    the input sequences (reference trainer.py:488-531).  The loss is the SUM over frames of
    softmax_cross_entropy_with_logits against the one-hot pdf-ids."""

    def compute_loss(self, targets, logits, logit_seq_length, target_seq_length):
        return "cross_enthropy"


class CTCTrainer(Trainer):
    """A trainer that minimises the CTC loss (reference trainer.py:533-570).  The reference's compute_loss cannot
    run -- it iterates over range(len(batch_size)) of an int, fills the sparse label values from the logits and
    returns nothing -- so this is what that method means to build: tf.nn.ctc_loss on the time-major logits with the
    op's conventions (the blank is the LAST class, so the classifier needs num_labels + 1 outputs; repeated labels
    are merged), summed over the utterances.  As everywhere in the Trainer, num_frames counts TARGET lengths
    (trainer.py:126-133): the reported loss and the mean gradient are per label.  Checked against
    oracle/ctc_oracle.py (pinned to torch's ctc_loss), not against the reference: parity unpinned."""

    def compute_loss(self, targets, logits, logit_seq_length, target_seq_length):
        return "ctc"

    def label_errors(self, inputs, targets, beam_width=None, lm=None, label_topk=None, rescore_paths=None):
        """Label errors of the batch under best-path decoding -- tf.nn.ctc_greedy_decoder(merge_repeated=True) followed by
        tf.edit_distance(normalize=False), the reference framework's standard CTC evaluation -- in evaluation mode, on the
        device (tfk_ctc_greedy).  Returns (sum of the Levenshtein distances, sum of the reference lengths) over the batch as
        Python ints: a corpus label error rate is sum(edits) / sum(reference labels) over its batches.  None when there is
        no data (as evaluate).  COLLECTIVE under data parallelism: the micro-batches are dealt to the ranks as in evaluate
        and the two counts summed over them.  beam_width: an int decodes by prefix beam search of that width instead
        (tf.nn.ctc_beam_search_decoder, tfk_ctc_beam) and counts the errors of its best path.  lm: a ctc_lm.NgramLM or GraphLM ranks
        the beam's prefixes by acoustic + language-model score (tfk_ctc_beam_lm); it needs a beam_width.  label_topk: an int
        prunes the search to the frame's label_topk most probable labels (tfk_ctc_beam_topk), which is what lets a model of
        more than 64 outputs be searched; it needs a beam_width too.  rescore_paths: an int N decodes the N best, scores
        them exactly on the device with their label errors (tfk_ctc_score) and counts the hypothesis that is best after
        re-ranking by exact score (+ lm.score with lm: decoder.ctc_rerank); it needs a beam_width as well."""
        _beam_settings(beam_width, lm, label_topk, rescore_paths)
        if inputs is None or targets is None:
            return None
        kw = {} if lm is None else {"lm": lm}
        if label_topk is not None:
            kw["label_topk"] = label_topk
        if rescore_paths is not None:
            kw["rescore_paths"] = rescore_paths
        return self.dp.label_errors(self.engine, self._microbatches(inputs, targets), beam_width=beam_width, **kw)

    # ---- training on the expected number of label errors over an N-best list (MWER) ----
    def _mwer_microbatches(self, inputs, targets, beam_width, top_paths, ctc_weight, lm, label_topk, add_reference, hyps):
        from .ctc_mwer import pair_tables
        if hyps is None:
            if beam_width is None:
                raise ValueError("MWER needs an N-best list: give beam_width (and top_paths), or hyps")
            top_paths = CtcMwerMicroBatch.search_paths(beam_width, top_paths)
        elif len(hyps) != len(inputs):
            raise ValueError("hyps: %d hypothesis lists for %d utterances" % (len(hyps), len(inputs)))
        if lm is not None and (beam_width is None or hyps is not None):
            raise ValueError("a language model ranks the prefixes of a beam search: give beam_width with lm (and no hyps)")
        if label_topk is not None and (beam_width is None or hyps is not None):
            raise ValueError("label_topk prunes a beam search: give beam_width with label_topk (and no hyps)")
        ctc_weight = _finite_nonneg("ctc_weight", ctc_weight)
        out = []
        for idx, mb in self._groups(inputs, targets):
            kw = dict(context_width=mb.context_width, cmvn=mb.cmvn, add_reference=add_reference, ctc_weight=ctc_weight)
            if hyps is None:
                kw.update(beam_width=int(beam_width), top_paths=int(top_paths), lm=lm, label_topk=label_topk)
            else:
                counts, labels, lens = pair_tables([hyps[i] for i in idx])
                kw.update(hyp_counts=counts, hyp_labels=labels, hyp_lens=lens)
            out.append(CtcMwerMicroBatch(mb.X, mb.utt_lens, mb.labels, mb.label_lens, **kw))
        return out

    def update_mwer(self, inputs, targets, beam_width=None, top_paths=None, ctc_weight=0.01, lm=None, label_topk=None,
                    add_reference=False, hyps=None):
        """One optimiser step on the EXPECTED NUMBER OF LABEL ERRORS over every utterance's N-best list (MWER,
        tfk_accumulate_ctc_mwer; Prabhavalkar et al. 2018) plus ctc_weight x the CTC loss -- the criterion label_errors
        reports, where update minimises the likelihood.  The list: the top_paths best (default: all beam_width) of a prefix
        beam search of width beam_width, decoded in evaluation mode by the rank that trains the micro-batch right before it
        does (lm: a ctc_lm.NgramLM or GraphLM ranks the search; label_topk: the pruned search, for models of more than 64 outputs); or
        hyps, a list per utterance of label arrays, which skips the search.  add_reference: the reference joins every list
        that lacks it.  The hypotheses are scored on the train-mode logits of the step itself.  Returns the step's loss:
        expected label errors per reference label + ctc_weight x CTC loss per label, before the update."""
        return self._step(self._mwer_microbatches(inputs, targets, beam_width, top_paths, ctc_weight, lm, label_topk,
                                                  add_reference, hyps), "CTCTrainer.update_mwer", len(inputs))

    def evaluate_mwer(self, inputs, targets, beam_width=None, top_paths=None, ctc_weight=0.01, lm=None, label_topk=None,
                      add_reference=False, hyps=None):
        """the same figure in evaluation mode, without an update; None when there is no data (as evaluate)"""
        return self._evaluation(inputs, targets, self._mwer_microbatches, beam_width, top_paths, ctc_weight, lm, label_topk,
                                add_reference, hyps)

    # ---- MMI against a denominator graph (CTC-CRF): the exact sum over every label sequence a grammar accepts ----
    def _mmi_microbatches(self, inputs, targets, graph, lm_scale, ctc_weight):
        if graph is None or getattr(graph, "next", None) is None:
            raise ValueError("MMI needs a denominator graph: a ctc_lm.GraphLM")
        lm_scale, ctc_weight = _finite_nonneg("lm_scale", lm_scale), _finite_nonneg("ctc_weight", ctc_weight)
        for u, ref in enumerate(targets):
            ref = np.asarray(ref).reshape(-1)
            s, at = graph._walk(ref)
            if s is None:
                raise ValueError("utterance %d: the denominator graph has no arc for label %d of its reference (position %d)"
                                 % (u, int(ref[at]), at))
            if not graph.table[s, -1] > -np.inf:
                raise ValueError("utterance %d: its reference ends in state %d of the denominator graph, which is not final"
                                 % (u, s))
        return [CtcMmiMicroBatch(mb.X, mb.utt_lens, mb.labels, mb.label_lens, graph, context_width=mb.context_width,
                                 cmvn=mb.cmvn, lm_scale=lm_scale, ctc_weight=ctc_weight)
                for mb in self._microbatches(inputs, targets)]

    def update_mmi(self, inputs, targets, graph, lm_scale=1.0, ctc_weight=0.0):
        """One optimiser step on MAXIMUM MUTUAL INFORMATION against the denominator graph (tfk_accumulate_ctc_mmi; CTC-CRF):
        per utterance -(log p_ctc(reference) + lm_scale G(reference)) + log Z, with Z the total likelihood of EVERY label
        sequence `graph` (a ctc_lm.GraphLM; its final weights are always read) accepts, summed exactly on the device -- no
        decode, no N-best list -- plus ctc_weight x the CTC loss.  The graph is set on the engine when it changes.  A
        denominator from transcripts is GraphLM.from_ngram(NgramLM.from_label_sequences(...)); a lexicon is
        GraphLM.from_lexicon(...).  A reference the graph rejects raises a ValueError that names the utterance before the
        step starts.  Returns the step's loss per reference label, before the update."""
        return self._step(self._mmi_microbatches(inputs, targets, graph, lm_scale, ctc_weight), "CTCTrainer.update_mmi",
                          len(inputs))

    def evaluate_mmi(self, inputs, targets, graph, lm_scale=1.0, ctc_weight=0.0):
        """the same figure in evaluation mode, without an update; None when there is no data (as evaluate)"""
        return self._evaluation(inputs, targets, self._mmi_microbatches, graph, lm_scale, ctc_weight)

    # ---- training on partial transcripts: the CTC loss with wildcard gaps (W-CTC / STC) ----
    def _wild_microbatches(self, inputs, targets, wild, penalty):
        from .decoder import Decoder
        if len(inputs) != len(targets):
            raise ValueError("%d utterances, %d label sequences" % (len(inputs), len(targets)))
        penalty = _finite_nonneg("penalty", penalty)
        seqs = [np.asarray(t).astype(np.int32).reshape(-1) for t in targets]
        flat = Decoder._gap_flags(wild, seqs)  # (validates `wild`; len(s) + 1 flags per utterance, back to back)
        first = np.concatenate([[0], np.cumsum([s.size + 1 for s in seqs], dtype=np.int64)])
        out = []
        # the flags are cut per micro-batch: utterance u's start at lab_off[u] + u THERE
        for idx, mb in self._groups(inputs, targets):
            cut = None if flat is None else np.concatenate([flat[first[i]:first[i + 1]] for i in idx])
            out.append(CtcWildMicroBatch(mb.X, mb.utt_lens, mb.labels, mb.label_lens, wild=cut, penalty=penalty,
                                         context_width=mb.context_width, cmvn=mb.cmvn))
        return out

    def update_wild(self, inputs, targets, wild="ends", penalty=0.0):
        """One optimiser step on the CTC loss with WILDCARD GAPS (tfk_accumulate_ctc_wild; W-CTC, Cai et al. 2022; the star
        token of STC, Pratap et al. 2022), for transcripts that cover only PART of a recording: a flagged gap of the label
        sequence absorbs any frames at `penalty` per frame (finite, >= 0; 0: free), where update would force them onto
        blanks or the neighbouring labels.  wild as Decoder.ctc_align_wild takes it: "ends" (untranscribed material before
        and after the transcript), "all", None (update's criterion), or one boolean array of len(targets[u]) + 1 flags per
        utterance.  The loss is the value of the lattice -- a frame labelling that several lattice paths reach through a
        wildcard counts once per path -- so it can be negative.  A bad wild or penalty raises a ValueError before the step
        starts.  Returns the step's loss per reference label, before the update."""
        return self._step(self._wild_microbatches(inputs, targets, wild, penalty), "CTCTrainer.update_wild", len(inputs))

    def evaluate_wild(self, inputs, targets, wild="ends", penalty=0.0):
        """the same figure in evaluation mode, without an update; None when there is no data (as evaluate)"""
        return self._evaluation(inputs, targets, self._wild_microbatches, wild, penalty)
