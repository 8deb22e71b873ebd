"""Decoding environment with the reference's interface (neuralNetworks/decoder.py)."""
import os

import numpy as np

from ..processing.feature_reader import Unspliced, cmvn_table
from .classifiers.dnn import ModelSaver


def ctc_segments(ali, labels):
    """The segments of one utterance's alignment (Decoder.ctc_align): `ali` per frame the position of the label the frame
    emits, -1 for a blank frame; `labels` the utterance's label sequence.  Returns [(label, first_frame,
    end_frame_exclusive)], one entry per label, in order: the frames that emit that label (consecutive in a valid
    alignment); blank frames belong to no segment.  `ali` None (no valid alignment) gives None."""
    if ali is None:
        return None
    ali = np.asarray(ali).reshape(-1)
    labels = np.asarray(labels).reshape(-1)
    frames = np.nonzero(ali >= 0)[0]
    pos = ali[frames]
    if pos.size and (pos.max() >= labels.size or np.any(np.diff(pos) < 0)):
        raise ValueError("not an alignment of %d labels: positions must be non-decreasing and below the label count"
                         % labels.size)
    first = np.searchsorted(pos, np.arange(labels.size), side="left")
    last = np.searchsorted(pos, np.arange(labels.size), side="right")
    if np.any(first == last):
        raise ValueError("label %d of %d emits no frame" % (int(np.nonzero(first == last)[0][0]), labels.size))
    if np.any(frames[last - 1] - frames[first] != last - 1 - first):
        raise ValueError("the frames of one label are not consecutive")
    return [(int(k), int(frames[a]), int(frames[b - 1]) + 1) for k, a, b in zip(labels, first, last)]


class _Graph(object):
    def finalize(self):
        pass


class Decoder(object):
    """Forward-only environment: evaluation-mode classifier + softmax (reference decoder.py:11-47)."""

    def __init__(self, classifier, input_dim, max_length, device=None):
        """
        Args:
            classifier: the classifier that will be used for decoding
            input_dim: the input dimension to the nnnetgraph
            max_length: the maximal utterance length
        """
        self.graph = _Graph()
        self.max_length = max_length
        if device is None:
            from ..dataparallel import local_device
            device = local_device()
        self.engine = classifier.create_engine(input_dim, max_frames=min(max(int(max_length), 1), 1 << 16), device=device)
        self.saver = ModelSaver(self.engine)
        self.graph.finalize()

    def _check(self, inputs):
        inputs = np.asarray(inputs)
        if inputs.shape[0] > self.max_length:  # the reference's zero padding has a negative size here
            raise ValueError("negative dimensions are not allowed")
        return inputs

    def _run(self, inputs, **kw):
        if isinstance(inputs, Unspliced):  # splice on the device
            self._check(inputs)
            return self.engine.posteriors_raw(np.asarray(inputs), [inputs.shape[0]], inputs.context_width,
                                              cmvn=cmvn_table([inputs]), **kw)
        return self.engine.posteriors(self._check(inputs), **kw)

    def __call__(self, inputs):
        """NxF features -> NxO state posteriors (reference decoder.py:49-71)"""
        return self._run(inputs)

    def log_likelihoods(self, inputs):
        """log(posterior / prior), fused in the softmax kernel; needs set_prior (reference nnet.py:280-286)"""
        return self._run(inputs, log_div_prior=True)

    def _batch(self, utterances):
        """The utterances of ONE forward pass: (lens, raw, frames, context_width, cmvn).  All `Unspliced`
        -> raw: the unspliced frames back to back with their context width and CMVN table, for the device-side splice with
        utterance boundaries; otherwise the spliced matrices stacked (frames are independent once spliced)."""
        for u in utterances:
            self._check(u)
        lens = [u.shape[0] for u in utterances]
        if all(isinstance(u, Unspliced) for u in utterances):
            return (lens, True, np.concatenate([np.asarray(u) for u in utterances]), utterances[0].context_width,
                    cmvn_table(utterances))
        stack = np.concatenate([u.spliced() if isinstance(u, Unspliced) else np.asarray(u, dtype=np.float32)
                                for u in utterances])
        return lens, False, stack, None, None

    def _ctc(self, entry, utterances, *args, **kw):
        """engine.<entry> (spliced) or engine.<entry>_raw (all `Unspliced`) on the batch of `utterances`"""
        lens, raw, frames, context_width, cmvn = self._batch(utterances)
        if raw:
            return getattr(self.engine, entry + "_raw")(frames, lens, context_width, *args, cmvn=cmvn, **kw)
        return getattr(self.engine, entry)(frames, lens, *args, **kw)

    def decode_batch(self, utterances, log_div_prior=True):
        """Several utterances in ONE forward pass: returns a list of per-utterance [N_i, O] arrays.
        All `Unspliced` -> device-side splice with utterance boundaries; otherwise the spliced matrices are
        simply stacked (frames are independent once spliced)."""
        lens, raw, frames, context_width, cmvn = self._batch(utterances)
        if raw:
            flat = self.engine.posteriors_raw(frames, lens, context_width, log_div_prior=log_div_prior, cmvn=cmvn)
        else:
            flat = self.engine.posteriors(frames, log_div_prior=log_div_prior)
        return np.split(flat, np.cumsum(lens)[:-1])

    def ctc_best_path(self, utterances):
        """Best-path decoding of a CTC model (tf.nn.ctc_greedy_decoder with merge_repeated=True, the reference framework's
        standard CTC evaluation): every utterance in ONE forward pass, per frame the largest logit, repeats merged, blanks
        (the last class) removed, on the device (tfk_ctc_greedy).  Returns one int32 label array per utterance; text comes
        from the trainer's TargetCoder.decode.  All `Unspliced` -> device-side splice, as decode_batch."""
        if len(utterances) == 0:
            return []
        return self._ctc("ctc_greedy", utterances)[0]

    def ctc_beam_search(self, utterances, beam_width=100, top_paths=1, label_topk=None):
        """Prefix beam search decoding of a CTC model (tf.nn.ctc_beam_search_decoder with merge_repeated=False, its default
        beam_width): every utterance in ONE forward pass, the search on the device (tfk_ctc_beam).  Returns (hyps, scores):
        hyps[u][n] the n-th best int32 label array of utterance u, scores float32 [U, top_paths] their natural-log
        probabilities.  All `Unspliced` -> device-side splice, as decode_batch.  label_topk: an int prunes the search to the
        frame's label_topk (1 to 63) most probable labels (tfk_ctc_beam_topk) -- the way to search a model of more than 64
        outputs, and a cheaper search below that; None is the unpruned search."""
        if len(utterances) == 0:
            return [], np.zeros((0, top_paths), dtype=np.float32)
        kw = {} if label_topk is None else {"label_topk": label_topk}
        return self._ctc("ctc_beam", utterances, beam_width=beam_width, top_paths=top_paths, **kw)[:2]

    def ctc_beam_search_lm(self, utterances, lm, beam_width=100, top_paths=1, label_topk=None):
        """ctc_beam_search with a character n-gram language model (ctc_lm.NgramLM; tfk_ctc_beam_lm): prefixes are ranked by
        acoustic score + lm.weight * model log-probability + lm.label_bonus per label.  Returns (hyps, scores, am_scores):
        as ctc_beam_search, scores the combined values, am_scores float32 [U, top_paths] their acoustic parts.  label_topk:
        as ctc_beam_search."""
        if len(utterances) == 0:
            return [], np.zeros((0, top_paths), dtype=np.float32), np.zeros((0, top_paths), dtype=np.float32)
        lens, raw, frames, context_width, cmvn = self._batch(utterances)
        kw = dict(beam_width=beam_width, top_paths=top_paths)
        if label_topk is not None:
            kw["label_topk"] = label_topk
        if raw:
            return self.engine.ctc_beam_lm_raw(frames, lens, context_width, lm, cmvn=cmvn, **kw)[:3]
        return self.engine.ctc_beam_lm(frames, lens, lm, **kw)[:3]

    def ctc_align(self, utterances, targets):
        """Forced alignment of a CTC model (tfk_ctc_align; the algorithm is stated in include/tfkaldi_hip.h): every
        utterance in ONE forward pass, the Viterbi path of its known label sequence `targets[u]` (one int label array per
        utterance) on the device.  Returns (alis, scores): alis[u] int32 [frames of u], per frame the position in
        targets[u] of the label the frame emits, -1 for a blank frame (None for an utterance too short for its labels);
        scores float32 [U], the natural-log probability of the alignment.  ctc_segments turns an alignment into (label,
        first frame, end frame) triples.  All `Unspliced` -> device-side splice, as decode_batch."""
        if len(utterances) != len(targets):
            raise ValueError("%d utterances, %d label sequences" % (len(utterances), len(targets)))
        if len(utterances) == 0:
            return [], np.zeros(0, dtype=np.float32)
        targets = [np.asarray(t, dtype=np.int32).reshape(-1) for t in targets]
        return self._ctc("ctc_align", utterances, np.concatenate(targets), [t.size for t in targets])

    def set_prior(self, prior):
        self.engine.set_prior(prior)

    def restore(self, filename):
        """load the saved neural net (reference decoder.py:73-81)"""
        self.saver.restore(None, filename)

    def close(self):
        self.engine.close()
