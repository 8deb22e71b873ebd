"""Decoding environment with the reference's interface (neuralNetworks/decoder.py)."""
import os

import numpy as np

from ..processing.feature_reader import StreamSplicer, Unspliced, cmvn_table
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


def ctc_rerank(hyps, exact_scores, lm=None):
    """Second-pass ranking of ONE utterance's N-best list: `hyps` int label arrays in the first pass's order,
    `exact_scores` their exact log-probabilities log p(labels | x) (Decoder.ctc_score).  The combined score of a hypothesis
    is its exact score plus lm.score(h) (a ctc_lm.NgramLM or GraphLM: weight, label bonus and end term as the search uses them), in
    float64.  Returns (order, scores, posteriors): `order` the indices into hyps by descending combined score -- a stable
    sort, so a tie keeps the first pass's order -- `scores` float64 the combined scores in that order, `posteriors` float64
    their softmax over the list (a -inf hypothesis sorts last with posterior 0; a list without a finite score gets zeros)."""
    am = np.asarray(exact_scores, dtype=np.float64).reshape(-1)
    if am.size != len(hyps):
        raise ValueError("%d hypotheses, %d scores" % (len(hyps), am.size))
    if np.any(np.isnan(am)) or np.any(am == np.inf):
        raise ValueError("exact scores are log-probabilities: finite or -inf")
    total = am.copy()
    if lm is not None:
        total += np.array([lm.score(h) for h in hyps], dtype=np.float64).reshape(am.shape)
    order = np.argsort(-total, kind="stable")
    scores = total[order]
    post = np.zeros_like(scores)
    if scores.size and scores[0] > -np.inf:
        post = np.exp(scores - scores[0])
        post /= post.sum()
    return order, scores, post


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
        """ctc_beam_search with a language model over the labels (ctc_lm.NgramLM, or a GraphLM, which
        also restricts the search to the sequences it accepts; tfk_ctc_beam_lm): prefixes are ranked by
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

    @staticmethod
    def _gap_flags(wild, seqs):
        """the gap flags of `seqs` (int label arrays) back to back, len(s) + 1 per sequence, as uint8 -- or None.  wild:
        "ends" (the gap before the first and after the last label), "all", None, or one boolean array per sequence."""
        if wild is None:
            return None
        if isinstance(wild, str):
            if wild not in ("ends", "all"):
                raise ValueError('wild is %r: expected "ends", "all", None or one flag array per sequence' % (wild,))
            flags = [np.ones(s.size + 1, dtype=np.uint8) for s in seqs]
            if wild == "ends":
                for f in flags:
                    f[1:-1] = 0
        else:
            if len(wild) != len(seqs):
                raise ValueError("%d flag arrays for %d label sequences" % (len(wild), len(seqs)))
            flags = [np.asarray(f).astype(bool).astype(np.uint8).reshape(-1) for f in wild]
            for f, s in zip(flags, seqs):
                if f.size != s.size + 1:
                    raise ValueError("%d gap flags for %d labels: a sequence of S labels has S + 1 gaps" % (f.size, s.size))
        return np.concatenate(flags) if flags else np.zeros(0, dtype=np.uint8)

    def ctc_align_wild(self, utterances, targets, wild="ends"):
        """ctc_align for transcripts that cover only PART of a recording (tfk_ctc_align_wild; the contract is stated in
        include/tfkaldi_hip.h): a gap of the label sequence -- before the first label, between two labels, after the last --
        whose flag is set is a wildcard that may hold anything (it emits the frame's best class).  wild: "ends" (untranscribed
        material before and after the transcript), "all", None (ctc_align's result), or one boolean array of
        len(targets[u]) + 1 flags per utterance.  Returns (alis, scores, free): as ctc_align, -1 for a frame in any gap (None
        for an utterance without a path), and free float32 [U], the log-probability of the unconstrained best path:
        scores - free <= 0 is what the transcript costs against it.  ctc_segments works on alis unchanged."""
        if len(utterances) != len(targets):
            raise ValueError("%d utterances, %d label sequences" % (len(utterances), len(targets)))
        if len(utterances) == 0:
            return [], np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32)
        targets = [np.asarray(t, dtype=np.int32).reshape(-1) for t in targets]
        return self._ctc("ctc_align_wild", utterances, np.concatenate(targets), [t.size for t in targets],
                         wild=self._gap_flags(wild, targets))

    def ctc_spot(self, utterances, patterns, wild="ends"):
        """Keyword spotting with a CTC model (tfk_ctc_spot; the contract is stated in include/tfkaldi_hip.h): every one of
        the K `patterns` (int label arrays) is searched in every utterance, U x K pairs in ONE forward pass.  wild as
        ctc_align_wild, per pattern ("ends": the keyword may lie anywhere in the utterance).  Returns (scores [U, K] float32,
        starts [U, K] int32, ends [U, K] int32, free [U] float32): for every pair what ctc_align_wild gives for that utterance
        and pattern -- the score of the best path, the first frame that emits a label and one past the last (-inf, -1, -1
        without a path; 0, 0 for an empty pattern).  scores - free[:, None] <= 0 ranks the hits: 0 means the pattern lies on
        the model's best path."""
        patterns = [np.asarray(p, dtype=np.int32).reshape(-1) for p in patterns]
        U, K = len(utterances), len(patterns)
        flags = self._gap_flags(wild, patterns)
        if U == 0:
            return (np.zeros((0, K), dtype=np.float32), np.zeros((0, K), dtype=np.int32), np.zeros((0, K), dtype=np.int32),
                    np.zeros(0, dtype=np.float32))
        labels = np.tile(np.concatenate(patterns), U) if K else np.zeros(0, dtype=np.int32)
        scores, starts, ends, free = self._ctc("ctc_spot", utterances, [K] * U, labels, [p.size for p in patterns] * U,
                                               wild=None if flags is None else np.tile(flags, U))
        return (np.asarray(scores, dtype=np.float32).reshape(U, K), np.asarray(starts, dtype=np.int32).reshape(U, K),
                np.asarray(ends, dtype=np.int32).reshape(U, K), free)

    def ctc_score(self, utterances, hyps, refs=None):
        """N-best rescoring of a CTC model (tfk_ctc_score; the contract is stated in include/tfkaldi_hip.h): every utterance
        in ONE forward pass, then for every hypothesis hyps[u][n] (a list of int label arrays per utterance, possibly empty)
        the EXACT log-probability log p(labels | x), the sum over all its CTC alignments, on the device.  refs: one int
        label array per utterance, for the label errors.  Returns (scores, edits): scores[u] float32 [len(hyps[u])], edits[u]
        int32 Levenshtein distances to refs[u] (edits None without refs).  All `Unspliced` -> device-side splice."""
        if len(utterances) != len(hyps) or (refs is not None and len(refs) != len(utterances)):
            raise ValueError("%d utterances, %d hypothesis lists, %s references"
                             % (len(utterances), len(hyps), "no" if refs is None else len(refs)))
        if len(utterances) == 0:
            return [], None if refs is None else []
        flat = [np.asarray(h, dtype=np.int32).reshape(-1) for hs in hyps for h in hs]
        labels = np.concatenate(flat) if flat else np.zeros(0, dtype=np.int32)
        kw = {}
        if refs is not None:
            refs = [np.asarray(r, dtype=np.int32).reshape(-1) for r in refs]
            kw = {"ref_labels": np.concatenate(refs), "ref_lens": [r.size for r in refs]}
        return self._ctc("ctc_score", utterances, [len(hs) for hs in hyps], labels, [h.size for h in flat], **kw)

    def ctc_rescore(self, utterances, beam_width=100, top_paths=10, lm=None, label_topk=None):
        """Two-pass decoding of a CTC model: the prefix beam search (ctc_beam_search, or ctc_beam_search_lm with `lm`;
        label_topk as there), then ONE ctc_score pass over the paths whose beam score is finite (padding paths are not
        scored), then ctc_rerank per utterance: the beam's scores count only the alignments that survived its pruning, the
        second pass ranks by what the model really assigns (plus lm.score).  Returns (hyps, scores, am_scores, beam_rank,
        posteriors), per utterance in the new order: hyps[u] the int32 label arrays, scores[u] float64 the combined scores,
        am_scores[u] float32 the exact log-probabilities, beam_rank[u] the position each hypothesis had in the beam's
        list, posteriors[u] float64 the softmax of the combined scores over the list."""
        if len(utterances) == 0:
            return [], [], [], [], []
        if lm is None:
            found, beam = self.ctc_beam_search(utterances, beam_width, top_paths, label_topk)
        else:
            found, _, beam = self.ctc_beam_search_lm(utterances, lm, beam_width, top_paths, label_topk)
        kept = [[h for h, s in zip(hs, sc) if s > -np.inf] for hs, sc in zip(found, beam)]
        exact = self.ctc_score(utterances, kept)[0]
        out = ([], [], [], [], [])
        for hs, am in zip(kept, exact):
            order, scores, post = ctc_rerank(hs, am, lm)
            for dst, v in zip(out, ([hs[i] for i in order], scores, am[order], order.astype(np.int32), post)):
                dst.append(v)
        return out

    def ctc_stream(self, lanes=1, beam_width=100, max_frames=None, lm=None, label_topk=None, context_width=None):
        """Streaming decoding of a CTC model: `lanes` live sessions whose beam search is resumed chunk by chunk
        (tfk_ctc_stream_*; the contract is stated in include/tfkaldi_hip.h).  Whatever the chunks are, the hypotheses and
        scores are those of ctc_beam_search (with lm: ctc_beam_search_lm) on the frames pushed so far, bit for bit on the same
        logits.  max_frames: the most frames a lane decodes between two resets (default: this decoder's max_length).
        context_width: given, the chunks are UNSPLICED frames [n, D] and every lane splices them on the host
        (processing.feature_reader.StreamSplicer), which holds a lane's newest context_width frames back until their right
        context has arrived; None, the chunks are spliced rows.  Returns a CtcStream."""
        return CtcStream(self, lanes, beam_width, self.max_length if max_frames is None else max_frames, lm, label_topk,
                         context_width)

    def set_prior(self, prior):
        self.engine.set_prior(prior)

    def restore(self, filename):
        """load the saved neural net (reference decoder.py:73-81)"""
        self.saver.restore(None, filename)

    def close(self):
        self.engine.close()


class CtcStream(object):
    """What Decoder.ctc_stream returns: the sessions of one decode stream.  push() feeds chunks, partial() reads the N-best so
    far (as often as wanted: it changes nothing), finish() ends a lane's utterance, reset() starts the next one."""

    def __init__(self, decoder, lanes, beam_width, max_frames, lm, label_topk, context_width):
        self.engine, self.lm, self.lanes = decoder.engine, lm, int(lanes)
        self.context_width = None if context_width is None else int(context_width)
        self.handle = self.engine.ctc_stream_open(lanes, beam_width, max_frames, label_topk)
        self.splicers = None
        if self.context_width is not None:
            win = 2 * self.context_width + 1
            if self.context_width < 0 or self.engine.F % win:
                raise ValueError("input_dim %d is not a multiple of 2 * context_width + 1 = %d" % (self.engine.F, win))
            self.splicers = [StreamSplicer(self.engine.F // win, self.context_width) for _ in range(self.lanes)]

    def _push_rows(self, rows):
        lens = [r.shape[0] for r in rows]
        self.handle.push(np.concatenate(rows), lens, self.lm)

    def push(self, chunks):
        """chunks: one array per lane -- unspliced frames [n, D] with context_width, else spliced rows [n, F] -- or None for
        a lane that has nothing new"""
        if len(chunks) != self.lanes:
            raise ValueError("%d chunks for %d lanes" % (len(chunks), self.lanes))
        empty = np.zeros((0, self.engine.F), dtype=np.float32)
        rows = []
        for l, chunk in enumerate(chunks):
            if chunk is None:
                rows.append(empty)
            elif self.splicers is not None:
                rows.append(self.splicers[l].push(chunk))
            else:
                rows.append(np.ascontiguousarray(chunk, dtype=np.float32).reshape(-1, self.engine.F))
        self._push_rows(rows)

    def _nbest(self, top_paths, final):
        hyps, scores, am = self.handle.result(top_paths, final=final)
        return (hyps, scores) if self.lm is None else (hyps, scores, am)

    def partial(self, top_paths=1):
        """(hyps, scores[, am_scores with a model]) of every lane over the rows decoded so far: hyps[l][n], scores
        [lanes, top_paths].  With context_width a lane's newest context_width frames are not in it yet."""
        return self._nbest(top_paths, False)

    def finish(self, lane, top_paths=1):
        """The end of lane's utterance: its held-back frames are spliced with zero right context and pushed, and its final
        N-best is returned -- (hyps[n], scores [top_paths][, am_scores]) -- ranked with the model's end term when the model has
        one.  The lane keeps its state until reset()."""
        rows = [np.zeros((0, self.engine.F), dtype=np.float32) for _ in range(self.lanes)]
        if self.splicers is not None:
            rows[lane] = self.splicers[lane].flush()
        self._push_rows(rows)
        return tuple(part[lane] for part in self._nbest(top_paths, True))

    def reset(self, lane=None, cmvn=None):
        """lane (None: every lane) starts a new utterance; cmvn: the [2, D] (mean, standard deviation) table its splicer
        normalises the coming frames with (None: they come normalised)"""
        self.handle.reset(lane)
        if self.splicers is not None:
            for l in range(self.lanes) if lane is None else [lane]:
                self.splicers[l].flush()
                self.splicers[l].set_cmvn(cmvn)

    def frames(self):
        return self.handle.frames()

    def close(self):
        self.handle.close()
