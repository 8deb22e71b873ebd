"""Python handle on one C-ABI engine (include/tfkaldi_hip.h): numpy in, numpy out.

This is plumbing only -- every FLOP of the hot path runs in libtfkaldi_hip.so.  The classes of
tfkaldi_amd.neuralNetworks (Trainer / Decoder / DNN) are built on it.
"""
from contextlib import contextmanager
from ctypes import byref, c_double, c_float, c_int, c_size_t, c_uint64, c_void_p

import numpy as np

from . import _lib
from ._lib import (ADAM_STEPS, BIASES, BN_BETA, BN_MOVING_MEAN, BN_MOVING_VAR, GLOBAL_STEP, INITIALISED_LAYERS,
                   LEARNING_RATE, LEARNING_RATE_FACT, SLOT_ADAM_M, SLOT_ADAM_V, SLOT_GRAD, SLOT_PARAM, WEIGHTS,
                   check)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return c_void_p(None) if a is None else a.ctypes.data_as(c_void_p)


def _finite_nonneg(name, value):
    """`value` (a weight, a scale, a per-frame penalty) as a float that is finite and >= 0, or a ValueError that names it"""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s %r must be finite and >= 0" % (name, value))
    if not (np.isfinite(v) and v >= 0.0):
        raise ValueError("%s %r must be finite and >= 0" % (name, v))
    return v


def _levenshtein(a, b):
    """Levenshtein distance (unit costs) of two int sequences: what the entries report when the engine is not called"""
    row = np.arange(len(b) + 1)
    for i, x in enumerate(a):
        new = np.empty_like(row)
        new[0] = i + 1
        for j, y in enumerate(b):
            new[j + 1] = min(row[j + 1] + 1, new[j] + 1, row[j] + (x != y))
        row = new
    return int(row[-1])


class Engine(object):
    """One engine per GPU.  `torch_state=True` keeps the persistent state in a torch CUDA tensor and
    runs on a torch stream so torch.distributed (RCCL) can all-reduce views of the gradient region."""

    def __init__(self, cfg, torch_state=False):
        self.lib = _lib.load()
        self.cfg = cfg
        self.F, self.L, self.H, self.O = cfg.input_dim, cfg.num_layers, cfg.num_units, cfg.output_dim
        self.batch_norm = bool(cfg.batch_norm)
        self._h = c_void_p()
        self._lm_table = None  # the NgramLM / GraphLM table tfk_ctc_lm_set / tfk_ctc_graph_set holds (ctc_set_lm)
        self._den_table = None  # the GraphLM table tfk_ctc_den_set holds (ctc_set_den)
        self._state = None
        self._stream = None
        self._cb = None
        self._layer_cb = None
        # Called before anything reads or writes the fp32 PARAMETERS from outside the optimiser (tensor get / set, the
        # layer-wise growth control ops).  The mixed-precision sharded exchange (dataparallel.BucketReducer) keeps the
        # fp32 masters of a span only on the rank that owns it; its hook refuses such an access until the masters have
        # been gathered collectively (DataParallel.gather_parameters) instead of handing out stale values.
        self.param_access_hook = None
        self.on_close = []
        self._raw_inflight = []   # (device tensor, event): inputs adopted in place that the engine may still be reading
        self._raw_pending = None
        if torch_state:
            import torch
            nbytes = c_size_t()
            check(self.lib.tfk_state_bytes(byref(cfg), byref(nbytes)))
            dev = torch.device("cuda", cfg.device)
            self._state = torch.zeros(nbytes.value // 4, dtype=torch.float32, device=dev)
            self._stream = torch.cuda.Stream(device=dev)
            torch.cuda.synchronize(dev)
            check(self.lib.tfk_create_ex(byref(cfg), c_void_p(self._state.data_ptr()), nbytes.value,
                                         c_void_p(self._stream.cuda_stream), byref(self._h)))
        else:
            check(self.lib.tfk_create(byref(cfg), byref(self._h)))

    # ---- lifetime ----
    def _raw_release(self, wait=False):
        """after a call that adopted a device tensor in place: mark the end of its use on the engine stream; drop the
        references whose work has completed (all of them with wait=True)"""
        if self._raw_pending is not None:
            import torch
            raw, ext = self._raw_pending
            ev = torch.cuda.Event()
            ev.record(ext)
            self._raw_inflight.append((raw, ev))
            self._raw_pending = None
        keep = []
        for raw, ev in self._raw_inflight:
            if wait:
                ev.synchronize()
            elif not ev.query():
                keep.append((raw, ev))
        self._raw_inflight = keep

    def close(self):
        if self._h:
            if self._raw_inflight or self._raw_pending:
                self._raw_release(wait=True)
            for fn in self.on_close:
                fn()
            del self.on_close[:]
            check(self.lib.tfk_destroy(self._h))
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- tensors / scalars ----
    def _shape(self, kind, layer):
        if kind == WEIGHTS:
            d_in = self.F if layer == 0 else self.H
            d_out = self.O if layer == self.L else self.H
            return (d_in, d_out)
        if kind == BIASES:
            return (self.O if layer == self.L else self.H,)
        return (self.H,)

    def _param_access(self, slot=SLOT_PARAM):
        if slot == SLOT_PARAM and self.param_access_hook is not None:
            self.param_access_hook()

    def get(self, kind, layer, slot=SLOT_PARAM):
        self._param_access(slot)
        out = np.empty(self._shape(kind, layer), dtype=np.float32)
        check(self.lib.tfk_tensor_get(self._h, kind, slot, layer, out.ctypes.data_as(c_void_p), out.size))
        return out

    def set(self, kind, layer, value, slot=SLOT_PARAM):
        v = _f32(value)
        if v.shape != self._shape(kind, layer):
            raise ValueError("tensor shape %s != %s" % (v.shape, self._shape(kind, layer)))
        self._param_access(slot)
        check(self.lib.tfk_tensor_set(self._h, kind, slot, layer, v.ctypes.data_as(c_void_p), v.size))

    def scalar(self, which):
        v = c_double()
        check(self.lib.tfk_scalar_get(self._h, which, byref(v)))
        return v.value

    def set_scalar(self, which, value):
        check(self.lib.tfk_scalar_set(self._h, which, float(value)))

    @property
    def global_step(self):
        return int(self.scalar(GLOBAL_STEP))

    def init_hidden_weights(self, rng):
        """neuralNetworks/classifiers/layer.py:39-44: hidden W ~ N(0, 1/sqrt(d_in)); everything else
        keeps the engine's defaults (biases 0, output layer 0: dnn.py:67-68)."""
        for l in range(self.L):
            d_in = self.F if l == 0 else self.H
            self.set(WEIGHTS, l, (rng.standard_normal((d_in, self.H)) / np.sqrt(d_in)).astype(np.float32))

    def model_tensors(self):
        """Everything the reference's model saver holds (dnn.py:129): W, b, BN beta + moving stats."""
        out = {}
        for l in range(self.L + 1):
            out["layer%d/weights" % l] = self.get(WEIGHTS, l)
            out["layer%d/biases" % l] = self.get(BIASES, l)
        if self.batch_norm:
            for l in range(self.L):
                out["layer%d/batch_norm/beta" % l] = self.get(BN_BETA, l)
                out["layer%d/batch_norm/moving_mean" % l] = self.get(BN_MOVING_MEAN, l)
                out["layer%d/batch_norm/moving_variance" % l] = self.get(BN_MOVING_VAR, l)
        out["initialisedlayers"] = np.array(int(self.scalar(INITIALISED_LAYERS)), dtype=np.int32)
        return out

    def load_model_tensors(self, tensors):
        for l in range(self.L + 1):
            self.set(WEIGHTS, l, tensors["layer%d/weights" % l])
            self.set(BIASES, l, tensors["layer%d/biases" % l])
        if self.batch_norm:
            for l in range(self.L):
                self.set(BN_BETA, l, tensors["layer%d/batch_norm/beta" % l])
                self.set(BN_MOVING_MEAN, l, tensors["layer%d/batch_norm/moving_mean" % l])
                self.set(BN_MOVING_VAR, l, tensors["layer%d/batch_norm/moving_variance" % l])
        if "initialisedlayers" in tensors:
            self.set_scalar(INITIALISED_LAYERS, int(tensors["initialisedlayers"]))

    # ---- training / evaluation ----
    @staticmethod
    def _host_batch(X, y):
        X = _f32(X)
        y = np.ascontiguousarray(y, dtype=np.int32)
        if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0]:
            raise ValueError("X %s / y %s are not [T, F] / [T]" % (X.shape, y.shape))
        return X, y

    def accumulate(self, X, y, last=False):
        X, y = self._host_batch(X, y)
        check(self.lib.tfk_accumulate(self._h, X.ctypes.data_as(c_void_p), X.shape[1], y.ctypes.data_as(c_void_p),
                                      X.shape[0], _lib.LAST_MICROBATCH if last else 0))

    def accumulate_device(self, x_ptr, ldx, y_ptr, T, last=False):
        """X / y already resident in HBM (raw device pointers)."""
        flags = _lib.DEVICE_PTRS | (_lib.LAST_MICROBATCH if last else 0)
        check(self.lib.tfk_accumulate(self._h, c_void_p(x_ptr), ldx, c_void_p(y_ptr), T, flags))

    # ---- device-side splice: unspliced frames in, spliced in HBM ----
    def _raw_device(self, raw, lens):
        """unspliced frames that already live in HBM (a float32 torch tensor, e.g. FeaturePlan.compute_device's result):
        (pointer, leading dimension, rows, utterance lengths); the engine's stream is ordered behind the tensor's producer"""
        import torch
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if raw.dtype != torch.float32 or raw.dim() != 2 or raw.stride(1) != 1 or int(lens.sum()) != raw.shape[0]:
            raise ValueError("device frames must be a float32 [T, D] tensor with unit column stride whose rows match the "
                             "utterance lengths (sum %d)" % int(lens.sum()))
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(raw.device))
        stream = c_void_p()
        check(self.lib.tfk_stream(self._h, byref(stream)))
        ext = torch.cuda.ExternalStream(stream.value, device=raw.device)
        ext.wait_event(done)
        # Lifetime contract (round-2 advisor finding): the call returns while the splice kernel that reads `raw` is still
        # pending on the ENGINE's stream, which torch's caching allocator knows nothing about -- if the caller dropped the
        # tensor, its block could be handed out again and overwritten under the pending kernel.  The engine therefore keeps
        # a reference until an event recorded behind the consuming work has completed (_raw_release).  (Not
        # Tensor.record_stream: the allocator would later touch a stream that dies with the engine.)
        self._raw_pending = (raw, ext)
        return c_void_p(raw.data_ptr()), int(raw.stride(0)), int(raw.shape[0]), lens

    @staticmethod
    def _raw_batch(raw, lens):
        raw = _f32(raw)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if raw.ndim != 2 or lens.ndim != 1 or int(lens.sum()) != raw.shape[0]:
            raise ValueError("raw %s / utterance lengths (sum %d) do not match" % (raw.shape, int(lens.sum())))
        return raw, lens

    @staticmethod
    def _cmvn_table(cmvn, raw, lens):
        """None or the [U, 2, D] (mean, std) table -> (keep-alive array, pointer)"""
        if cmvn is None:
            return None, c_void_p(None)
        cmvn = np.ascontiguousarray(cmvn, dtype=np.float32)
        if cmvn.shape != (lens.size, 2, raw.shape[1]):
            raise ValueError("cmvn table %s, expected %s" % (cmvn.shape, (lens.size, 2, raw.shape[1])))
        return cmvn, cmvn.ctypes.data_as(c_void_p)

    @contextmanager
    def _raw_args(self, raw, lens, cmvn, flags=0):
        """The unspliced frames of one *_raw call, for the length of the call: `raw` host [T, D] frames or a float32 CUDA
        tensor (TFK_RAW_DEVICE: adopted in place), `lens` frames per utterance, `cmvn` None or the [U, 2, D] table.  Yields
        (pointer, leading dimension, rows, lens, cmvn pointer, flags) and, however the block ends, marks the end of the
        tensor's use (_raw_release)."""
        try:
            if hasattr(raw, "is_cuda") and raw.is_cuda:
                ptr, ld, rows, lens = self._raw_device(raw, lens)
                flags |= _lib.RAW_DEVICE
            else:
                raw, lens = self._raw_batch(raw, lens)
                ptr, ld, rows = raw.ctypes.data_as(c_void_p), raw.shape[1], raw.shape[0]
            cmvn, cmvn_ptr = self._cmvn_table(cmvn, raw, lens)
            yield ptr, ld, rows, lens, cmvn_ptr, flags
        finally:
            self._raw_release()

    def accumulate_raw(self, raw, y, lens, context_width, last=False, cmvn=None):
        """`raw`: host [T, D] frames, or a float32 CUDA tensor (TFK_RAW_DEVICE)"""
        y = np.ascontiguousarray(y, dtype=np.int32)
        with self._raw_args(raw, lens, cmvn, _lib.LAST_MICROBATCH if last else 0) as (ptr, ld, rows, lens, cmvn_ptr, flags):
            if y.shape != (rows,):
                raise ValueError("targets %s do not match %d frames" % (y.shape, rows))
            check(self.lib.tfk_accumulate_raw(self._h, ptr, ld, y.ctypes.data_as(c_void_p), rows,
                                              lens.ctypes.data_as(c_void_p), lens.size, int(context_width), cmvn_ptr, flags))

    # ---- several micro-batches of one optimiser step in one call (stacked pass: include/tfkaldi_hip.h) ----
    def accumulate_stacked(self, X, y, seg_rows, last=False):
        """the micro-batches X[rows_0 + rows_1 + ..., F] back to back, seg_rows frames each: the same result as one
        accumulate per micro-batch, the GEMMs run once over all of them"""
        X, y = self._host_batch(X, y)
        seg = np.ascontiguousarray(seg_rows, dtype=np.int32)
        check(self.lib.tfk_accumulate_stacked(self._h, X.ctypes.data_as(c_void_p), X.shape[1], y.ctypes.data_as(c_void_p),
                                              X.shape[0], seg.ctypes.data_as(c_void_p), seg.size,
                                              _lib.LAST_MICROBATCH if last else 0))

    def accumulate_stacked_device(self, x_ptr, ldx, y_ptr, T, seg_rows, last=False):
        seg = np.ascontiguousarray(seg_rows, dtype=np.int32)
        flags = _lib.DEVICE_PTRS | (_lib.LAST_MICROBATCH if last else 0)
        check(self.lib.tfk_accumulate_stacked(self._h, c_void_p(x_ptr), ldx, c_void_p(y_ptr), T, seg.ctypes.data_as(c_void_p),
                                              seg.size, flags))

    def _raw_targets(self, raw, y, lens, cmvn):
        """host frames, targets and cmvn table of a frame-level *_raw entry that takes no device tensor, checked against
        each other: (raw, y, lens, cmvn table to keep alive over the call, its pointer)"""
        raw, lens = self._raw_batch(raw, lens)
        y = np.ascontiguousarray(y, dtype=np.int32)
        cmvn, cmvn_ptr = self._cmvn_table(cmvn, raw, lens)
        if y.shape != (raw.shape[0],):
            raise ValueError("targets %s do not match %d frames" % (y.shape, raw.shape[0]))
        return raw, y, lens, cmvn, cmvn_ptr

    def _stacked_raw(self, fn, raw, y, lens, context_width, seg_utts, cmvn, flags):
        seg = np.ascontiguousarray(seg_utts, dtype=np.int32)  # (in front of the cmvn and target checks, as it always was)
        raw, y, lens, cmvn, cmvn_ptr = self._raw_targets(raw, y, lens, cmvn)
        check(fn(self._h, _ptr(raw), raw.shape[1], _ptr(y), raw.shape[0], _ptr(lens), lens.size, int(context_width), cmvn_ptr,
                 _ptr(seg), seg.size, flags))

    def accumulate_stacked_raw(self, raw, y, lens, context_width, seg_utts, last=False, cmvn=None):
        """unspliced frames of all utterances back to back, seg_utts utterances per micro-batch (CMVN + splice on the device)"""
        self._stacked_raw(self.lib.tfk_accumulate_stacked_raw, raw, y, lens, context_width, seg_utts, cmvn,
                          _lib.LAST_MICROBATCH if last else 0)

    def eval_accumulate_stacked(self, X, y, seg_rows):
        """Trainer.evaluate's micro-batches X[rows_0 + rows_1 + ..., F] back to back in ONE call: rows are independent in
        evaluation mode, so the engine runs one pass of the GEMMs over all of them (tfk_eval_accumulate_stacked)"""
        X, y = self._host_batch(X, y)
        seg = np.ascontiguousarray(seg_rows, dtype=np.int32)
        check(self.lib.tfk_eval_accumulate_stacked(self._h, X.ctypes.data_as(c_void_p), X.shape[1], y.ctypes.data_as(c_void_p),
                                                   X.shape[0], seg.ctypes.data_as(c_void_p), seg.size, 0))

    def eval_accumulate_stacked_raw(self, raw, y, lens, context_width, seg_utts, cmvn=None):
        """the same from unspliced frames (CMVN + splice on the device), seg_utts utterances per micro-batch"""
        self._stacked_raw(self.lib.tfk_eval_accumulate_stacked_raw, raw, y, lens, context_width, seg_utts, cmvn, 0)

    def eval_accumulate_raw(self, raw, y, lens, context_width, cmvn=None):
        raw, y, lens, cmvn, cmvn_ptr = self._raw_targets(raw, y, lens, cmvn)
        check(self.lib.tfk_eval_accumulate_raw(self._h, _ptr(raw), raw.shape[1], _ptr(y), raw.shape[0], _ptr(lens), lens.size,
                                               int(context_width), cmvn_ptr, 0))

    def _out_buffer(self, rows):
        """[rows, O] result array; in pinned host memory (torch's caching pinned allocator) so that the engine can
        DMA straight into it -- the decode path moves 8 KB per frame back to the host"""
        if rows * self.O >= 1 << 16:
            try:
                import torch
                return torch.empty((rows, self.O), dtype=torch.float32, pin_memory=True).numpy()
            except Exception:  # noqa: BLE001  (no torch / no pinned memory: plain pageable memory works as well)
                pass
        return np.empty((rows, self.O), dtype=np.float32)

    def posteriors_raw(self, raw, lens, context_width, log_div_prior=False, raw_logits=False, cmvn=None):
        """`raw`: host [T, D] frames, or a float32 CUDA tensor (TFK_RAW_DEVICE: features that never left HBM)"""
        flags = (_lib.LOG_DIV_PRIOR if log_div_prior else 0) | (_lib.RAW_LOGITS if raw_logits else 0)
        with self._raw_args(raw, lens, cmvn, flags) as (ptr, ld, rows, lens, cmvn_ptr, flags):
            out = self._out_buffer(rows)
            check(self.lib.tfk_posteriors_raw(self._h, ptr, ld, rows, lens.ctypes.data_as(c_void_p), lens.size,
                                              int(context_width), cmvn_ptr, out.ctypes.data_as(c_void_p), self.O, flags))
        return out

    # ---- the forward-only CTC entries (greedy, beam, align; plain and raw): one call shape ----
    @staticmethod
    def _refs(utt_lens, labels, label_lens, optional, what):
        """utterance lengths and label sequences (labels back to back, label_lens per utterance) as int32 vectors;
        optional: labels and label_lens may both be None (no references)"""
        utt_lens = np.ascontiguousarray(utt_lens, dtype=np.int32).reshape(-1)
        if optional and (labels is None) != (label_lens is None):
            raise ValueError("labels and label_lens go together")
        if optional and labels is None:
            return utt_lens, None, None
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        label_lens = np.ascontiguousarray(label_lens, dtype=np.int32).reshape(-1)
        if label_lens.size != utt_lens.size or int(label_lens.sum()) != labels.size:
            raise ValueError("%s: %d label counts (sum %d) for %d utterances and %d labels"
                             % (what, label_lens.size, int(label_lens.sum()), utt_lens.size, labels.size))
        return utt_lens, labels, label_lens

    def _decode(self, fn, frames, utt_lens, refs, outputs, result, extra=(), raw=None, own_flags=0):
        """One call of a forward-only CTC entry `fn`: tfk_ctc_X on spliced frames [sum(utt_lens), F], or tfk_ctc_X_raw on
        unspliced ones with raw = (context_width, cmvn).  refs: (labels, label_lens) after _refs.  outputs(rows, U) makes
        the arrays the entry fills, in the order of its signature (None: a NULL pointer); with rows == 0 -- only zero-frame
        utterances, the engine is not called -- it fills them itself.  extra: the entry's own arguments behind the common ones,
        own_flags: its own flag bits.  Returns result(utt_lens, *arrays)."""
        def run(ptr, ld, rows, lens, raw_args, flags):
            outs = outputs(rows, lens.size)
            if rows:
                check(fn(self._h, ptr, ld, rows, _ptr(lens), lens.size, *raw_args, *extra, _ptr(refs[0]), _ptr(refs[1]),
                         *[_ptr(o) for o in outs], flags | own_flags))
            return result(lens, *outs)
        if raw is None:
            X = _f32(frames)
            if int(utt_lens.sum()) != X.shape[0]:
                raise ValueError("frames %s / utterance lengths (sum %d) do not match" % (X.shape, int(utt_lens.sum())))
            return run(_ptr(X), X.shape[1], X.shape[0], utt_lens, (), 0)
        with self._raw_args(frames, utt_lens, raw[1]) as (ptr, ld, rows, lens, cmvn_ptr, flags):
            return run(ptr, ld, rows, lens, (int(raw[0]), cmvn_ptr), flags)

    # ---- best-path CTC decoding: tf.nn.ctc_greedy_decoder(merge_repeated=True) + tf.edit_distance(normalize=False) ----
    def _greedy(self, fn, frames, utt_lens, labels, label_lens, raw=None):
        utt_lens, labels, label_lens = self._refs(utt_lens, labels, label_lens, True, "references")

        def outputs(rows, U):  # (no frames: empty hypotheses, the reference lengths as distances)
            edits = None if labels is None else (np.empty(U, dtype=np.int32) if rows else label_lens.copy())
            return np.empty(rows, dtype=np.int32), np.zeros(U, dtype=np.int32), edits

        def result(lens, hyp, hyp_len, edits):
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            return [hyp[s:s + n].copy() for s, n in zip(starts, hyp_len)], edits
        return self._decode(fn, frames, utt_lens, (labels, label_lens), outputs, result, raw=raw)

    def ctc_greedy(self, X, utt_lens, labels=None, label_lens=None):
        """Best-path decoding of the utterances X [sum(utt_lens), F] (tfk_ctc_greedy): per frame the largest logit, repeats
        merged, blanks (the last class) removed.  With references (labels back to back, label_lens per utterance) also the
        Levenshtein distance of every hypothesis to its reference.  Returns (list of int32 label arrays, int32 [U] edit
        distances or None)."""
        return self._greedy(self.lib.tfk_ctc_greedy, X, utt_lens, labels, label_lens)

    def ctc_greedy_raw(self, raw, utt_lens, context_width, cmvn=None, labels=None, label_lens=None):
        """ctc_greedy on UNSPLICED frames (CMVN + splice on the device, as posteriors_raw); `raw` may be a float32 CUDA
        tensor (TFK_RAW_DEVICE)"""
        return self._greedy(self.lib.tfk_ctc_greedy_raw, raw, utt_lens, labels, label_lens, raw=(context_width, cmvn))

    # ---- CTC prefix beam search: tf.nn.ctc_beam_search_decoder(merge_repeated=False), N best with log-probabilities ----
    def _beam(self, fn, frames, utt_lens, beam_width, top_paths, labels, label_lens, raw=None, label_topk=None):
        beam_width, top_paths = int(beam_width), int(top_paths)
        if not 1 <= top_paths <= beam_width:
            raise ValueError("top_paths %d outside [1, beam_width = %d]" % (top_paths, beam_width))
        utt_lens, labels, label_lens = self._refs(utt_lens, labels, label_lens, True, "references")

        def outputs(rows, U):  # (no frames: the empty hypothesis with score 0, the other paths empty with score -inf)
            score = np.full((top_paths, U), -np.inf, dtype=np.float32)
            score[0] = 0.0
            edits = None if labels is None else (np.empty(U, dtype=np.int32) if rows else label_lens.copy())
            return np.empty((top_paths, rows), dtype=np.int32), np.zeros((top_paths, U), dtype=np.int32), score, edits

        def result(lens, hyp, hyp_len, score, edits):
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            hyps = [[hyp[n, s:s + hyp_len[n, u]].copy() for n in range(top_paths)] for u, s in enumerate(starts)]
            return hyps, np.ascontiguousarray(score.T), edits
        if label_topk is not None:  # the pruned entry without a model: its acoustic-score output is not asked for (NULL)
            def outputs_topk(rows, U):
                hyp, hyp_len, score, edits = outputs(rows, U)
                return hyp, hyp_len, score, None, edits

            def result_topk(lens, hyp, hyp_len, score, _, edits):
                return result(lens, hyp, hyp_len, score, edits)
            fn = self.lib.tfk_ctc_beam_topk if raw is None else self.lib.tfk_ctc_beam_topk_raw
            return self._decode(fn, frames, utt_lens, (labels, label_lens), outputs_topk, result_topk,
                                (beam_width, top_paths, int(label_topk), c_float(0.0), c_float(0.0)), raw)
        return self._decode(fn, frames, utt_lens, (labels, label_lens), outputs, result, (beam_width, top_paths), raw)

    def ctc_beam(self, X, utt_lens, beam_width=100, top_paths=1, labels=None, label_lens=None, label_topk=None):
        """Prefix beam search over the utterances X [sum(utt_lens), F] (tfk_ctc_beam; the algorithm is stated in
        include/tfkaldi_hip.h): the `top_paths` most probable label sequences of every utterance among those that stay in a
        beam of `beam_width`, best first, with their natural-log probabilities.  Returns (hyps, scores, edits): hyps[u][n]
        int32 label arrays, scores float32 [U, top_paths] (-inf where fewer prefixes survived), edits int32 [U] = Levenshtein
        distance of the BEST path to the reference (labels back to back, label_lens per utterance) or None.
        label_topk: None is that search (at most 64 outputs); an int in [1, 63] is the search with per-frame label pruning
        (tfk_ctc_beam_topk), where only the frame's label_topk most probable labels may start a new label: any output_dim up
        to 65536, and less work per frame below 64."""
        return self._beam(self.lib.tfk_ctc_beam, X, utt_lens, beam_width, top_paths, labels, label_lens,
                          label_topk=label_topk)

    def ctc_beam_raw(self, raw, utt_lens, context_width, cmvn=None, beam_width=100, top_paths=1, labels=None,
                     label_lens=None, label_topk=None):
        """ctc_beam on UNSPLICED frames (CMVN + splice on the device, as posteriors_raw); `raw` may be a float32 CUDA
        tensor (TFK_RAW_DEVICE)"""
        return self._beam(self.lib.tfk_ctc_beam_raw, raw, utt_lens, beam_width, top_paths, labels, label_lens,
                          raw=(context_width, cmvn), label_topk=label_topk)

    # ---- the same search ranked with a language model over the labels: a character n-gram (neuralNetworks/ctc_lm.NgramLM)
    # or a deterministic finite-state grammar, which also forbids what it does not accept (ctc_lm.GraphLM) ----
    def ctc_set_lm(self, lm):
        """Make `lm` (an NgramLM or a GraphLM, or None to drop it) the engine's language model (tfk_ctc_lm_set /
        tfk_ctc_graph_set: the tables are copied to the device; either replaces the other).  Nothing is uploaded when the
        same table object is already set."""
        if lm is None:
            if self._lm_table is not None:
                check(self.lib.tfk_ctc_lm_set(self._h, c_void_p(None), 0))
                self._lm_table = None
            return
        lm.check(self.O)
        if self._lm_table is lm.table:
            return
        self._lm_table = None
        if getattr(lm, "next", None) is not None:
            check(self.lib.tfk_ctc_graph_set(self._h, _ptr(lm.table), _ptr(lm.next), lm.num_states, lm.start))
        else:
            check(self.lib.tfk_ctc_lm_set(self._h, _ptr(lm.table), lm.order))
        self._lm_table = lm.table

    def _beam_lm(self, fn, frames, utt_lens, lm, beam_width, top_paths, labels, label_lens, raw=None, label_topk=None):
        beam_width, top_paths = int(beam_width), int(top_paths)
        if not 1 <= top_paths <= beam_width:
            raise ValueError("top_paths %d outside [1, beam_width = %d]" % (top_paths, beam_width))
        utt_lens, labels, label_lens = self._refs(utt_lens, labels, label_lens, True, "references")
        self.ctc_set_lm(lm)

        def outputs(rows, U):  # (no frames: the empty hypothesis, acoustic score 0, combined 0 or the model's end term)
            score = np.full((top_paths, U), -np.inf, dtype=np.float32)
            am = score.copy()
            am[0] = 0.0
            end = lm.table[lm.start, -1]  # (a graph's start state that is not final: -inf whatever the weight is)
            score[0] = (end if end == -np.inf else np.float32(lm.weight) * end) if lm.end_of_sequence else 0.0
            edits = None if labels is None else (np.empty(U, dtype=np.int32) if rows else label_lens.copy())
            return np.empty((top_paths, rows), dtype=np.int32), np.zeros((top_paths, U), dtype=np.int32), score, am, edits

        def result(lens, hyp, hyp_len, score, am, edits):
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            hyps = [[hyp[n, s:s + hyp_len[n, u]].copy() for n in range(top_paths)] for u, s in enumerate(starts)]
            return hyps, np.ascontiguousarray(score.T), np.ascontiguousarray(am.T), edits
        own = _lib.CTC_LM_EOS if lm.end_of_sequence else 0
        if label_topk is not None:  # the pruned entry, ranked by the model
            fn = self.lib.tfk_ctc_beam_topk if raw is None else self.lib.tfk_ctc_beam_topk_raw
            return self._decode(fn, frames, utt_lens, (labels, label_lens), outputs, result,
                                (beam_width, top_paths, int(label_topk), c_float(lm.weight), c_float(lm.label_bonus)), raw,
                                own | _lib.CTC_LM)
        return self._decode(fn, frames, utt_lens, (labels, label_lens), outputs, result,
                            (beam_width, top_paths, c_float(lm.weight), c_float(lm.label_bonus)), raw, own)

    def ctc_beam_lm(self, X, utt_lens, lm, beam_width=100, top_paths=1, labels=None, label_lens=None, label_topk=None):
        """ctc_beam with prefixes ranked by acoustic score + language-model score (tfk_ctc_beam_lm; the search is stated in
        include/tfkaldi_hip.h).  lm: an NgramLM or a GraphLM over this model's labels (a GraphLM also restricts the search to
        the label sequences it accepts: tfk_ctc_graph_set) -- its table is set on the engine if it is not already, its weight, label bonus and end-of-sequence switch go with the call.  Returns (hyps, scores, am_scores,
        edits): as ctc_beam, scores the COMBINED values the paths are ordered by, am_scores float32 [U, top_paths] their
        acoustic parts; edits of the best path by combined score.  label_topk: as ctc_beam."""
        return self._beam_lm(self.lib.tfk_ctc_beam_lm, X, utt_lens, lm, beam_width, top_paths, labels, label_lens,
                             label_topk=label_topk)

    def ctc_beam_lm_raw(self, raw, utt_lens, context_width, lm, cmvn=None, beam_width=100, top_paths=1, labels=None,
                        label_lens=None, label_topk=None):
        """ctc_beam_lm on UNSPLICED frames (CMVN + splice on the device, as posteriors_raw); `raw` may be a float32 CUDA
        tensor (TFK_RAW_DEVICE)"""
        return self._beam_lm(self.lib.tfk_ctc_beam_lm_raw, raw, utt_lens, lm, beam_width, top_paths, labels, label_lens,
                             raw=(context_width, cmvn), label_topk=label_topk)

    # ---- streaming decode: the beam search resumable across chunks (tfk_ctc_stream_*) ----
    def ctc_stream_open(self, lanes, beam_width, max_frames, label_topk=None):
        """A decode stream of `lanes` independent sessions on this engine (the contract is stated in include/tfkaldi_hip.h at
        tfk_ctc_stream_create): each lane decodes at most max_frames frames between two resets.  label_topk: as ctc_beam.
        Returns a CtcStreamHandle."""
        return CtcStreamHandle(self, lanes, beam_width, max_frames, label_topk)

    # ---- CTC forced alignment: the Viterbi path of the known label sequence, per frame the label POSITION it emits ----
    def _align(self, fn, frames, utt_lens, labels, label_lens, raw=None):
        utt_lens, labels, label_lens = self._refs(utt_lens, labels, label_lens, False, "alignment")

        def outputs(rows, U):  # (no frames: the empty alignment with score 0 where there is nothing to emit, else no path)
            score = np.empty(U, dtype=np.float32) if rows else np.where(label_lens == 0, 0.0, -np.inf).astype(np.float32)
            return np.empty(rows, dtype=np.int32), score

        def result(lens, ali, score):
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            return [ali[s:s + n].copy() if sc > -np.inf else None for s, n, sc in zip(starts, lens, score)], score
        return self._decode(fn, frames, utt_lens, (labels, label_lens), outputs, result, raw=raw)

    def ctc_align(self, X, utt_lens, labels, label_lens):
        """Forced alignment of the utterances X [sum(utt_lens), F] to their label sequences (tfk_ctc_align; the algorithm and
        its tie rule are stated in include/tfkaldi_hip.h): the most probable CTC path of every utterance.  labels back to
        back, label_lens per utterance, as accumulate_ctc.  Returns (alis, scores): alis[u] int32 [utt_lens[u]], per frame
        the POSITION in the utterance's label sequence of the label the frame emits, -1 for a blank frame -- None for an
        utterance too short for its labels; scores float32 [U], the natural-log probability of the path (-inf for None)."""
        return self._align(self.lib.tfk_ctc_align, X, utt_lens, labels, label_lens)

    def ctc_align_raw(self, raw, utt_lens, context_width, labels, label_lens, cmvn=None):
        """ctc_align on UNSPLICED frames (CMVN + splice on the device, as posteriors_raw); `raw` may be a float32 CUDA
        tensor (TFK_RAW_DEVICE)"""
        return self._align(self.lib.tfk_ctc_align_raw, raw, utt_lens, labels, label_lens, raw=(context_width, cmvn))

    # ---- CTC N-best rescoring: the exact log p(labels | x) of named hypotheses, and their label errors ----
    def _score(self, fn, frames, utt_lens, hyp_counts, labels, label_lens, ref_labels, ref_lens, raw=None):
        utt_lens, ref_labels, ref_lens = self._refs(utt_lens, ref_labels, ref_lens, True, "references")
        hyp_counts = np.ascontiguousarray(hyp_counts, dtype=np.int32).reshape(-1)
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        label_lens = np.ascontiguousarray(label_lens, dtype=np.int32).reshape(-1)
        if hyp_counts.size != utt_lens.size or np.any(hyp_counts < 0):
            raise ValueError("hypotheses: %d counts (smallest %d) for %d utterances"
                             % (hyp_counts.size, int(hyp_counts.min()) if hyp_counts.size else 0, utt_lens.size))
        P = int(hyp_counts.sum(dtype=np.int64))
        if label_lens.size != P or np.any(label_lens < 0) or int(label_lens.sum(dtype=np.int64)) != labels.size:
            raise ValueError("hypotheses: %d label counts (sum %d) for %d hypotheses and %d labels"
                             % (label_lens.size, int(label_lens.sum(dtype=np.int64)), P, labels.size))
        cuts = np.cumsum(hyp_counts, dtype=np.int64)[:-1]

        def outputs(rows, U):  # (no frames: only the empty labelling has an alignment, the empty one)
            if rows:
                return np.empty(P, dtype=np.float32), None if ref_labels is None else np.empty(P, dtype=np.int32)
            score = np.where(label_lens == 0, 0.0, -np.inf).astype(np.float32)
            if ref_labels is None:
                return score, None
            hyps = np.split(labels, np.cumsum(label_lens, dtype=np.int64)[:-1]) if P else []
            refs = np.split(ref_labels, np.cumsum(ref_lens, dtype=np.int64)[:-1])
            utt = np.repeat(np.arange(U), hyp_counts)
            return score, np.array([_levenshtein(h, refs[u]) for h, u in zip(hyps, utt)], dtype=np.int32)

        def result(lens, score, edits):
            return np.split(score, cuts), None if edits is None else np.split(edits, cuts)
        return self._decode(fn, frames, utt_lens, (ref_labels, ref_lens), outputs, result, (_ptr(hyp_counts), _ptr(labels),
                                                                                           _ptr(label_lens)), raw)

    def ctc_score(self, X, utt_lens, hyp_counts, labels, label_lens, ref_labels=None, ref_lens=None):
        """N-best rescoring over the utterances X [sum(utt_lens), F] (tfk_ctc_score; the contract is stated in
        include/tfkaldi_hip.h): for every (utterance, hypothesis) pair the EXACT natural-log probability log p(labels | x) --
        the sum over all CTC alignments, minus the utterance's CTC loss with those labels -- where a beam search reports only
        the alignments that survived its pruning.  hyp_counts[u] hypotheses per utterance (0 is allowed); labels back to back
        in pair order (by utterance, then by hypothesis), label_lens per pair, at most 511 labels each.  With references
        (ref_labels back to back, ref_lens per UTTERANCE) also the Levenshtein distance of every hypothesis to its
        utterance's reference.  Returns (scores, edits): per utterance a float32 array of its hypotheses' scores (-inf for
        one its utterance is too short for) and an int32 array of their distances (edits None without references)."""
        return self._score(self.lib.tfk_ctc_score, X, utt_lens, hyp_counts, labels, label_lens, ref_labels, ref_lens)

    def ctc_score_raw(self, raw, utt_lens, context_width, hyp_counts, labels, label_lens, ref_labels=None, ref_lens=None,
                      cmvn=None):
        """ctc_score on UNSPLICED frames (CMVN + splice on the device, as posteriors_raw); `raw` may be a float32 CUDA
        tensor (TFK_RAW_DEVICE)"""
        return self._score(self.lib.tfk_ctc_score_raw, raw, utt_lens, hyp_counts, labels, label_lens, ref_labels, ref_lens,
                           raw=(context_width, cmvn))

    # ---- CTC alignment with wildcard gaps and keyword spotting: gap states that may emit the frame's best class ----
    @staticmethod
    def _wild(wild, label_lens, what):
        """the flags of tfk_ctc_align_wild / tfk_ctc_spot: None, or uint8 with label_lens[i] + 1 values per sequence"""
        if wild is None:
            return None
        wild = np.ascontiguousarray(wild).reshape(-1)
        if wild.dtype == np.bool_:
            wild = wild.astype(np.uint8)
        if wild.dtype != np.uint8:
            raise ValueError("%s: wild is %s, expected uint8 or bool" % (what, wild.dtype))
        need = int(label_lens.sum(dtype=np.int64)) + label_lens.size
        if wild.size != need:
            raise ValueError("%s: %d gap flags for %d sequences of %d labels (one more than labels each: %d)"
                             % (what, wild.size, label_lens.size, need - label_lens.size, need))
        return wild

    def _align_wild(self, fn, frames, utt_lens, labels, label_lens, wild, raw=None):
        utt_lens, labels, label_lens = self._refs(utt_lens, labels, label_lens, False, "alignment")
        wild = self._wild(wild, label_lens, "alignment")

        def outputs(rows, U):  # (wild rides in front: an array the entry reads.  No frames: as _align, and free = 0)
            score = np.empty(U, dtype=np.float32) if rows else np.where(label_lens == 0, 0.0, -np.inf).astype(np.float32)
            return wild, np.empty(rows, dtype=np.int32), score, np.zeros(U, dtype=np.float32)

        def result(lens, _, ali, score, free):
            starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            return [ali[s:s + n].copy() if sc > -np.inf else None for s, n, sc in zip(starts, lens, score)], score, free
        return self._decode(fn, frames, utt_lens, (labels, label_lens), outputs, result, raw=raw)

    def ctc_align_wild(self, X, utt_lens, labels, label_lens, wild=None):
        """ctc_align with WILDCARD GAPS (tfk_ctc_align_wild; the contract is stated in include/tfkaldi_hip.h): `wild` holds
        label_lens[u] + 1 flags per utterance, back to back (uint8 or bool; None: none set) -- flag g of an utterance lets
        the gap before label g (gap S: after the last label) emit the frame's best class instead of the blank, so that
        stretch may hold anything.  Returns (alis, scores, free): as ctc_align (-1 for a frame in any gap), and free float32
        [U], the log-probability of the unconstrained best path; scores <= free, and scores - free is what the pattern costs."""
        return self._align_wild(self.lib.tfk_ctc_align_wild, X, utt_lens, labels, label_lens, wild)

    def ctc_align_wild_raw(self, raw, utt_lens, context_width, labels, label_lens, wild=None, cmvn=None):
        """ctc_align_wild on UNSPLICED frames (CMVN + splice on the device, as posteriors_raw); `raw` may be a float32 CUDA
        tensor (TFK_RAW_DEVICE)"""
        return self._align_wild(self.lib.tfk_ctc_align_wild_raw, raw, utt_lens, labels, label_lens, wild,
                                raw=(context_width, cmvn))

    def _spot(self, fn, frames, utt_lens, pat_counts, labels, label_lens, wild, raw=None):
        utt_lens = self._refs(utt_lens, None, None, True, "patterns")[0]
        pat_counts = np.ascontiguousarray(pat_counts, dtype=np.int32).reshape(-1)
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        label_lens = np.ascontiguousarray(label_lens, dtype=np.int32).reshape(-1)
        if pat_counts.size != utt_lens.size or np.any(pat_counts < 0):
            raise ValueError("patterns: %d counts (smallest %d) for %d utterances"
                             % (pat_counts.size, int(pat_counts.min()) if pat_counts.size else 0, utt_lens.size))
        P = int(pat_counts.sum(dtype=np.int64))
        if label_lens.size != P or np.any(label_lens < 0) or int(label_lens.sum(dtype=np.int64)) != labels.size:
            raise ValueError("patterns: %d label counts (sum %d) for %d pairs and %d labels"
                             % (label_lens.size, int(label_lens.sum(dtype=np.int64)), P, labels.size))
        wild = self._wild(wild, label_lens, "patterns")
        cuts = np.cumsum(pat_counts, dtype=np.int64)[:-1]

        def outputs(rows, U):  # (no frames: only the empty pattern has a path, the empty one)
            if rows:
                return (wild, np.empty(P, dtype=np.float32), np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32),
                        np.empty(U, dtype=np.float32))
            span = np.where(label_lens == 0, 0, -1).astype(np.int32)
            return (wild, np.where(label_lens == 0, 0.0, -np.inf).astype(np.float32), span, span.copy(),
                    np.zeros(U, dtype=np.float32))

        def result(lens, _, score, start, end, free):
            return np.split(score, cuts), np.split(start, cuts), np.split(end, cuts), free
        return self._decode(fn, frames, utt_lens, (labels, label_lens), outputs, result, (_ptr(pat_counts),), raw)

    def ctc_spot(self, X, utt_lens, pat_counts, labels, label_lens, wild=None):
        """Keyword spotting over the utterances X [sum(utt_lens), F] (tfk_ctc_spot; the contract is stated in
        include/tfkaldi_hip.h): pat_counts[u] patterns per utterance (0 is allowed), labels back to back in pair order (by
        utterance, then by pattern), label_lens per pair, at most 511 labels each; `wild` label_lens[p] + 1 flags per PAIR, as
        ctc_align_wild takes them per utterance.  Returns (scores, starts, ends, free): per utterance a float32 array of its
        patterns' scores and int32 arrays of the first frame that emits a label and one past the last -- for every pair what
        ctc_align_wild gives for that utterance and pattern (-inf, -1, -1 without a path; 0, 0 for an empty pattern) -- and
        free float32 [U]."""
        return self._spot(self.lib.tfk_ctc_spot, X, utt_lens, pat_counts, labels, label_lens, wild)

    def ctc_spot_raw(self, raw, utt_lens, context_width, pat_counts, labels, label_lens, wild=None, cmvn=None):
        """ctc_spot on UNSPLICED frames (CMVN + splice on the device, as posteriors_raw); `raw` may be a float32 CUDA
        tensor (TFK_RAW_DEVICE)"""
        return self._spot(self.lib.tfk_ctc_spot_raw, raw, utt_lens, pat_counts, labels, label_lens, wild,
                          raw=(context_width, cmvn))

    # ---- CTC loss: frames [T, F] of U utterances + their label sequences ----
    def _ctc_args(self, X, utt_lens, labels, label_lens):
        X = _f32(X)
        utt_lens = np.ascontiguousarray(utt_lens, dtype=np.int32)
        label_lens = np.ascontiguousarray(label_lens, dtype=np.int32)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if int(utt_lens.sum()) != X.shape[0] or int(label_lens.sum()) != labels.size or utt_lens.size != label_lens.size:
            raise ValueError("CTC micro-batch: frames %s / utterance lengths / labels do not match" % (X.shape,))
        return X, utt_lens, labels, label_lens

    def _accumulate_ctc(self, stem, X, utt_lens, labels, label_lens, own=(), last=False, train=True, raw=None):
        """The C call of every CTC training entry, tfk_[eval_]accumulate_ctc<stem>[_raw]: stem "", "_wild", "_mwer" or
        "_mmi"; X, utt_lens, labels, label_lens after _ctc_args; own: the criterion's own arguments behind the label counts,
        validated, in the order of its signature -- arrays (None: a NULL pointer) and floats.  train=False is the
        evaluation-mode entry, which never ends a step; raw = (context_width, cmvn): X holds UNSPLICED frames."""
        name = "tfk_%saccumulate_ctc%s%s" % ("" if train else "eval_", stem, "" if raw is None else "_raw")
        splice = ()
        if raw is not None:
            cmvn, cmvn_ptr = self._cmvn_table(raw[1], X, utt_lens)  # (cmvn: the array, alive for the length of the call)
            splice = (int(raw[0]), cmvn_ptr)
        check(getattr(self.lib, name)(self._h, _ptr(X), X.shape[1], X.shape[0], _ptr(utt_lens), utt_lens.size, *splice,
                                      _ptr(labels), _ptr(label_lens),
                                      *[_ptr(a) if a is None or isinstance(a, np.ndarray) else a for a in own],
                                      _lib.LAST_MICROBATCH if (last and train) else 0))

    def accumulate_ctc_raw(self, raw, utt_lens, context_width, labels, label_lens, last=False, cmvn=None, train=True):
        """CTC micro-batch from UNSPLICED frames: CMVN + splice on the device (as accumulate_raw)"""
        self._accumulate_ctc("", *self._ctc_args(raw, utt_lens, labels, label_lens), last=last, train=train,
                             raw=(context_width, cmvn))

    def accumulate_ctc(self, X, utt_lens, labels, label_lens, last=False):
        self._accumulate_ctc("", *self._ctc_args(X, utt_lens, labels, label_lens), last=last)

    def eval_accumulate_ctc(self, X, utt_lens, labels, label_lens):
        self._accumulate_ctc("", *self._ctc_args(X, utt_lens, labels, label_lens), train=False)

    # ---- expected label errors over an N-best list (MWER) on top of ctc_weight x the CTC loss ----
    @staticmethod
    def _mwer_args(utt_lens, hyp_counts, hyp_labels, hyp_lens, ctc_weight):
        hyp_counts = np.ascontiguousarray(hyp_counts, dtype=np.int32).reshape(-1)
        hyp_labels = np.ascontiguousarray(hyp_labels, dtype=np.int32).reshape(-1)
        hyp_lens = np.ascontiguousarray(hyp_lens, dtype=np.int32).reshape(-1)
        if hyp_counts.size != utt_lens.size or np.any(hyp_counts < 0):
            raise ValueError("hypotheses: %d counts (smallest %d) for %d utterances"
                             % (hyp_counts.size, int(hyp_counts.min()) if hyp_counts.size else 0, utt_lens.size))
        P = int(hyp_counts.sum(dtype=np.int64))
        if hyp_lens.size != P or np.any(hyp_lens < 0) or int(hyp_lens.sum(dtype=np.int64)) != hyp_labels.size:
            raise ValueError("hypotheses: %d label counts (sum %d) for %d hypotheses and %d labels"
                             % (hyp_lens.size, int(hyp_lens.sum(dtype=np.int64)), P, hyp_labels.size))
        return hyp_counts, hyp_labels, hyp_lens, _finite_nonneg("ctc_weight", ctc_weight)

    def accumulate_ctc_mwer(self, X, utt_lens, labels, label_lens, hyp_counts, hyp_labels, hyp_lens, ctc_weight=0.0,
                            last=False, train=True):
        """One micro-batch of the MWER criterion (tfk_accumulate_ctc_mwer; the contract is stated in include/tfkaldi_hip.h):
        the expected number of label errors over the utterances' hypothesis lists, on the train-mode logits of this pass,
        plus ctc_weight x the CTC loss of the references.  X, utt_lens, labels (the references), label_lens as
        accumulate_ctc; hyp_counts[u] hypotheses per utterance (0 allowed), hyp_labels back to back in pair order, hyp_lens
        per pair, as ctc_score takes them (neuralNetworks/ctc_mwer.pair_tables builds the three from lists).  The step's
        average (apply) is expected label errors per reference label + ctc_weight x CTC loss per label.
        train=False: evaluation-mode forward, loss only."""
        args = self._ctc_args(X, utt_lens, labels, label_lens)
        self._accumulate_ctc("_mwer", *args, self._mwer_args(args[1], hyp_counts, hyp_labels, hyp_lens, ctc_weight), last, train)

    def accumulate_ctc_mwer_raw(self, raw, utt_lens, context_width, labels, label_lens, hyp_counts, hyp_labels, hyp_lens,
                                ctc_weight=0.0, last=False, cmvn=None, train=True):
        """accumulate_ctc_mwer from UNSPLICED frames: CMVN + splice on the device (as accumulate_ctc_raw)"""
        args = self._ctc_args(raw, utt_lens, labels, label_lens)
        self._accumulate_ctc("_mwer", *args, self._mwer_args(args[1], hyp_counts, hyp_labels, hyp_lens, ctc_weight), last, train,
                             (context_width, cmvn))

    # ---- MMI against a denominator graph (CTC-CRF): the exact sum over every label sequence a grammar accepts ----
    def ctc_set_den(self, graph):
        """Make `graph` (a neuralNetworks/ctc_lm.GraphLM, or None to drop it) the engine's DENOMINATOR graph
        (tfk_ctc_den_set): a model of its own beside the decoder's (ctc_set_lm); its final weights are always read, its
        weight / label_bonus / end_of_sequence settings are not (the scale travels with accumulate_ctc_mmi).  Nothing is
        compiled or uploaded when the same table object is already set.  A denominator from transcripts is
        GraphLM.from_ngram(NgramLM.from_label_sequences(...)); graph.composed_states is the N the device limits to 65536, and
        ctc_den_info() says where the sweeps of the graph in force keep their data."""
        if graph is None:
            if self._den_table is not None:
                check(self.lib.tfk_ctc_den_set(self._h, c_void_p(None), c_void_p(None), 0, 0))
                self._den_table = None
            return
        graph.check(self.O)
        if self._den_table is graph.table:
            return
        # (a refused call leaves the old model in force on the device: _den_table keeps saying so)
        check(self.lib.tfk_ctc_den_set(self._h, _ptr(graph.table), _ptr(graph.next), graph.num_states, graph.start))
        self._den_table = graph.table

    def ctc_den_info(self):
        """what the compile of the denominator graph in force found (tfk_ctc_den_info): a dict of num_states, num_arcs,
        num_groups, composed_states and residence -- "global", "lds" (the vector and the sums in LDS) or "lds+tables"""
        from ctypes import c_int32
        S, A, K, where = c_int32(), c_int32(), c_int32(), c_int32()
        check(self.lib.tfk_ctc_den_info(self._h, byref(S), byref(A), byref(K), byref(where)))
        return {"num_states": S.value, "num_arcs": A.value, "num_groups": K.value, "composed_states": S.value + A.value,
                "residence": ("global", "lds", "lds+tables")[where.value]}

    def accumulate_ctc_mmi(self, X, utt_lens, labels, label_lens, lm_scale=1.0, ctc_weight=0.0, last=False, train=True):
        """One micro-batch of the MMI criterion (tfk_accumulate_ctc_mmi; the contract is stated in include/tfkaldi_hip.h):
        -(log p_ctc(reference) + lm_scale G(reference)) + log Z, Z the exact sum over every label sequence the denominator
        graph of ctc_set_den accepts, plus ctc_weight x the CTC loss.  Arguments as accumulate_ctc.  train=False:
        evaluation-mode forward, loss only."""
        args = self._ctc_args(X, utt_lens, labels, label_lens)
        self._accumulate_ctc("_mmi", *args, (_finite_nonneg("lm_scale", lm_scale), _finite_nonneg("ctc_weight", ctc_weight)),
                             last, train)

    def eval_accumulate_ctc_mmi(self, X, utt_lens, labels, label_lens, lm_scale=1.0, ctc_weight=0.0):
        self.accumulate_ctc_mmi(X, utt_lens, labels, label_lens, lm_scale, ctc_weight, train=False)

    def accumulate_ctc_mmi_raw(self, raw, utt_lens, context_width, labels, label_lens, lm_scale=1.0, ctc_weight=0.0,
                               last=False, cmvn=None, train=True):
        """accumulate_ctc_mmi from UNSPLICED frames: CMVN + splice on the device (as accumulate_ctc_raw)"""
        args = self._ctc_args(raw, utt_lens, labels, label_lens)
        self._accumulate_ctc("_mmi", *args, (_finite_nonneg("lm_scale", lm_scale), _finite_nonneg("ctc_weight", ctc_weight)),
                             last, train, (context_width, cmvn))

    # ---- CTC loss with wildcard gaps (W-CTC / STC): training on transcripts that cover only part of a recording ----
    def accumulate_ctc_wild(self, X, utt_lens, labels, label_lens, wild=None, penalty=0.0, last=False, train=True):
        """One micro-batch of the CTC loss with WILDCARD GAPS (tfk_accumulate_ctc_wild; the contract is stated in
        include/tfkaldi_hip.h): `wild` as ctc_align_wild takes it -- label_lens[u] + 1 flags per utterance, back to back
        (uint8 or bool; None: none set) -- and a flagged gap absorbs any frames at `penalty` per frame (finite, >= 0).  The
        loss is the value of the lattice: a labelling that several paths reach through a wildcard counts once per path, so
        it can be negative.  With no flag set this is accumulate_ctc bit for bit.  train=False: evaluation-mode forward,
        loss only."""
        args = self._ctc_args(X, utt_lens, labels, label_lens)
        self._accumulate_ctc("_wild", *args, (self._wild(wild, args[3], "CTC micro-batch"), _finite_nonneg("penalty", penalty)),
                             last, train)

    def eval_accumulate_ctc_wild(self, X, utt_lens, labels, label_lens, wild=None, penalty=0.0):
        self.accumulate_ctc_wild(X, utt_lens, labels, label_lens, wild, penalty, train=False)

    def accumulate_ctc_wild_raw(self, raw, utt_lens, context_width, labels, label_lens, wild=None, penalty=0.0, last=False,
                                cmvn=None, train=True):
        """accumulate_ctc_wild from UNSPLICED frames: CMVN + splice on the device (as accumulate_ctc_raw)"""
        args = self._ctc_args(raw, utt_lens, labels, label_lens)
        self._accumulate_ctc("_wild", *args, (self._wild(wild, args[3], "CTC micro-batch"), _finite_nonneg("penalty", penalty)),
                             last, train, (context_width, cmvn))

    # ---- the optimiser step in parts (data parallel: Adam per reduced span, see dataparallel.BucketReducer) ----
    def apply_begin(self):
        check(self.lib.tfk_apply_begin(self._h))

    def apply_span(self, offset_floats, num_floats):
        check(self.lib.tfk_apply_span(self._h, int(offset_floats), int(num_floats)))

    def apply_end(self):
        loss = c_float()
        check(self.lib.tfk_apply_end(self._h, byref(loss)))
        return float(loss.value)

    def apply(self):
        loss = c_float()
        check(self.lib.tfk_apply(self._h, byref(loss)))
        return float(loss.value)

    def apply_enqueue(self):
        """the optimiser step on the streams, not waited for: apply_end() collects the loss"""
        check(self.lib.tfk_apply_enqueue(self._h))

    def eval_accumulate(self, X, y):
        X, y = self._host_batch(X, y)
        check(self.lib.tfk_eval_accumulate(self._h, X.ctypes.data_as(c_void_p), X.shape[1],
                                           y.ctypes.data_as(c_void_p), X.shape[0], 0))

    def eval_finish(self):
        loss = c_float()
        check(self.lib.tfk_eval_finish(self._h, byref(loss)))
        return float(loss.value)

    def halve_learning_rate(self):
        check(self.lib.tfk_halve_learning_rate(self._h))

    def add_layer(self):
        self._param_access()  # (a control op on the parameters: refused while the fp32 masters are sharded)
        check(self.lib.tfk_add_layer(self._h))

    def init_last_layer(self):
        self._param_access()
        check(self.lib.tfk_init_last_layer(self._h))

    # ---- decoding ----
    def set_prior(self, prior):
        p = _f32(prior)
        check(self.lib.tfk_set_prior(self._h, p.ctypes.data_as(c_void_p), p.size))

    def posteriors(self, X, log_div_prior=False, raw_logits=False):
        X = _f32(X)
        out = self._out_buffer(X.shape[0])
        flags = (_lib.LOG_DIV_PRIOR if log_div_prior else 0) | (_lib.RAW_LOGITS if raw_logits else 0)
        check(self.lib.tfk_posteriors(self._h, X.ctypes.data_as(c_void_p), X.shape[1], X.shape[0],
                                      out.ctypes.data_as(c_void_p), self.O, flags))
        return out

    # ---- data parallelism ----
    def reduce_region(self):
        ptr, n = c_void_p(), c_size_t()
        check(self.lib.tfk_reduce_region(self._h, byref(ptr), byref(n)))
        return ptr.value, n.value

    def bucket_order(self):
        """the order in which accumulate(last=True) announces the buckets: scalars + BN increments, the weight
        matrices from the output layer down, the bias / beta gradients (include/tfkaldi_hip.h)"""
        L = self.L
        return [L + 2] + list(range(L + 1)) + [L + 1]

    def buckets(self):
        nb = c_int()
        check(self.lib.tfk_num_buckets(self._h, byref(nb)))
        out = []
        for b in range(nb.value):
            off, n = c_size_t(), c_size_t()
            check(self.lib.tfk_reduce_bucket(self._h, b, byref(off), byref(n)))
            out.append((off.value, n.value))
        return out

    def reduce_view(self):
        """torch view of the reduce region (requires torch_state=True)."""
        if self._state is None:
            raise RuntimeError("reduce_view needs Engine(..., torch_state=True)")
        ptr, n = self.reduce_region()
        off = (ptr - self._state.data_ptr()) // 4
        return self._state[off:off + n]

    def param_view(self):
        """torch view of the parameter arena [P] (same offsets as the gradient part of the reduce region); the
        sharded exchange step all-gathers the updated parameters straight into it (requires torch_state=True)"""
        if self._state is None:
            raise RuntimeError("param_view needs Engine(..., torch_state=True)")
        ptr, _ = self.reduce_region()
        return self._state[0:(ptr - self._state.data_ptr()) // 4]

    def params_touched(self):
        check(self.lib.tfk_params_touched(self._h))

    def twins_from_params(self, offset, n, stream=None):
        """the fp32 parameters [offset, offset + n) (whole weight matrices) were written behind the optimiser's back: rebuild
        what the contractions read from them (emulated fp32: the three-plane twins) on `stream` (None: the engine's).  True
        when that is now current for the span, False when nothing was done (the caller then uses params_touched)"""
        cur = c_int()
        check(self.lib.tfk_twins_from_params(self._h, int(offset), int(n), c_void_p(stream), byref(cur)))
        return bool(cur.value)

    def shadow_view(self):
        """torch bfloat16 view of the arena-mirroring weight shadow (mixed precision, every leading dimension a multiple
        of 8; requires torch_state=True), element offsets = those of the fp32 weight arena; None when there is none"""
        if self._state is None:
            raise RuntimeError("shadow_view needs Engine(..., torch_state=True)")
        import torch
        ptr, n, mirrors = c_void_p(), c_size_t(), c_int()
        check(self.lib.tfk_shadow_region(self._h, byref(ptr), byref(n), byref(mirrors)))
        if not mirrors.value or not n.value:
            return None
        off = (ptr.value - self._state.data_ptr()) // 4
        return self._state[off:off + (n.value + 1) // 2].view(torch.bfloat16)[:n.value]

    def apply_writes_shadow(self):
        """between apply_begin and apply_end: does apply_span write the bf16 shadow with the update?"""
        d = c_int()
        check(self.lib.tfk_apply_writes_shadow(self._h, byref(d)))
        return bool(d.value)

    def param_checksum(self, which=0):
        """64-bit integer checksum of the fp32 parameter arena (0) or the bf16 shadow (1); synchronises"""
        v = c_uint64()
        check(self.lib.tfk_param_checksum(self._h, int(which), byref(v)))
        return int(v.value)

    def set_bucket_callback(self, fn):
        """fn(bucket) is called from accumulate(last=True) once the bucket's kernels are enqueued."""
        if fn is None:
            self._cb = None
            check(self.lib.tfk_set_bucket_callback(self._h, _lib.BUCKET_FN(), None))
            return
        self._cb = _lib.BUCKET_FN(lambda user, bucket: fn(bucket))
        check(self.lib.tfk_set_bucket_callback(self._h, self._cb, None))

    def set_layer_callback(self, fn):
        """fn(layer) is called right before kernels that read the parameters of `layer` (0 .. L; -1 = all) are
        enqueued (tfk_set_layer_callback): the hook of the asynchronous parameter all-gather."""
        if fn is None:
            self._layer_cb = None
            check(self.lib.tfk_set_layer_callback(self._h, _lib.BUCKET_FN(), None))
            return
        self._layer_cb = _lib.BUCKET_FN(lambda user, layer: fn(layer))
        check(self.lib.tfk_set_layer_callback(self._h, self._layer_cb, None))

    def zero_accumulators(self):
        check(self.lib.tfk_zero_accumulators(self._h))

    def set_later_microbatches(self, later):
        check(self.lib.tfk_set_later_microbatches(self._h, int(later)))

    @property
    def torch_stream(self):
        return self._stream

    # ---- misc ----
    def synchronize(self):
        check(self.lib.tfk_synchronize(self._h))

    def profile_begin(self):
        check(self.lib.tfk_profile_begin(self._h))

    def profile_end(self):
        stats = (_lib.TfkKernelStat * 32)()
        n = c_int()
        check(self.lib.tfk_profile_end(self._h, stats, 32, byref(n)))
        return [dict(name=stats[i].name.decode(), launches=int(stats[i].launches), total_ms=stats[i].total_ms,
                     flops=stats[i].flops, bytes=stats[i].bytes) for i in range(min(n.value, 32))]

    def debug_fetch(self, what, layer, T):
        cols = self.O if what in (_lib.DBG_LOGITS, _lib.DBG_TRAIN_LOGITS) else self.H
        out = np.empty((T, cols), dtype=np.float32)
        check(self.lib.tfk_debug_fetch(self._h, what, layer, out.ctypes.data_as(c_void_p), out.size))
        return out

    def debug_capture(self, on=True):
        """tfk_debug_capture: the later non-stacked training passes keep the training logits (DBG_TRAIN_LOGITS; the loss
        overwrites them in place) and every hidden layer's dz as its bf16 twin, the only form mixed precision stores it in
        (TWIN_DPREACT; DBG_DPREACT returns the same values widened).  bf16 mode.  Off by default: a pass then enqueues nothing
        extra."""
        check(self.lib.tfk_debug_capture(self._h, int(bool(on))))

    def debug_fetch_twin(self, what, layer=0, T=None):
        """tfk_debug_fetch_twin: a bf16 operand twin as the contractions read it (bf16 mode), as a float32 array that holds
        exactly the bf16 values.  T: rows of the last call (not needed for TWIN_WEIGHTS)."""
        if what == _lib.TWIN_WEIGHTS:
            shape = (self.F if layer == 0 else self.H, self.O if layer == self.L else self.H)
        else:
            shape = (T, {_lib.TWIN_INPUT: self.F, _lib.TWIN_DLOGITS: self.O}.get(what, self.H))
        bits = np.empty(shape, dtype=np.uint16)
        check(self.lib.tfk_debug_fetch_twin(self._h, what, layer, bits.ctypes.data_as(c_void_p), bits.size))
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


class CtcStreamHandle(object):
    """A decode stream (tfk_ctc_stream_*; the contract is stated in include/tfkaldi_hip.h) that decodes with one Engine's model,
    on that engine's HIP stream.  Any way of cutting a lane's frames into pushes gives the result of one ctc_beam /
    ctc_beam_lm call on all of them, bit for bit."""

    def __init__(self, engine, lanes, beam_width, max_frames, label_topk=None):
        self.engine, self.lib = engine, engine.lib
        self.lanes, self.beam_width, self.max_frames = int(lanes), int(beam_width), int(max_frames)
        self.label_topk = 0 if label_topk is None else int(label_topk)
        if label_topk is not None and self.label_topk < 1:
            raise ValueError("label_topk %d outside [1, 63]" % self.label_topk)
        self._lm = None  # the model of the last push: what final=True takes the end-of-sequence switch from
        self._h = c_void_p()
        check(self.lib.tfk_ctc_stream_create(engine.O, self.lanes, self.beam_width, self.max_frames, self.label_topk,
                                             byref(self._h)))
        engine.on_close.append(self.close)  # (a stream is destroyed before the engine whose HIP stream it works on)

    def _hip_stream(self):
        stream = c_void_p()
        check(self.lib.tfk_stream(self.engine._h, byref(stream)))
        return stream

    def push(self, rows, chunk_lens, lm=None):
        """rows: SPLICED frames [sum(chunk_lens), F], lane l's chunk behind lane l - 1's; chunk_lens [lanes] (0: the lane
        idles).  lm: None, or the NgramLM / GraphLM the prefixes are ranked by -- the same one, with the same weights, for as
        long as a lane holds frames."""
        chunk_lens = np.ascontiguousarray(chunk_lens, dtype=np.int32).reshape(-1)
        if chunk_lens.size != self.lanes:
            raise ValueError("%d chunk lengths for %d lanes" % (chunk_lens.size, self.lanes))
        X = _f32(rows).reshape(-1, self.engine.F)
        flags, weight, bonus = 0, 0.0, 0.0
        if lm is not None:
            self.engine.ctc_set_lm(lm)
            flags, weight, bonus = _lib.CTC_LM, lm.weight, lm.label_bonus
        check(self.lib.tfk_ctc_stream_push(self.engine._h, self._h, _ptr(X) if X.shape[0] else c_void_p(None), X.shape[1],
                                           X.shape[0], _ptr(chunk_lens), c_float(weight), c_float(bonus), flags))
        self._lm = lm

    def result(self, top_paths=1, final=False, hyp_cap=None):
        """The N-best of every lane over what has been pushed: (hyps, scores, am_scores) -- hyps[l][n] int32 label arrays (cut
        at hyp_cap labels if given), scores / am_scores float32 [lanes, top_paths] as ctc_beam_lm returns them (without a
        model the two are equal).  final: with a model whose end_of_sequence is set, rank and score with its end term."""
        top_paths = int(top_paths)
        frames = self.frames()
        cap = int(frames.max()) if hyp_cap is None else int(hyp_cap)
        hyp = np.empty((top_paths, self.lanes, max(cap, 0)), dtype=np.int32)
        hyp_len = np.zeros((top_paths, self.lanes), dtype=np.int32)
        score = np.empty((top_paths, self.lanes), dtype=np.float32)
        am = np.empty((top_paths, self.lanes), dtype=np.float32)
        flags = _lib.CTC_LM_EOS if final and self._lm is not None and self._lm.end_of_sequence else 0
        check(self.lib.tfk_ctc_stream_result(self._h, self._hip_stream(), top_paths, flags, _ptr(hyp), cap, _ptr(hyp_len),
                                             _ptr(score), _ptr(am)))
        hyps = [[hyp[n, l, :min(hyp_len[n, l], cap)].copy() for n in range(top_paths)] for l in range(self.lanes)]
        return hyps, np.ascontiguousarray(score.T), np.ascontiguousarray(am.T)

    def reset(self, lane=None):
        check(self.lib.tfk_ctc_stream_reset(self._h, self._hip_stream(), -1 if lane is None else int(lane)))

    def frames(self):
        out = np.zeros(self.lanes, dtype=np.int32)
        check(self.lib.tfk_ctc_stream_frames(self._h, _ptr(out)))
        return out

    def close(self):
        if self._h:
            if self.engine._h:  # (the engine closes its streams itself, before it goes)
                self.engine.synchronize()
            check(self.lib.tfk_ctc_stream_destroy(self._h))
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass
