"""Data-parallel training over the GPUs of one node: one process per GPU, torch.distributed (backend
"nccl" = RCCL over xGMI) for the single exchange step of the path.

The reference splits every optimiser step into B/U independent micro-batches whose only coupling is
`G += g`, `batch_loss += loss`, `num_frames += n` (reference neuralNetworks/trainer.py:165-169) followed by
one mean -> clip -> Adam (:174-184).  Running the micro-batches on different GPUs and SUM-all-reducing the
engine's reduce region ([G | loss, frames, #micro-batches | BN moving-average increments]) before
`apply` is therefore the same computation.  Micro-batches are assigned to ranks in contiguous blocks (rank
order = the reference's serial order) so the BN moving averages compose exactly as its sequential updates
do (tfk_set_later_microbatches).  The all-reduce is bucketed per layer and launched from the engine's
bucket callback while the rest of backward is still being enqueued, i.e. overlapped with backward.

Works with any object that has the Engine methods used below; tests drive it with world_size-2 gloo
process groups on CPU.
"""
import contextlib
import os
import time
import weakref


def _share_device():
    """tests only -- several ranks on ONE GPU.  TFK_SHARE_DEVICE=1: pair it with TFK_DIST_BACKEND=gloo (RCCL refuses two
    ranks with the same host hash and PCI bus id).  TFK_FAKE_NODES=1: every rank claims a host of its own (NCCL_HOSTID), so
    REAL RCCL accepts them and the ranks talk through its socket transport over the loopback interface -- slow, but it is
    RCCL's own bootstrap, group launches and collective kernels at world > 1 on a 1-GPU box (tools/rccl_fake_nodes_probe.py)."""
    return os.environ.get("TFK_SHARE_DEVICE") == "1" or os.environ.get("TFK_FAKE_NODES") == "1"


def local_device():
    """the GPU this rank computes on: torchrun's LOCAL_RANK (folded onto the visible devices in the tests' shared-device modes)"""
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if _share_device():
        import torch
        if torch.cuda.is_available():
            local_rank %= torch.cuda.device_count()
    return local_rank


def init_from_env():
    """Join the process group described by torchrun's environment (RANK / WORLD_SIZE / LOCAL_RANK /
    MASTER_ADDR / MASTER_PORT).  Returns (rank, world, local_rank); a no-op for single-process runs."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # TFK_FORCE_DP=1 (tests only): run the exchange step even with a single rank, so that the RCCL call path
    # (async all-reduce of engine-state views from the bucket callback) is exercised on a 1-GPU box
    if world > 1 or os.environ.get("TFK_FORCE_DP") == "1":
        import torch
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            use_gpu = torch.cuda.is_available()
            if use_gpu:
                # TFK_SHARE_DEVICE=1 (tests only): several ranks on one GPU -- RCCL refuses that, so pair it
                # with TFK_DIST_BACKEND=gloo to exercise the host-side bucket / overlap logic on a 1-GPU box
                if _share_device():
                    local_rank = local_rank % torch.cuda.device_count()
                if os.environ.get("TFK_FAKE_NODES") == "1":  # (before RCCL is initialised: it reads these at init)
                    os.environ["NCCL_HOSTID"] = "tfk-fake-node-%d" % rank
                    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
                    os.environ.setdefault("NCCL_IB_DISABLE", "1")
                torch.cuda.set_device(local_rank)
            backend = os.environ.get("TFK_DIST_BACKEND") or ("nccl" if use_gpu else "gloo")
            if backend == "nccl":
                if world > 1 and os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY") != "0":
                    # (tfkaldi_amd/__init__.py sets it unless the launcher exported another value)
                    raise RuntimeError("HSA_ENABLE_IPC_MODE_LEGACY=%r: RCCL between processes needs dmabuf IPC on this "
                                       "driver -- export HSA_ENABLE_IPC_MODE_LEGACY=0 before the first HIP call"
                                       % os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"))
                dist.init_process_group(backend=backend, rank=rank, world_size=world,
                                        device_id=torch.device("cuda", local_rank))
            else:
                dist.init_process_group(backend=backend, rank=rank, world_size=world)
    if _share_device():
        import torch
        if torch.cuda.is_available():
            local_rank = local_rank % torch.cuda.device_count()
    return rank, world, local_rank


def rank_seed(seed, rank):
    """The dropout RNG key of data-parallel rank `rank`.  The engine draws the keep mask of element (row, column) of
    layer l in its k-th accumulate call from Philox(key = seed, counter = (column / 4, row, l, k)); ranks run the same
    call indices on DIFFERENT micro-batches, so with one shared key the micro-batches of a step would all be dropped
    with the same pattern (the reference draws a fresh mask in every session.run, activation.py:140-141).  Rank 0
    keeps `seed`, so a single-process run is unchanged."""
    return (int(seed) ^ ((int(rank) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF


class RawMicroBatch(object):
    """A micro-batch whose +-context splice (and optionally CMVN) happens on the device: unspliced frames
    [T, D], targets [T], utterance lengths [U], the context width and the optional [U, 2, D] (mean, std) table
    (tfk_accumulate_raw)."""

    def __init__(self, raw, y, lens, context_width, cmvn=None):
        self.raw, self.y, self.lens, self.context_width, self.cmvn = raw, y, lens, context_width, cmvn

    def accumulate(self, engine, last, train):
        if train:
            engine.accumulate_raw(self.raw, self.y, self.lens, self.context_width, last=last, cmvn=self.cmvn)
        else:
            engine.eval_accumulate_raw(self.raw, self.y, self.lens, self.context_width, cmvn=self.cmvn)


class StackedRawMicroBatches(object):
    """SEVERAL consecutive micro-batches of one optimiser step handed to the engine in one call
    (tfk_accumulate_stacked_raw): the unspliced frames of all their utterances back to back and the number of utterances of
    each micro-batch.  The engine multiplies them in one pass of the GEMMs and keeps what couples the rows of a micro-batch
    (batch-norm statistics, dropout stream) per micro-batch; the result is that of one accumulate_raw per micro-batch."""

    def __init__(self, raw, y, lens, context_width, cmvn, seg_utts):
        self.raw, self.y, self.lens, self.context_width, self.cmvn = raw, y, lens, context_width, cmvn
        self.seg_utts = list(seg_utts)

    def accumulate(self, engine, last, train):
        args = (self.raw, self.y, self.lens, self.context_width, self.seg_utts)
        if train:
            engine.accumulate_stacked_raw(*args, last=last, cmvn=self.cmvn)
        else:
            engine.eval_accumulate_stacked_raw(*args, cmvn=self.cmvn)


class CtcMicroBatch(object):
    """A micro-batch for the CTC loss: spliced frames [T, F] of U utterances, their frame counts, their label
    sequences back to back and the label counts (tfk_accumulate_ctc)."""

    def __init__(self, X, utt_lens, labels, label_lens, context_width=None, cmvn=None):
        self.X, self.utt_lens, self.labels, self.label_lens = X, utt_lens, labels, label_lens
        self.context_width, self.cmvn = context_width, cmvn  # context_width set: X holds UNSPLICED frames

    def _call(self, engine, stem, *extra, **kw):
        """engine.<stem>(frames, frame counts, labels, label counts, *extra, **kw) on spliced frames; on unspliced ones
        engine.<stem>_raw with the context width behind the frame counts and the cmvn table by keyword"""
        if self.context_width is None:
            return getattr(engine, stem)(self.X, self.utt_lens, self.labels, self.label_lens, *extra, **kw)
        return getattr(engine, stem + "_raw")(self.X, self.utt_lens, self.context_width, self.labels, self.label_lens, *extra,
                                              cmvn=self.cmvn, **kw)

    def accumulate(self, engine, last, train):
        if train:
            self._call(engine, "accumulate_ctc", last=last)
        elif self.context_width is None:
            engine.eval_accumulate_ctc(self.X, self.utt_lens, self.labels, self.label_lens)
        else:  # (unspliced frames have no evaluation method of their own: the training one's switch)
            self._call(engine, "accumulate_ctc", train=False)


class CtcMwerMicroBatch(CtcMicroBatch):
    """A CTC micro-batch trained on the expected number of label errors over an N-best list (tfk_accumulate_ctc_mwer) plus
    ctc_weight x the CTC loss.  It carries EITHER the pair tables (hyp_counts, hyp_labels, hyp_lens as Engine.ctc_score takes
    them) OR the settings of the search that finds the list: then the rank that trains the micro-batch decodes its N best
    itself, on the same engine, right before the accumulate (beam_width, top_paths; lm: an NgramLM or GraphLM that ranks the search;
    label_topk: the pruned search).  add_reference: the reference joins every list that lacks it."""

    def __init__(self, X, utt_lens, labels, label_lens, context_width=None, cmvn=None, hyp_counts=None, hyp_labels=None,
                 hyp_lens=None, beam_width=None, top_paths=None, lm=None, label_topk=None, add_reference=False,
                 ctc_weight=0.0):
        CtcMicroBatch.__init__(self, X, utt_lens, labels, label_lens, context_width, cmvn)
        tables = hyp_counts is not None
        if tables == (beam_width is not None):
            raise ValueError("a CtcMwerMicroBatch carries either the pair tables or the search settings (beam_width)")
        if tables and (hyp_labels is None or hyp_lens is None):
            raise ValueError("pair tables: hyp_counts, hyp_labels and hyp_lens go together")
        if not tables:
            top_paths = self.search_paths(beam_width, top_paths)
        self.hyp_counts, self.hyp_labels, self.hyp_lens = hyp_counts, hyp_labels, hyp_lens
        self.beam_width, self.top_paths, self.lm, self.label_topk = beam_width, top_paths, lm, label_topk
        self.add_reference, self.ctc_weight = bool(add_reference), float(ctc_weight)

    @staticmethod
    def search_paths(beam_width, top_paths):
        """the length of the N-best list of a search of width beam_width: top_paths, by default all of the beam"""
        top_paths = beam_width if top_paths is None else top_paths
        if not 1 <= int(top_paths) <= int(beam_width):
            raise ValueError("top_paths %r outside [1, beam_width = %r]" % (top_paths, beam_width))
        return top_paths

    def accumulate(self, engine, last, train):
        self._call(engine, "accumulate_ctc_mwer", *_mwer_tables(engine, self), ctc_weight=self.ctc_weight, last=last,
                   train=train)


class CtcMmiMicroBatch(CtcMicroBatch):
    """A CTC micro-batch trained on MMI against a denominator graph (tfk_accumulate_ctc_mmi): -(log p_ctc(reference) +
    lm_scale G(reference)) + log Z plus ctc_weight x the CTC loss.  graph: the GraphLM that is the denominator; the rank
    that trains the micro-batch sets it on its engine (Engine.ctc_set_den uploads only when it changes)."""

    def __init__(self, X, utt_lens, labels, label_lens, graph, context_width=None, cmvn=None, lm_scale=1.0, ctc_weight=0.0):
        CtcMicroBatch.__init__(self, X, utt_lens, labels, label_lens, context_width, cmvn)
        if graph is None:
            raise ValueError("a CtcMmiMicroBatch needs its denominator graph")
        self.graph, self.lm_scale, self.ctc_weight = graph, float(lm_scale), float(ctc_weight)

    def accumulate(self, engine, last, train):
        engine.ctc_set_den(self.graph)
        self._call(engine, "accumulate_ctc_mmi", lm_scale=self.lm_scale, ctc_weight=self.ctc_weight, last=last, train=train)


class CtcWildMicroBatch(CtcMicroBatch):
    """A CTC micro-batch trained on the CTC loss with wildcard gaps (tfk_accumulate_ctc_wild): wild holds label_lens[u] + 1
    flags per utterance, back to back (None: none set), and a flagged gap absorbs any frames at `penalty` per frame."""

    def __init__(self, X, utt_lens, labels, label_lens, wild=None, penalty=0.0, context_width=None, cmvn=None):
        CtcMicroBatch.__init__(self, X, utt_lens, labels, label_lens, context_width, cmvn)
        self.wild, self.penalty = wild, float(penalty)

    def accumulate(self, engine, last, train):
        self._call(engine, "accumulate_ctc_wild", wild=self.wild, penalty=self.penalty, last=last, train=train)


def _search(mb, beam_width=None, lm=None, label_topk=None):
    """(Engine method, keywords) of the decode of a CTC micro-batch: best path (beam_width None) or prefix beam search of that
    width, ranked by lm, pruned to label_topk labels per frame; the *_raw entry when the micro-batch holds unspliced frames"""
    entry, kw = ("ctc_greedy", {}) if beam_width is None else ("ctc_beam", {"beam_width": beam_width})
    if lm is not None:
        entry, kw = "ctc_beam_lm", dict(kw, lm=lm)
    if label_topk is not None:  # (forwarded only when given: an engine without the keyword keeps serving the other calls)
        kw = dict(kw, label_topk=label_topk)
    if mb.context_width is not None:  # unspliced frames: CMVN + splice on the device
        entry, kw = entry + "_raw", dict(kw, context_width=mb.context_width, cmvn=mb.cmvn)
    return entry, kw


def _nbest(engine, mb, top_paths, beam_width, lm, label_topk):
    """per utterance the top_paths best of that search, without the padding paths: they are not hypotheses, and the search's
    own ranking value -- beam score -inf -- is what marks them"""
    import numpy as np
    entry, kw = _search(mb, beam_width, lm, label_topk)
    found, beam = getattr(engine, entry)(mb.X, mb.utt_lens, top_paths=int(top_paths), **kw)[:2]
    return [[h for h, s in zip(hs, sc) if s > -np.inf] for hs, sc in zip(found, beam)]


def _mwer_tables(engine, mb):
    """the pair tables of an MWER micro-batch: its own, or the N best of a search on `engine` (evaluation passes that leave
    the sums of an open step alone)"""
    import numpy as np
    from .neuralNetworks.ctc_mwer import pair_tables
    refs = np.split(np.asarray(mb.labels, dtype=np.int32), np.cumsum(mb.label_lens, dtype=np.int64)[:-1])
    if mb.hyp_counts is not None:
        if not mb.add_reference:
            return mb.hyp_counts, mb.hyp_labels, mb.hyp_lens
        flat = np.split(np.asarray(mb.hyp_labels, dtype=np.int32), np.cumsum(mb.hyp_lens, dtype=np.int64)[:-1]) \
            if len(mb.hyp_lens) else []
        cuts = np.cumsum(mb.hyp_counts, dtype=np.int64)
        hyps = [flat[int(a):int(b)] for a, b in zip(np.concatenate([[0], cuts[:-1]]), cuts)]
        return pair_tables(hyps, refs, add_reference=True)
    kept = _nbest(engine, mb, mb.top_paths, mb.beam_width, mb.lm, mb.label_topk)
    return pair_tables(kept, refs, add_reference=mb.add_reference)


def _dispatch(engine, mb, last, train):
    """one micro-batch into the sums of the step (train) or of the evaluation: the classes above know their entry, anything
    else is an (X, y) pair of spliced frames and targets"""
    if hasattr(mb, "accumulate"):
        mb.accumulate(engine, last, train)
    elif train:
        engine.accumulate(mb[0], mb[1], last=last)
    else:
        engine.eval_accumulate(mb[0], mb[1])


def _accumulate(engine, mb, last):
    _dispatch(engine, mb, last, True)


def _eval_accumulate(engine, mb):
    _dispatch(engine, mb, False, False)


def _eval_accumulate_all(engine, mine):
    """validation over this rank's micro-batches (reference trainer.py:356-441: one run per micro-batch).  Rows are independent
    in evaluation mode, so plain (X, y) micro-batches go to the engine as ONE stacked pass (tfk_eval_accumulate_stacked: the
    weights are read once, the GEMMs fill the chip); anything else (CTC, already stacked) one by one"""
    plain = all(isinstance(mb, tuple) and len(mb) == 2 for mb in mine)
    if plain and len(mine) > 1 and hasattr(engine, "eval_accumulate_stacked") and os.environ.get("TFK_STACK", "1") != "0":
        import numpy as np
        engine.eval_accumulate_stacked(np.concatenate([np.asarray(x, dtype=np.float32) for x, _ in mine], 0),
                                       np.concatenate([np.asarray(y) for _, y in mine], 0), [len(y) for _, y in mine])
        return
    for mb in mine:
        _eval_accumulate(engine, mb)


def _beam_settings(beam_width, lm=None, label_topk=None, rescore_paths=None):
    """refuse the settings of a beam search where there is none (beam_width None: best-path decoding)"""
    if rescore_paths is not None and beam_width is None:
        raise ValueError("rescoring re-ranks the N best of a beam search: give beam_width with rescore_paths")
    if lm is not None and beam_width is None:
        raise ValueError("a language model ranks the prefixes of a beam search: give beam_width with lm")
    if label_topk is not None and beam_width is None:
        raise ValueError("label_topk prunes a beam search: give beam_width with label_topk")


def _label_errors(engine, mb, beam_width=None, lm=None, label_topk=None, rescore_paths=None):
    """(sum of the edit distances, number of reference labels) of one CTC micro-batch under best-path decoding
    (beam_width None) or under prefix beam search of that width (its best path; lm: ranked with that NgramLM or GraphLM; label_topk:
    pruned to the frame's label_topk most probable labels).  rescore_paths: an int N takes the search's N best, scores them
    exactly with their label errors (ctc_score) and counts the hypothesis that is best after decoder.ctc_rerank."""
    _beam_settings(beam_width, lm, label_topk, rescore_paths)
    if not isinstance(mb, CtcMicroBatch):
        raise TypeError("label errors need CTC micro-batches (label sequences), not %s" % type(mb).__name__)
    import numpy as np
    if rescore_paths is not None:
        from .neuralNetworks.decoder import ctc_rerank
        kept = _nbest(engine, mb, rescore_paths, beam_width, lm, label_topk)
        flat = [h for hs in kept for h in hs]
        labels = np.concatenate(flat) if flat else np.zeros(0, dtype=np.int32)
        raw = mb.context_width is not None
        scores, dists = getattr(engine, "ctc_score_raw" if raw else "ctc_score")(
            mb.X, mb.utt_lens, *((mb.context_width,) if raw else ()), [len(hs) for hs in kept], labels,
            [h.size for h in flat], ref_labels=mb.labels, ref_lens=mb.label_lens, **({"cmvn": mb.cmvn} if raw else {}))
        edits = [int(d[ctc_rerank(hs, sc, lm)[0][0]]) if len(hs) else int(n)
                 for hs, sc, d, n in zip(kept, scores, dists, mb.label_lens)]
        return int(np.sum(edits, dtype=np.int64)), int(np.sum(mb.label_lens, dtype=np.int64))
    entry, kw = _search(mb, beam_width, lm, label_topk)
    edits = getattr(engine, entry)(mb.X, mb.utt_lens, labels=mb.labels, label_lens=mb.label_lens, **kw)[-1]
    return int(np.sum(edits, dtype=np.int64)), int(np.sum(mb.label_lens, dtype=np.int64))


def _run_overlap(overlap):
    """the host work a step overlaps with the GPU (the dispenser's prefetch): run it, and hand back what it raised instead of
    letting it unwind in the middle of the step -- the collective part of the step must complete on every rank first (a rank
    that leaves early would hang its peers in their collectives); the caller re-raises after its wait"""
    if overlap is None:
        return None
    try:
        overlap()
    except BaseException as exc:  # noqa: BLE001 (re-raised by the caller, once the step is complete)
        return exc
    return None


def partition(num_items, world):
    """contiguous [start, end) blocks per rank, sizes differing by at most one (larger blocks first)"""
    base, extra = divmod(num_items, world)
    out, start = [], 0
    for r in range(world):
        n = base + (1 if r < extra else 0)
        out.append((start, start + n))
        start += n
    return out


class BucketReducer(object):
    """Turns the engine's bucket announcements (one per weight matrix, in backward order, then the vector / scalar
    tail) into asynchronous collectives launched while backward is still being enqueued.

    Consecutive announcements are adjacent in the reduce region (the arena is W_0 .. W_L and they arrive as
    W_L .. W_0), so they are COALESCED until a collective carries at least `min_bytes`: xGMI is point-to-point and a
    ring / tree step is bound by one link, so a few large collectives reach a much higher bus bandwidth than one
    per 16 MB layer, at the price of starting a little later.  TFK_DP_BUCKET_MB sets the size (default 48, 24 for the
    sharded exchange).

    Two exchange steps (`mode`, env TFK_DP_EXCHANGE):
      "sharded" (default)  every coalesced gradient span is REDUCE-SCATTERED in place (rank r receives the sum of
                 sub-span r), the optimiser (mean -> clip -> Adam, tfk_apply_span) runs on that 1/world of the
                 span only, and the updated parameters are ALL-GATHERED in place.  Same bytes on the wire as an
                 all-reduce, 1/world of the optimiser's HBM traffic per GPU (28 B per parameter: the step is
                 optimiser-bound at BASELINE cfg3 / cfg4 sizes).  Adam is element-wise, so the result is
                 identical to the replicated update.  Spans that do not divide (or are tiny: the bias / beta
                 vectors, the scalar + BN tail) are all-reduced and updated on every rank.
                 Mixed precision (engine.shadow_view() is not None): what is gathered is the rank's shard of the
                 bf16 weight SHADOW that tfk_apply_span wrote with the update -- 2 B per parameter instead of 4, and the
                 next forward pass (which reads only the shadow) waits for it layer by layer.  The fp32 masters of a
                 span then stay valid on its owner only; gather_masters() (collective) brings them home before a
                 checkpoint or a tensor get / set, and until then the engine's param_access_hook refuses such an access.
      "allreduce"  SUM all-reduce of every span, full optimiser on every rank (round 1).

    Whether the backend can reduce-scatter / all-gather tensors of this kind is decided ONCE, at construction, by a
    probe collective on a scratch tensor next to the engine state, agreed over all ranks (gloo on device memory, used by
    the single-GPU tests, cannot): without it the reducer runs "allreduce" and says so; with TFK_DP_EMULATE_RS=1
    (tests) the sharded protocol runs with the reduce-scatter emulated by an all-reduce.  Errors of the collectives
    themselves are never swallowed -- the probe's included when the backend is RCCL.

    The first TFK_DP_VERIFY_STEPS (default 2) sharded steps end with a replica check: every rank's checksum of the
    gathered parameters (tfk_param_checksum) must agree, otherwise the step raises -- a mis-ordered collective would
    train on stale weights silently (round-2 advisor finding)."""

    MIN_SHARD_FLOATS = int(os.environ.get("TFK_DP_MIN_SHARD", str(1 << 14)))  # smaller spans are all-reduced

    def __init__(self, engine, group=None, min_bytes=None, stream_ctx=None, mode=None):
        if os.environ.get("TFK_DP_WIRE") == "bf16":
            raise ValueError("TFK_DP_WIRE=bf16 is a feature of the in-library exchange (csrc/exchange.hip over RCCL); this job runs "
                             "the exchange through torch.distributed (TFK_DP_COMM=torch, a gloo group, or the fallback)")
        import torch.distributed as dist
        self._dist = dist
        self.group = group
        self.view, self.buckets = engine.reduce_view(), engine.buckets()
        self._stream_ctx = stream_ctx or contextlib.nullcontext
        mode = mode or os.environ.get("TFK_DP_EXCHANGE", "sharded")
        if mode not in ("sharded", "allreduce"):
            raise ValueError("exchange mode %r" % (mode,))
        if mode == "sharded" and not (hasattr(engine, "param_view") and hasattr(engine, "apply_span")):
            mode = "allreduce"
        ready = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if ready else 1
        self.rank = dist.get_rank(group) if ready else 0
        self.rs_impl = self.ag_impl = None  # "native" | "emulated"
        if mode == "sharded" and ready:
            self._probe()
            if self.rs_impl is None:
                mode = "allreduce"
        self.mode = mode
        if min_bytes is None:
            # 32 MiB per collective (csrc/exchange.hip: tfk_comm_create has the same default and the reasoning: a fixed cost
            # per collective speaks for few spans, the layer-by-layer consumption of the gathers and the exposed tail of
            # backward for small ones; exchange_timeline prices it).  Not tuned on a multi-GPU node: none was available
            default_mb = str(DEFAULT_BUCKET_MB)
            min_bytes = int(float(os.environ.get("TFK_DP_BUCKET_MB", default_mb)) * (1 << 20))
        self.min_floats = max(1, min_bytes // 4)
        self.num_params = self.buckets[-1][0]  # the scalar + BN tail starts where the gradient arena ends
        self.vec_off = self.buckets[-2][0] if len(self.buckets) >= 2 else self.num_params  # bias / beta vectors
        self.handles, self.errors = [], []
        self._lo = self._hi = None
        self.launched = []  # (offset, floats) of every collective of the current step (tests / diagnostics)
        self.kinds = []     # "rs" (reduce-scatter: only sub-span `rank` is valid afterwards) or "ar" per collective
        self.executed = []  # the torch.distributed calls actually issued this step, by name (bench.py reports them)
        self.last_launched, self.last_kinds, self.last_executed = [], [], []
        # Parameter all-gathers of the last sharded step that nobody has waited for yet, in launch order (ascending
        # offsets = forward order).  With an engine that announces parameter reads (tfk_set_layer_callback) they stay
        # in flight across the step boundary and the NEXT forward pass waits layer by layer: the gather of layer l+1's
        # weights travels over xGMI while layer l is being multiplied.
        self.pending = []
        self.async_gather = mode == "sharded" and hasattr(engine, "set_layer_callback")
        if self.async_gather:
            engine.set_layer_callback(self.on_layer)
        # mixed precision: gather the bf16 shadow instead of the fp32 parameters (masters stay with their owner)
        self.shadow = engine.shadow_view() if (mode == "sharded" and hasattr(engine, "shadow_view")) else None
        self.masters_stale = False
        self.shard_spans = set()
        if self.shadow is not None:
            engine.param_access_hook = self._param_access
        self.verify_left = int(os.environ.get("TFK_DP_VERIFY_STEPS", "2")) if (mode == "sharded" and ready) else 0
        # host time spent inside the callbacks / the apply pipeline (tools/dp_overhead.py)
        self.host_s = {"on_bucket": 0.0, "on_layer": 0.0, "finish_and_apply": 0.0}
        self.host_calls = {"on_bucket": 0, "on_layer": 0, "finish_and_apply": 0}

    # ---- what the backend can do, decided once ----
    def _probe(self):
        """reduce_scatter_tensor / all_gather_into_tensor, in place, on a scratch tensor of the state's kind; the outcome
        is agreed over the ranks (MIN), so that every rank issues the same collectives for the life of the reducer"""
        import torch
        d = self._dist
        n = 4 * self.world
        if not hasattr(self.view, "new_zeros"):
            return
        ok_rs = ok_ag = 1
        with self._stream_ctx():  # (the scratch tensor too: operands and collectives on one stream)
            scratch = self.view.new_zeros(n)
            own = scratch[self.rank * 4:(self.rank + 1) * 4]
            # Only a backend that CANNOT do the operation on this kind of tensor is a reason to fall back (gloo on device
            # memory: the single-GPU tests).  On RCCL a failing probe is a fault of the job -- a RuntimeError like any
            # other -- and is raised: swallowed, it would silently turn the whole run into all-reduce + replicated optimiser
            # (and ranks that did not fail would wait inside the probe for ever).
            can_fall_back = d.get_backend(self.group) != "nccl"
            try:
                d.reduce_scatter_tensor(own, scratch, op=d.ReduceOp.SUM, group=self.group)
            except (RuntimeError, NotImplementedError):
                if not can_fall_back:
                    raise
                ok_rs = 0
            try:
                d.all_gather_into_tensor(scratch, own, group=self.group)
            except (RuntimeError, NotImplementedError):
                if not can_fall_back:
                    raise
                ok_ag = 0
            flags = scratch.new_tensor([float(ok_rs), float(ok_ag)])
            d.all_reduce(flags, op=d.ReduceOp.MIN, group=self.group)
            ok_rs, ok_ag = (int(v) for v in flags.tolist())
        emulate = os.environ.get("TFK_DP_EMULATE_RS") == "1"
        self.rs_impl = "native" if ok_rs else ("emulated" if emulate else None)
        self.ag_impl = "native" if ok_ag else "emulated"  # (list-form all_gather into views: always available)
        if self.rs_impl is None:  # (said by EVERY rank: the log of any one of them shows the mode the job settled on)
            import sys
            sys.stderr.write("tfkaldi_amd.dataparallel[rank %d]: backend %r cannot reduce-scatter %s tensors in place; the "
                             "exchange step runs as all-reduce + replicated optimiser\n"
                             % (self.rank, d.get_backend(self.group), self.view.device))

    def _param_access(self):
        if self.masters_stale:
            raise RuntimeError(
                "the fp32 master weights are sharded over the data-parallel ranks (mixed-precision sharded exchange: each "
                "rank holds the masters of its own spans, everyone holds the bf16 shadow); call "
                "DataParallel.gather_parameters(engine) on EVERY rank before reading or writing parameters")

    def _shardable(self, lo, hi):
        n = hi - lo
        return (self.mode == "sharded" and hi <= self.vec_off and n % (4 * self.world) == 0
                and n >= self.MIN_SHARD_FLOATS)

    def _launch(self):
        if self._lo is None:
            return
        lo, hi, self._lo, self._hi = self._lo, self._hi, None, None
        if self.mode == "sharded":
            # a coalesced span that runs from the weight matrices into the bias / beta vectors, or from the gradient
            # arena into the scalar + BN tail, is cut there: only weight matrices are sharded (the vectors are a few
            # thousand values: all-reduced and updated on every rank, so that no layer ever waits for THEIR gather)
            for cut in (self.vec_off, self.num_params):
                if lo < cut < hi:
                    self._lo, self._hi = lo, cut
                    self._launch()
                    self._lo, self._hi = cut, hi
                    self._launch()
                    return
        d = self._dist
        with self._stream_ctx():
            if self._shardable(lo, hi) and self.rs_impl == "native":
                c = (hi - lo) // self.world
                own = self.view[lo + self.rank * c:lo + (self.rank + 1) * c]
                self.handles.append(d.reduce_scatter_tensor(own, self.view[lo:hi], op=d.ReduceOp.SUM, group=self.group,
                                                            async_op=True))
                self.kinds.append("rs")
                self.executed.append("reduce_scatter_tensor")
            else:
                # (emulated reduce-scatter, tests: every rank receives the whole sum and uses its own sub-span only)
                emu = self._shardable(lo, hi) and self.rs_impl == "emulated"
                self.handles.append(d.all_reduce(self.view[lo:hi], op=d.ReduceOp.SUM, group=self.group,
                                                 async_op=True))
                self.kinds.append("rs" if emu else "ar")
                self.executed.append("all_reduce(emulating reduce_scatter)" if emu else "all_reduce")
        self.launched.append((lo, hi - lo))

    # ---- the three things DataParallel asks of a reducer around a step (NativeExchange has the same) ----
    native = False

    def begin_step(self, engine):
        engine.set_bucket_callback(self.on_bucket)

    def end_step(self, engine):
        engine.set_bucket_callback(None)

    def idle(self, engine):
        """a rank without a micro-batch in this step: contribute zeros, announced in the engine's own order (every rank
        must launch the same collectives in the same order)"""
        engine.zero_accumulators()
        order = engine.bucket_order() if hasattr(engine, "bucket_order") else range(len(self.buckets))
        for b in order:
            self.on_bucket(b)

    def eval_finish(self, engine, dp):
        off, n = engine.buckets()[-1]
        with self._stream_ctx():
            self._dist.all_reduce(engine.reduce_view()[off:off + n], op=self._dist.ReduceOp.SUM, group=self.group)
        return engine.eval_finish()

    def on_bucket(self, b):
        t0 = time.perf_counter()
        try:  # exceptions cannot propagate through the C callback
            off, n = self.buckets[b]
            if self._lo is not None and off + n == self._lo:
                self._lo = off
            elif self._lo is not None and off == self._hi:
                self._hi = off + n
            else:
                self._launch()
                self._lo, self._hi = off, off + n
            if self._hi - self._lo >= self.min_floats:
                self._launch()
        except Exception as exc:  # noqa: BLE001
            self.errors.append(exc)
        self.host_s["on_bucket"] += time.perf_counter() - t0
        self.host_calls["on_bucket"] += 1

    def _raise_errors(self):
        if self.errors:
            exc = self.errors[0]
            del self.errors[:]  # reported once; the reducer stays usable for a caller that handles it
            raise exc

    def drain(self):
        """make the engine's stream wait for every parameter all-gather still in flight"""
        if self.pending:
            with self._stream_ctx():
                for _, _, h in self.pending:  # each one: a backend may complete collectives out of launch order (gloo
                    h.wait()                  # runs them on a thread pool; the 8-rank cfg2-size test caught exactly that)
            del self.pending[:]

    def on_layer(self, layer):
        """engine hook (tfk_set_layer_callback): kernels that read the parameters of `layer` (0 .. L, -1 = all) are
        about to be enqueued -- wait for the gathers that cover them (weights of the layer + the bias / beta vectors)"""
        if not self.pending:
            return
        t0 = time.perf_counter()
        try:
            if layer < 0:
                self.drain()
            else:
                num_layers = len(self.buckets) - 3
                spans = [self.buckets[num_layers - layer], self.buckets[num_layers + 1]]
                last = -1
                for i, (off, n, _) in enumerate(self.pending):
                    if any(off < so + sn and off + n > so for so, sn in spans):
                        last = i
                if last >= 0:
                    with self._stream_ctx():
                        for _, _, h in self.pending[:last + 1]:  # (everything launched before it as well: see drain)
                            h.wait()
                    del self.pending[:last + 1]
        except Exception as exc:  # noqa: BLE001  (cannot propagate through the C callback)
            self.errors.append(exc)
        self.host_s["on_layer"] += time.perf_counter() - t0
        self.host_calls["on_layer"] += 1

    def finish(self):
        """launch what is still pending, make the engine's stream wait for every collective of the step (all-reduce
        mode only: after a reduce-scatter the gradient arena is not whole)"""
        if self.mode != "allreduce":
            raise RuntimeError("BucketReducer.finish() needs mode='allreduce'; use finish_and_apply()")
        self._launch()
        self._raise_errors()
        with self._stream_ctx():
            for h in self.handles:
                h.wait()
        del self.handles[:]
        self.last_kinds, self.kinds = self.kinds, []
        self.last_executed, self.executed = self.executed, []
        self.last_launched, self.launched = self.launched, []
        return self.last_launched

    def _all_gather(self, whole, own):
        d = self._dist
        if self.ag_impl == "emulated":  # (gloo on device memory, tests) list form, straight into the sub-span views
            self.executed.append("all_gather(list)")
            return d.all_gather(list(whole.chunk(self.world)), own, group=self.group, async_op=True)
        self.executed.append("all_gather_into_tensor(bf16 shadow)" if whole.element_size() == 2
                             else "all_gather_into_tensor")
        return d.all_gather_into_tensor(whole, own, group=self.group, async_op=True)

    def finish_and_apply(self, engine, overlap=None):
        """(`overlap`: host work to run once EVERYTHING of the step is launched -- collectives, Adam, gathers -- and before the
        host waits for the loss.)  The optimiser step pipelined behind the collectives: the engine's stream waits for the (small, early)
        collective that carries the scalars, starts the step (tfk_apply_begin), then waits for each remaining
        collective in launch order and runs Adam on exactly the span of parameters whose gradient sum this rank now
        holds (tfk_apply_span) while the later collectives are still in flight; a reduce-scattered span's updated
        parameters (mixed precision: its bf16 shadow) are all-gathered behind its Adam.  Returns the average loss
        (tfk_apply_end)."""
        if not hasattr(engine, "apply_span"):
            self.finish()
            failed = _run_overlap(overlap)
            loss = engine.apply()
            if failed is not None:
                raise failed
            return loss
        t0 = time.perf_counter()
        self._launch()
        self._raise_errors()
        head_off, head_n = self.buckets[-1]
        waited = set()

        def wait(i):
            if i not in waited:
                with self._stream_ctx():
                    self.handles[i].wait()
                waited.add(i)

        for i, (off, n) in enumerate(self.launched):
            if off < head_off + head_n and off + n > head_off:
                wait(i)
        self.drain()  # (gathers of the previous step that no forward pass has consumed: none in a training loop)
        engine.apply_begin()
        # mixed precision: does this step's Adam write the shadow (it does unless parameters were set from outside
        # since the last forward pass)?  Then the shadow is what travels.
        via_shadow = self.shadow is not None
        if via_shadow and not engine.apply_writes_shadow():
            # (cannot happen: tfk_apply_begin makes an arena-mirroring shadow current on every rank -- the choice of what
            # is gathered must never depend on what one rank happened to run)
            raise RuntimeError("mixed-precision engine with an arena-mirroring shadow that the optimiser does not write")
        sharded = []
        for i, (off, n) in enumerate(self.launched):
            wait(i)
            if self.kinds[i] == "rs":
                c = n // self.world
                engine.apply_span(off + self.rank * c, c)
                sharded.append((off, n))
            else:
                engine.apply_span(off, n)  # (spans beyond the parameter arena are clipped by the engine)
        if sharded:
            if self.masters_stale and not via_shadow:
                # (parameters were injected between two sharded steps without gather_parameters: refused by the hook
                # long before this point; kept as a guard)
                raise RuntimeError("sharded fp32 masters and a step that does not write the shadow")
            target = self.shadow if via_shadow else engine.param_view()
            with self._stream_ctx():  # behind the optimiser kernels on the engine stream, lowest offsets (layer 0) first
                for off, n in sorted(sharded):
                    c = n // self.world
                    lo = off + self.rank * c
                    self.pending.append((off, n, self._all_gather(target[off:off + n], target[lo:lo + c])))
            if via_shadow:
                self.masters_stale = True
                self.shard_spans.update(sharded)
            elif hasattr(engine, "params_touched"):
                # parameters outside this rank's spans change behind the optimiser's back.  Emulated fp32: the three-plane twins
                # of each span are rebuilt right behind ITS gather on a side stream (tfk_twins_from_params, as csrc/exchange.hip
                # does), and the forward pass waits for gather + rebuild layer by layer -- instead of all twins, every gather
                # awaited, in front of the next pass (tfk_params_touched; round-5 advisor finding)
                if not self._twins_behind_gathers(engine, len(sharded)):
                    engine.params_touched()
            if not self.async_gather:
                self.drain()
        del self.handles[:]
        self.last_launched, self.launched = self.launched, []
        self.last_kinds, self.kinds = self.kinds, []
        self.last_executed, self.executed = self.executed, []
        self.host_s["finish_and_apply"] += time.perf_counter() - t0
        failed = _run_overlap(overlap)
        t0 = time.perf_counter()
        loss = engine.apply_end()
        if self.verify_left > 0 and sharded:
            self.verify_left -= 1
            self.verify_replicas(engine, via_shadow)
        self.host_s["finish_and_apply"] += time.perf_counter() - t0
        self.host_calls["finish_and_apply"] += 1
        if failed is not None:
            raise failed
        return loss

    def _twins_behind_gathers(self, engine, count):
        """the last `count` pending gathers: what the contractions read of their spans rebuilt behind each, on a side stream;
        False when the engine has nothing of the kind or refuses (nothing pending was changed then)"""
        if not self.async_gather or not hasattr(engine, "twins_from_params") or getattr(engine, "torch_stream", None) is None:
            return False
        import torch

        class _Behind(object):
            def __init__(self, event):
                self.event = event

            def wait(self):
                torch.cuda.current_stream().wait_event(self.event)

        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream()
        done = []
        try:
            with torch.cuda.stream(self._side):
                for off, n, h in self.pending[-count:]:
                    h.wait()
                    if not engine.twins_from_params(off, n, stream=self._side.cuda_stream):
                        return False
                    ev = torch.cuda.Event()
                    ev.record(self._side)
                    done.append((off, n, _Behind(ev)))
        except Exception:  # noqa: BLE001  (a span the engine refuses: the general way, params_touched)
            return False
        self.pending[-count:] = done
        return True

    def verify_replicas(self, engine, via_shadow):
        """every rank must hold the same parameters after the gathers (tfk_param_checksum); collective"""
        if not hasattr(engine, "param_checksum"):
            return
        import torch
        self.drain()
        sums = [engine.param_checksum(1), engine.param_checksum(2)] if via_shadow else [engine.param_checksum(0)]
        d = self._dist
        dev = self.view.device
        mine = [s & 0x7FFFFFFFFFFFFFFF for s in sums]
        # Everything on ONE stream -- the upload, the collectives (a backend orders itself against the stream that is
        # current when it is called) and the read-back: built on the default stream and reduced under the engine's, the
        # operands could reach the collective before their values did (seen as a rank reporting checksum 0 with eight
        # gloo ranks on one GPU).
        with self._stream_ctx():
            lo = torch.tensor(mine, dtype=torch.int64, device=dev)
            hi = lo.clone()
            d.all_reduce(lo, op=d.ReduceOp.MIN, group=self.group)
            d.all_reduce(hi, op=d.ReduceOp.MAX, group=self.group)
            lo, hi = lo.tolist(), hi.tolist()
        if lo != hi:
            raise RuntimeError("data-parallel replicas diverged after the sharded exchange step: rank %d holds parameter "
                               "checksum %s, the ranks' values span %s .. %s" % (self.rank, mine, lo, hi))

    def gather_masters(self, engine):
        """Collective.  Mixed-precision sharded exchange: all-gather the fp32 masters of every sharded span (each rank
        holds only its own shard up to date), so that parameters can be read / written from outside the optimiser."""
        if not self.masters_stale:
            return
        self.drain()
        params = engine.param_view()
        with self._stream_ctx():
            for off, n in sorted(self.shard_spans):
                c = n // self.world
                lo = off + self.rank * c
                self._all_gather(params[off:off + n], params[lo:lo + c]).wait()
        del self.executed[:]
        self.masters_stale = False


class NativeExchange(object):
    """The exchange step run INSIDE the library (include/tfkaldi_hip.h: tfk_comm, csrc/exchange.hip): the protocol of
    BucketReducer -- coalesced reduce-scatter / all-reduce of the gradient spans from backward's bucket announcements,
    Adam per reduced span, all-gather of the updated parameters (bf16 shadow in mixed precision) consumed layer by layer
    by the next forward pass -- with RCCL called from C++ on a stream the library owns.  No Python callback, no
    torch.distributed call and no ctypes round trip per span is left in the step: one call replaces engine.apply().

    torch.distributed is used once, to hand rank 0's RCCL unique id to the other ranks.  `loopback` (tests): a
    (group handle, rank) pair instead -- N engines of one process on one GPU, each driven by its own thread."""

    native = True

    def __init__(self, engine, group=None, mode=None, min_bytes=None, loopback=None):
        import ctypes
        from . import _lib
        self.lib = engine.lib
        self._check = _lib.check
        mode = mode or os.environ.get("TFK_DP_EXCHANGE", "sharded")
        if mode not in _lib.EXCHANGE:
            raise ValueError("exchange mode %r" % (mode,))
        if min_bytes is None and os.environ.get("TFK_DP_BUCKET_MB"):
            min_bytes = int(float(os.environ["TFK_DP_BUCKET_MB"]) * (1 << 20))
        self._h = ctypes.c_void_p()
        if loopback is not None:
            handle, rank = loopback
            self._check(self.lib.tfk_comm_create_loopback(engine._h, handle, int(rank), _lib.EXCHANGE[mode], int(min_bytes or 0),
                                                          ctypes.byref(self._h)))
        else:
            import torch
            import torch.distributed as dist
            rank, world = dist.get_rank(group), dist.get_world_size(group)
            uid, failed = ctypes.create_string_buffer(128), None
            if rank == 0:
                try:
                    self._check(self.lib.tfk_comm_unique_id(uid, 128, None))
                except Exception as e:  # noqa: BLE001 (the others are about to wait for the id: they must hear of it first)
                    failed = e
            # the id travels as a byte tensor over the process group that is already up (its only use in this class);
            # byte 0 says whether rank 0 has one at all
            t = torch.frombuffer(bytearray((b"\0" if failed else b"\1") + uid.raw), dtype=torch.uint8).clone()
            on_gpu = dist.get_backend(group) == "nccl"
            if on_gpu:
                t = t.cuda(engine.cfg.device)
            dist.broadcast(t, src=0, group=group)
            if failed is not None:
                raise failed
            raw = bytes(t.cpu().numpy().tobytes())
            if raw[0] != 1:
                raise RuntimeError("rank 0 could not obtain an RCCL unique id")
            raw = raw[1:]
            self._check(self.lib.tfk_comm_create(engine._h, raw, 128, rank, world, _lib.EXCHANGE[mode], int(min_bytes or 0),
                                                 ctypes.byref(self._h)))
        r, w, m, sh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self.lib.tfk_comm_info(self._h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(m), ctypes.byref(sh)))
        self.rank, self.world = r.value, w.value
        self.mode = "sharded" if m.value == 0 else "allreduce"
        self.backend = self.lib.tfk_comm_backend(self._h).decode()
        self.shadow = sh.value == 1   # mixed precision: the bf16 shadow is what is gathered
        self.planes = sh.value == 2   # emulated fp32 with TFK_DP_GATHER=planes: owner-written three-plane twin rows
        self.buckets = engine.buckets()
        if self.mode == "sharded":    # (either way the fp32 masters may be left with their owners: refuse to hand out stale ones)
            engine.param_access_hook = self._param_access
        engine.on_close.insert(0, self.close)  # (the comm goes before its engine)
        self.last_launched, self.last_kinds, self.last_executed = [], [], []
        self.host_s = {"on_bucket": 0.0, "on_layer": 0.0, "finish_and_apply": 0.0}
        self.host_calls = {"on_bucket": 0, "on_layer": 0, "finish_and_apply": 0}
        # wire format of the reduce-scattered gradient spans (csrc/exchange.hip reads the same variable at attach)
        self.wire = "bf16" if os.environ.get("TFK_DP_WIRE") == "bf16" else "fp32"

    def close(self):
        if self._h:
            self._check(self.lib.tfk_comm_destroy(self._h))
            self._h = None

    @property
    def masters_stale(self):
        import ctypes
        v = ctypes.c_int()
        self._check(self.lib.tfk_comm_masters_stale(self._h, ctypes.byref(v)))
        return bool(v.value)

    def _param_access(self):
        if self._h and self.masters_stale:
            raise RuntimeError(
                "the fp32 master weights are sharded over the data-parallel ranks (mixed-precision sharded exchange: each "
                "rank holds the masters of its own spans, everyone holds the bf16 shadow -- or, TFK_DP_GATHER=planes, the "
                "three-plane twins); call DataParallel.gather_parameters(engine) on EVERY rank before reading or writing parameters")

    def set_gather(self, planes):
        """COLLECTIVE, between steps (tfk_comm_set_gather): gather the owner-written three-plane twin rows of every weight matrix
        (emulated fp32) instead of fp32 parameters + a rebuild on every rank; False switches back and brings the masters home"""
        self._check(self.lib.tfk_comm_set_gather(self._h, 1 if planes else 0))
        self.planes = bool(planes)

    def set_bucket_bytes(self, nbytes):
        """between steps, every rank alike: adjacent gradient buckets are coalesced until a collective carries this much (0: the default, 32 MiB)"""
        self._check(self.lib.tfk_comm_set_bucket_bytes(self._h, int(nbytes)))

    def my_shards(self, off, n, rank=None):
        """[(offset, floats)] of what rank `rank` (default: this one) owns of the reduce-scattered span [off, off + n): the
        rank-th of world equal parts of the span -- or, with plane gathers, of every weight matrix in it"""
        r = self.rank if rank is None else rank
        if not self.planes:
            return [(off + r * (n // self.world), n // self.world)]
        out = []
        for bo, bn in sorted(self.buckets[:len(self.buckets) - 2]):
            if bo >= off and bo + bn <= off + n:
                out.append((bo + r * (bn // self.world), bn // self.world))
        return out

    def begin_step(self, engine):
        pass  # (the comm sits behind the engine's bucket hook since it was created)

    def end_step(self, engine):
        pass

    def idle(self, engine):
        self._check(self.lib.tfk_comm_idle(self._h))

    def finish_reduce(self):
        """(tests) every collective of the step launched and awaited on the engine stream, the optimiser not yet run"""
        self._check(self.lib.tfk_comm_finish_reduce(self._h))

    def finish_and_apply(self, engine, overlap=None):
        """tail collectives, Adam on this rank's spans and the parameter gathers launched (tfk_comm_apply_enqueue), then
        `overlap()` -- host work while the GPU is busy --, then the wait for the loss (tfk_comm_apply_end)"""
        import ctypes
        t0 = time.perf_counter()
        loss = ctypes.c_float()
        self._check(self.lib.tfk_comm_apply_enqueue(self._h))
        self.host_s["finish_and_apply"] += time.perf_counter() - t0
        failed = _run_overlap(overlap)
        t0 = time.perf_counter()
        self._check(self.lib.tfk_comm_apply_end(self._h, ctypes.byref(loss)))
        self.host_s["finish_and_apply"] += time.perf_counter() - t0
        self.host_calls["finish_and_apply"] += 1
        self._last_step()
        if failed is not None:
            raise failed
        return float(loss.value)

    def _last_step(self):
        import ctypes
        rs, ag, ar, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        spans = (ctypes.c_size_t * 96)()
        self._check(self.lib.tfk_comm_last_step(self._h, ctypes.byref(rs), ctypes.byref(ag), ctypes.byref(ar), spans, 32,
                                                ctypes.byref(n)))
        self.last_launched = [(int(spans[3 * i]), int(spans[3 * i + 1])) for i in range(min(n.value, 32))]
        self.last_span_kinds = ["rs" if spans[3 * i + 2] else "ar" for i in range(min(n.value, 32))]
        gather = "all_gather(bf16 shadow)" if self.shadow else "all_gather(three-plane twins)" if self.planes else "all_gather"
        # (the backend's own collectives keep their plain names; the direct algorithm / the bf16 wire are said in brackets)
        info = self.exchange_info()
        rs_tag = "".join(t for t, on in (("[direct]", info["reduce_scatter"] == "direct" and info["wire"] == "fp32"),
                                         ("[direct, bf16 wire]", info["wire"] == "bf16")) if on)
        ag_tag = "[direct]" if info["all_gather"] == "direct" else ""
        self.last_executed = (["%s:reduce_scatter%s" % (self.backend, rs_tag)] * rs.value
                              + ["%s:all_reduce" % self.backend] * ar.value
                              + ["%s:%s%s" % (self.backend, gather, ag_tag)] * ag.value)
        self.last_kinds = ["rs"] * rs.value + ["ar"] * ar.value

    def eval_finish(self, engine, dp):
        import ctypes
        loss = ctypes.c_float()
        self._check(self.lib.tfk_comm_eval_finish(self._h, ctypes.byref(loss)))
        return float(loss.value)

    # ---- how the spans travel (include/tfkaldi_hip.h, ABI 8) ----
    ALGOS, WIRES = ("rccl", "direct"), ("fp32", "bf16")
    PHASES = ("reduce_scatter", "all_reduce", "tail_exposed", "adam", "all_gather", "twin_rebuild", "gather_exposed")

    def set_exchange(self, algo=None, wire=None):
        """between steps, every rank alike: algo "rccl" | "direct" (RCCL's own reduce-scatter / all-gather, or grouped
        send / recv to all peers + the owner's rank-ordered sum), wire "fp32" | "bf16"; None keeps what is in force"""
        a = -1 if algo is None else self.ALGOS.index(algo)
        w = -1 if wire is None else self.WIRES.index(wire)
        self._check(self.lib.tfk_comm_set_exchange(self._h, a, w))
        if wire is not None:
            self.wire = wire

    def exchange_info(self):
        import ctypes
        rs, ag, w, by = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        us = (ctypes.c_double * 4)()
        self._check(self.lib.tfk_comm_get_exchange(self._h, ctypes.byref(rs), ctypes.byref(ag), ctypes.byref(w), ctypes.byref(by), us))
        out = {"reduce_scatter": self.ALGOS[rs.value], "all_gather": self.ALGOS[ag.value], "wire": self.WIRES[w.value],
               "chosen_by": ("default", "environment", "tuned at attach", "set")[by.value]}
        if any(us):
            out["tuned_us_slowest_rank"] = {"reduce_scatter_rccl": us[0], "reduce_scatter_direct": us[1],
                                            "all_gather_rccl": us[2], "all_gather_direct": us[3]}
        return out

    def tune(self, floats, iters=5):
        """COLLECTIVE: time both algorithms on scratch memory and keep the faster per operation (what attach does under `auto`)"""
        self._check(self.lib.tfk_comm_tune(self._h, int(floats), int(iters)))
        return self.exchange_info()

    def timing_begin(self):
        self._check(self.lib.tfk_comm_timing(self._h, 1))

    def timing_read(self):
        """{phase: device ms per step} over the steps since timing_begin (tfk_comm_timing_read), and their number"""
        import ctypes
        ms, steps = (ctypes.c_double * 8)(), ctypes.c_long()
        self._check(self.lib.tfk_comm_timing_read(self._h, ms, 8, ctypes.byref(steps)))
        self._check(self.lib.tfk_comm_timing(self._h, 0))
        return dict(zip(self.PHASES, list(ms)[:len(self.PHASES)])), int(steps.value)

    def drain(self):
        if self._h:
            self._check(self.lib.tfk_comm_drain(self._h))

    def gather_masters(self, engine):
        self._check(self.lib.tfk_comm_gather_masters(self._h))


DEFAULT_BUCKET_MB = 32   # coalescing threshold of the gradient spans, MiB (csrc/exchange.hip: kDefaultBucketBytes)
XGMI_LINK_GBPS = 153.0  # MI355X: 7 xGMI links per GPU, point to point, ~153 GB/s per link (8-GPU full mesh) -- taken here as the rate of ONE
# direction; if the quoted figure is the two directions' sum (MI300X's 128 GB/s per link is: 64 each way) every wire time below
# doubles -- exchange_timeline_sweep therefore runs at 1.0 / 0.5 / 0.3 of it, and bench.py's measured_wire_rate says what a run got


def exchange_model(buckets, world, fwd_ms, bwd_ms, adam_ms, step_ms, mode="sharded", min_bytes=DEFAULT_BUCKET_MB << 20, gather_elem_bytes=4,
                   fixed_ms=0.045, link_gbps=XGMI_LINK_GBPS, reduce_elem_bytes=4, twin_rebuild_ms=0.0):
    """What the exchange step of a `world`-GPU job should cost, from one GPU's measured step -- a PREDICTION to hold the first
    real scaling line against (no multi-GPU node was available to any round of this build; reference seam
    neuralNetworks/trainer.py:165-184).

    buckets: the engine's announcements [(offset, floats)]: W_L .. W_0 in backward order, then the vectors, then the scalar +
    BN tail.  fwd_ms / bwd_ms / adam_ms / step_ms: one rank's forward (incl. loss), backward, optimiser and whole-step time.
    Model: weight buckets coalesce into spans of >= min_bytes in announcement order (BucketReducer.on_bucket /
    csrc/exchange.hip); a span is ready when the backward pass has produced its last (lowest) layer, backward time spread
    evenly over the layers; collectives of one communicator run one after the other.  Two wire models per collective over the
    full mesh: `direct` -- every rank exchanges its 1/world sub-spans with all world - 1 peers at once, one sub-span per link
    (what a reduce-scatter / all-gather IS on point-to-point links) -- and `ring` (one link's rate bounds the whole transfer).
    sharded: reduce-scatter reduce_elem_bytes/param in (4; 2 with TFK_DP_WIRE=bf16), Adam on 1/world of the span, all-gather
    gather_elem_bytes/param out (2 with the bf16 shadow), the gathers hidden under the next forward pass except the first span's; allreduce: both halves before a full
    Adam.  fixed_ms: stream bookkeeping measured with one RCCL rank (profiles/r04_dp_overhead.txt).  twin_rebuild_ms (emulated
    fp32, sharded): the time to rebuild the three-plane twins of ALL weight matrices from gathered fp32 parameters.  Each span's
    share runs right behind its gather on the gather's stream (tfk_twins_from_params) -- no longer in front of the forward pass
    with every gather awaited -- but it is charged IN FULL: an HBM-bound kernel beside power-bound contractions takes its own
    time out of them (measured with one RCCL rank: sharded costs ~50 us more than all-reduce at cfg2, profiles/r05_dp_overhead.txt)."""
    L1 = len(buckets) - 2  # weight matrices
    min_floats = max(1, min_bytes // 4)
    spans, lo = [], None
    for b in range(L1):  # announcement order: W_L first
        off, n = buckets[b]
        if lo is None:
            lo, hi, first = off, off + n, b
        elif off + n == lo:
            lo = off
        elif off == hi:
            hi = off + n
        else:
            spans.append((lo, hi - lo, first, b - 1))
            lo, hi, first = off, off + n, b
        if hi - lo >= min_floats:
            spans.append((lo, hi - lo, first, b))
            lo = None
    if lo is not None:
        spans.append((lo, hi - lo, first, L1 - 1))
    tail = sum(n for _, n in buckets[L1:])
    per_layer_bwd = bwd_ms / float(L1)
    out = {"world": world, "mode": mode, "link_GBps_per_direction": link_gbps, "links_used": world - 1, "spans": [],
           "min_span_bytes": min_bytes}

    def wire_ms(bytes_total, kind):
        """one in-place collective over `bytes_total` bytes per rank buffer"""
        shard = bytes_total / float(world)
        if kind == "direct":
            return shard / (link_gbps * 1e9) * 1e3            # world - 1 links in parallel, one shard each
        return shard * (world - 1) / (link_gbps * 1e9) * 1e3  # ring: world - 1 steps over one link

    for model in ("direct", "ring"):
        t = 0.0  # the communicator's clock, from the start of backward
        for i, (off, n, b0, b1) in enumerate(spans):
            ready = (b1 + 1) * per_layer_bwd
            cost = wire_ms(float(reduce_elem_bytes) * n, model) * (1 if mode == "sharded" else 2)
            t = max(t, ready) + cost
            if model == "direct":
                out["spans"].append({"offset": off, "floats": n, "layers": [L1 - 1 - b1, L1 - 1 - b0], "ready_ms_into_backward": ready,
                                     "reduce_ms_direct": cost})
            else:
                out["spans"][i]["reduce_ms_ring"] = cost
        t += wire_ms(4.0 * tail, model) * 2  # vectors + scalar tail: all-reduced behind the last backward kernel
        exposed_reduce = max(0.0, t - bwd_ms)
        p_w = sum(n for _, n, _, _ in spans)
        if mode == "sharded":
            first_gather = wire_ms(float(gather_elem_bytes) * spans[-1][1], model) if spans else 0.0  # (layer 0's span: read first)
            all_gather = wire_ms(float(gather_elem_bytes) * p_w, model)
            # the remaining gathers run under the next forward pass; they show only if they outlast it
            exposed_gather = first_gather + max(0.0, (all_gather - first_gather) - fwd_ms)
            exposed_gather += twin_rebuild_ms
            adam = adam_ms / world
        else:
            exposed_gather, adam = 0.0, adam_ms
        out["exposed_ms_" + model] = {"reduce": exposed_reduce, "gather": exposed_gather}
        out["predicted_ms_per_step_" + model] = step_ms - adam_ms + adam + exposed_reduce + exposed_gather + fixed_ms
        if mode == "sharded" and twin_rebuild_ms > 0:
            # the alternative under the emulated arithmetic (round-5 verdict 1c): the shard owner's Adam writes the three planes
            # anyway -- gather THEM (6 B per weight instead of 4) and rebuild nothing; the fp32 masters then stay with their owner
            # as in mixed precision.  Same model, 1.5 x the gather bytes, no rebuild term
            fg = wire_ms(6.0 * spans[-1][1], model) if spans else 0.0
            ag = wire_ms(6.0 * p_w, model)
            eg = fg + max(0.0, (ag - fg) - fwd_ms)
            alt = step_ms - adam_ms + adam + exposed_reduce + eg + fixed_ms
            out.setdefault("plane_gather", {})["exposed_gather_ms_" + model] = eg
            out["plane_gather"]["predicted_ms_per_step_" + model] = alt
            out["plane_gather"]["gain_ms_" + model] = out["predicted_ms_per_step_" + model] - alt
    out["wire_bytes_per_rank_per_step"] = {
        "reduce_scatter_in_out" if mode == "sharded" else "all_reduce_in_out":
            float(reduce_elem_bytes) * p_w * (world - 1) / world * (1 if mode == "sharded" else 2),
        "all_gather_in_out": (float(gather_elem_bytes) * p_w * (world - 1) / world) if mode == "sharded" else 0.0,
        "tail_all_reduce": 8.0 * tail * (world - 1) / world}
    out["overlap_window_ms"] = bwd_ms - (out["spans"][0]["ready_ms_into_backward"] if out["spans"] else 0.0)
    out["single_rank"] = {"fwd_ms": fwd_ms, "bwd_ms": bwd_ms, "adam_ms": adam_ms, "step_ms": step_ms, "fixed_ms": fixed_ms,
                          "twin_rebuild_ms": twin_rebuild_ms}
    out["predicted_weak_scaling_efficiency_direct"] = step_ms / out["predicted_ms_per_step_direct"]
    if "plane_gather" in out:
        # break-even: the planes' extra wire time (half of the fp32 gather's exposed part) against the rebuild they save --
        # expressed as the all-gather rate per rank (bytes received / s) above which gathering planes wins
        first = spans[-1][1] if spans else 0
        extra_bytes = 2.0 * first * (world - 1) / world  # the exposed first span: 6 - 4 bytes per weight, from world - 1 peers
        out["plane_gather"]["break_even_gather_GBps_per_rank"] = (extra_bytes / (twin_rebuild_ms * 1e-3) / 1e9
                                                                  if twin_rebuild_ms > 0 else None)
        out["plane_gather"]["note"] = ("gather the owner-written three-plane twins (6 B per weight) instead of fp32 parameters (4 B) + a "
                                       "local rebuild (%.3f ms charged in full); wins when the exposed first-span gather runs faster "
                                       "than break_even_gather_GBps_per_rank and the rest still fits under the forward pass.  Built "
                                       "(TFK_DP_GATHER=planes, off by default until a multi-GPU run has measured it: bench.py's "
                                       "exchange_ab times both)" % twin_rebuild_ms)
    return out


def coalesced_spans(buckets, min_bytes):
    """the weight spans the coalescing rule of BucketReducer.on_bucket / csrc/exchange.hip cuts from the announcements
    W_L .. W_0: adjacent buckets are merged until a span carries >= min_bytes.  [(offset, floats, first bucket, last bucket)]"""
    L1 = len(buckets) - 2
    min_floats = max(1, int(min_bytes) // 4)
    spans, lo = [], None
    for b in range(L1):
        off, n = buckets[b]
        if lo is None:
            lo, hi, first = off, off + n, b
        elif off + n == lo:
            lo = off
        elif off == hi:
            hi = off + n
        else:
            spans.append((lo, hi - lo, first, b - 1))
            lo, hi, first = off, off + n, b
        if hi - lo >= min_floats:
            spans.append((lo, hi - lo, first, b))
            lo = None
    if lo is not None:
        spans.append((lo, hi - lo, first, L1 - 1))
    return spans


def exchange_timeline(buckets, world, fwd_ms, bwd_ms, adam_ms, step_ms, min_bytes=DEFAULT_BUCKET_MB << 20, rate_fraction=1.0, latency_ms=0.03,
                      gather_elem_bytes=4, reduce_elem_bytes=4, link_gbps=XGMI_LINK_GBPS, early_apply=False, record_ms=0.006):
    """exchange_model's question asked as a TIMELINE of the sharded step, with the two things that model leaves out: a fixed
    latency per collective, and the fact that a layer of the next forward pass waits for the WHOLE gather that covers it (so a
    span of five matrices holds its first layer back until the fifth has arrived).  It exists to choose the span size and to say
    what overlapping the optimiser with backward would buy, over a RANGE of wire rates -- no multi-GPU node was available to any
    round of this build, so the rate RCCL really reaches on the mesh is the unknown, not a constant.

    One communicator: its collectives run one after the other in launch order.  rate = rate_fraction x (world - 1) links x
    link_gbps per rank (1.0: every link at its peak; measured vendor collectives on such meshes reach roughly 0.3-0.6 of that at
    these sizes); a collective over B bytes per rank buffer costs latency_ms + B (world - 1) / world / rate.  Layer l's share of
    the forward / backward pass is proportional to its parameter count.  Backward announces W_L first; a span's reduce-scatter
    is launched when its lowest layer has been announced (the LAST span and the vectors: behind the last backward kernel, on the
    engine stream); every span launched under backward costs the engine stream record_ms of idle time.  Adam on the rank's
    1/world follows the last reduce (early_apply: each span's follows ITS reduce on the communicator's stream, and so does its
    gather -- the optimiser overlapped with backward, which is possible because mean -> clip -> Adam is element-wise once the
    frame count is known: reference trainer.py:174-184).  Gathers go lowest span first; the next forward pass starts layer l
    when the gather covering it is complete.  Returns the steady-state step time and where it went."""
    L1 = len(buckets) - 2
    spans = coalesced_spans(buckets, min_bytes)
    floats = [buckets[b][1] for b in range(L1)]            # announcement order: W_L .. W_0
    total = float(sum(floats))
    rate = rate_fraction * (world - 1) * link_gbps * 1e9   # bytes / s received (or sent) per rank

    def coll(nbytes):
        return latency_ms + (nbytes * (world - 1) / float(world)) / rate * 1e3 if world > 1 else 0.0

    # backward: bucket b (layer L - b) is announced at done_b
    done, t = [], 0.0
    for b in range(L1):
        t += bwd_ms * floats[b] / total
        done.append(t)
    comm = 0.0                      # the communicator's clock, from the start of backward
    reduce_end, gather_end_early = {}, {}
    engine_idle = 0.0
    for i, (off, n, b0, b1) in enumerate(spans):
        last = i == len(spans) - 1
        ready = bwd_ms if last else done[b1]
        if not last:
            engine_idle += record_ms
        comm = max(comm, ready) + coll(float(reduce_elem_bytes) * n)
        reduce_end[i] = comm
        if early_apply and not last:
            comm += adam_ms * n / total / world
            comm += coll(float(gather_elem_bytes) * n)
            gather_end_early[i] = comm
    tail_end = comm + (latency_ms if world > 1 else 0.0)  # vectors + scalars: one small grouped all-reduce behind the last reduce-scatter
    exposed_reduce = max(0.0, tail_end - bwd_ms)
    # optimiser: everything (apply at the end) or what early_apply left (the last span + the vectors)
    if early_apply:
        adam = adam_ms * spans[-1][1] / total / world if spans else 0.0
    else:
        adam = adam_ms / world
    t0 = max(bwd_ms, tail_end) + adam + engine_idle      # the next forward pass may start here (if its first gather allows)
    # gathers, lowest span first
    g, gather_end = t0, {}
    for i in reversed(range(len(spans))):
        if i in gather_end_early:
            gather_end[i] = gather_end_early[i]
            continue
        g += coll(float(gather_elem_bytes) * spans[i][1])
        gather_end[i] = g
    # next forward pass: layer l = bucket L - l; layer of bucket b is covered by the span holding b
    span_of = {}
    for i, (off, n, b0, b1) in enumerate(spans):
        for b in range(b0, b1 + 1):
            span_of[b] = i
    f = t0
    waited = 0.0
    for b in reversed(range(L1)):   # W_0 first
        start = max(f, gather_end[span_of[b]])
        waited += start - f
        f = start + fwd_ms * floats[b] / total
    other = step_ms - fwd_ms - bwd_ms - adam_ms   # what a single-rank step spends outside the three (loss hand-over, launches)
    predicted = (f - t0) + bwd_ms + (t0 - bwd_ms) + other
    return {"world": world, "min_span_bytes": int(min_bytes), "spans": len(spans), "rate_fraction": rate_fraction,
            "GBps_per_rank": rate / 1e9, "latency_ms": latency_ms, "early_apply": bool(early_apply),
            "exposed_reduce_ms": exposed_reduce, "adam_ms": adam, "gather_wait_ms": waited, "engine_idle_ms": engine_idle,
            "predicted_ms_per_step": predicted, "predicted_weak_scaling_efficiency": step_ms / predicted}


def exchange_timeline_sweep(buckets, world, fwd_ms, bwd_ms, adam_ms, step_ms, early=(False,), **kw):
    """exchange_timeline over span sizes x wire rates x per-collective latencies x (apply at the end | optimiser under backward):
    {"span_MiB/rate_fraction/latency_us[/early]": predicted ms per step}, and per (rate, latency) the best span size"""
    table, best = {}, {}
    for rate in (1.0, 0.5, 0.3):
        for lat in (0.015, 0.04):
            for early_apply in early:
                row = {}
                for mib in (16, 32, 64, 128):
                    r = exchange_timeline(buckets, world, fwd_ms, bwd_ms, adam_ms, step_ms, min_bytes=mib << 20, rate_fraction=rate,
                                          latency_ms=lat, early_apply=early_apply, **kw)
                    key = "%d/%.1f/%d%s" % (mib, rate, round(lat * 1e3), "/early" if early_apply else "")
                    table[key] = r["predicted_ms_per_step"]
                    row[mib] = r["predicted_ms_per_step"]
                best["%.1f/%d%s" % (rate, round(lat * 1e3), "/early" if early_apply else "")] = min(row, key=row.get)
    return {"ms_per_step": table, "best_span_MiB": best,
            "key": "span MiB / fraction of (world - 1) x %.0f GB/s per rank / latency per collective in us [/ optimiser under backward]"
                   % kw.get("link_gbps", XGMI_LINK_GBPS)}


class DataParallel(object):
    """Shards the micro-batches of one optimiser step over the ranks of a process group."""

    def __init__(self, group=None, mode=None):
        self.group = group
        self.mode = mode  # exchange step of BucketReducer (None: TFK_DP_EXCHANGE or "sharded")
        self.rank, self.world = 0, 1
        self._forced = False
        # one BucketReducer per engine: it carries the in-flight parameter gathers across steps.  Keyed weakly (and
        # dropped by Engine.close): a later engine that happens to get the same id() must not inherit views into a
        # closed engine's state.
        self._reducers = weakref.WeakKeyDictionary()
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
                self._forced = os.environ.get("TFK_FORCE_DP") == "1"
        except ImportError:
            pass

    @property
    def enabled(self):
        return self.world > 1 or self._forced

    @staticmethod
    def _stream_ctx(engine):
        stream = getattr(engine, "torch_stream", None)
        if stream is None:
            return contextlib.nullcontext()
        import torch
        return torch.cuda.stream(stream)

    def reducer(self, engine):
        """the engine's BucketReducer; created on first use -- COLLECTIVELY (it probes the backend), i.e. at the same
        point of the program on every rank, which the first train_step is"""
        r = self._reducers.get(engine)
        if r is None:
            ref = weakref.ref(engine)
            r = self._native_exchange(engine) if self._native(engine) else None
            if r is None:
                r = BucketReducer(engine, self.group, stream_ctx=lambda: self._stream_ctx(ref()), mode=self.mode)
                r.fallback_reason = self.native_failure
            self._reducers[engine] = r
            if hasattr(engine, "on_close"):
                engine.on_close.append(lambda: self._forget(ref()))
        return r

    def _native(self, engine):
        """RCCL from inside the library (csrc/exchange.hip) whenever the process group runs on RCCL and the engine is a real
        one; TFK_DP_COMM=torch keeps the exchange in BucketReducer over torch.distributed (gloo groups always do)"""
        want = os.environ.get("TFK_DP_COMM", "native")
        if want not in ("native", "native-only", "torch"):
            raise ValueError("TFK_DP_COMM=%r (native | native-only | torch)" % want)
        if want == "torch" or not hasattr(getattr(engine, "lib", None), "tfk_comm_create"):
            return False
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_backend(self.group) == "nccl"

    native_failure = None  # why the in-library exchange was given up (None: it was not)

    def _native_exchange(self, engine):
        """NativeExchange, or None when ANY rank cannot bring it up (RCCL not loadable from the library, engine or mode
        refused, communicator refused): everyone then runs BucketReducer over torch.distributed, and the reason goes to stderr
        and into bench.py's `exchange_driver` -- a job that would otherwise die at its first step keeps running on the slower
        driver, and says so.  TFK_DP_COMM=native-only makes the failure fatal instead.

        Two agreements over the process group that is already up, in this order: (1) BEFORE anything collective of RCCL's --
        every rank probes locally (`tfk_comm_available`: no other rank is involved) and the answers are MIN-reduced; only if
        every rank can go on does rank 0 make the unique id and everyone enter `tfk_comm_create` (ncclCommInitRank blocks
        until all ranks have arrived: a rank that failed earlier would leave the others waiting there for ever -- round 4
        announced rank 0's failures only); (2) after it, the outcome of the creation itself."""
        import torch
        import torch.distributed as dist
        from . import _lib
        on_gpu = dist.get_backend(self.group) == "nccl"

        def agree(flag):
            ok = torch.tensor([1 if flag else 0], dtype=torch.int32)
            if on_gpu:
                ok = ok.cuda(engine.cfg.device)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=self.group)
            return int(ok.item()) == 1

        r, err = None, None
        mode = self.mode or os.environ.get("TFK_DP_EXCHANGE", "sharded")
        try:
            if mode not in _lib.EXCHANGE:
                raise ValueError("exchange mode %r" % (mode,))
            _lib.check(engine.lib.tfk_comm_available(engine._h, _lib.EXCHANGE[mode]))
        except Exception as e:  # noqa: BLE001 (whatever it was, the other ranks must hear of it)
            err = "%s: %s" % (type(e).__name__, e)
        if agree(err is None):
            try:
                r = NativeExchange(engine, self.group, mode=self.mode)
            except Exception as e:  # noqa: BLE001
                err = "%s: %s" % (type(e).__name__, e)
            if agree(r is not None):
                return r
        if r is not None:
            engine.on_close.remove(r.close)
            engine.param_access_hook = None
            r.close()
        self.native_failure = err or "another rank could not bring the in-library exchange up"
        if os.environ.get("TFK_DP_COMM") == "native-only":
            raise RuntimeError("in-library exchange unavailable: %s" % self.native_failure)
        import sys
        sys.stderr.write("tfkaldi_amd: WARNING in-library RCCL exchange unavailable on rank %d (%s); this job runs the exchange "
                         "through torch.distributed (dataparallel.BucketReducer)\n" % (self.rank, self.native_failure))
        return None

    def _forget(self, engine):
        if engine is not None:
            r = self._reducers.pop(engine, None)
            if r is not None:
                r.drain()

    def drain(self, engine):
        """wait (on the engine's stream) for parameter all-gathers still in flight: before the engine is closed or its
        state tensor is read behind the engine's back"""
        r = self._reducers.get(engine)
        if r is not None:
            r.drain()

    def gather_parameters(self, engine):
        """COLLECTIVE (every rank must call it): make the fp32 parameters whole on every rank.  Only the mixed-precision
        sharded exchange leaves them sharded (each rank keeps the masters of its own spans; all ranks share the bf16
        shadow the forward pass reads); everywhere else this only waits for the gathers in flight.  Call it before
        checkpointing, tensor get / set, or handing the engine to code that reads parameters."""
        r = self._reducers.get(engine)
        if r is not None:
            r.gather_masters(engine)
            r.drain()

    def train_step(self, engine, microbatches):
        """`microbatches`: the (X[T, F], y[T]) micro-batches of the WHOLE step, identical on every rank.
        Returns the average loss over all of them (reference Trainer.update's return value)."""
        if not self.enabled:
            return self.train_own(engine, microbatches, 0)
        start, end = partition(len(microbatches), self.world)[self.rank]
        return self.train_own(engine, microbatches[start:end], len(microbatches) - end)

    def train_own(self, engine, mine, later, overlap=None):
        """One optimiser step from THIS rank's micro-batches only (`later` = micro-batches of the step that belong to
        higher ranks: the BN moving averages compose in the reference's serial order).  `overlap`, if given, is called once
        the WHOLE step is enqueued -- micro-batches, tail collectives, optimiser, parameter gathers -- and before the host
        waits for its loss: the place for host work that should run while the GPU is busy (the dispenser's prefetch of the
        next batch).  What it raises is re-raised after the step has completed (under data parallelism the peers are waiting
        in collectives this rank must still take part in)."""
        if not self.enabled:
            for i, mb in enumerate(mine):
                _accumulate(engine, mb, i == len(mine) - 1)
            if overlap is None or not hasattr(engine, "apply_enqueue"):
                failed = _run_overlap(overlap)
                loss = engine.apply()
            else:
                engine.apply_enqueue()
                failed = _run_overlap(overlap)
                loss = engine.apply_end()
            if failed is not None:
                raise failed
            return loss
        engine.set_later_microbatches(later)
        reducer = self.reducer(engine)
        reducer.begin_step(engine)
        try:
            for i, mb in enumerate(mine):
                _accumulate(engine, mb, i == len(mine) - 1)
            if not mine:  # more ranks than micro-batches: this rank contributes zeros
                reducer.idle(engine)
        finally:
            reducer.end_step(engine)
        loss = reducer.finish_and_apply(engine, overlap)
        self.last_collectives = reducer.last_launched
        self.last_kinds = reducer.last_kinds
        self.last_executed = reducer.last_executed  # names of the torch.distributed calls that really ran
        return loss

    def eval_step(self, engine, microbatches):
        """average validation loss (reference Trainer.evaluate); only the scalar tail is reduced"""
        if not self.enabled:
            return self.eval_own(engine, microbatches)
        start, end = partition(len(microbatches), self.world)[self.rank]
        return self.eval_own(engine, microbatches[start:end])

    def label_errors(self, engine, microbatches, beam_width=None, lm=None, label_topk=None, rescore_paths=None):
        """(edits, reference labels): label errors summed over the CTC micro-batches of the WHOLE batch (identical on every
        rank) under best-path decoding (beam_width None) or the best path of a prefix beam search of that width (lm: an
        NgramLM or GraphLM the search ranks its prefixes with; label_topk: an int prunes the search to the frame's label_topk most
        probable labels, for models of any output size; rescore_paths: an int N re-ranks the search's N best by their exact
        scores (ctc_score + ctc_rerank, lm honoured) and counts the new best; every rank passes the same ones).
        COLLECTIVE when enabled: each rank decodes its block of micro-batches (partitioned as eval_step) and the two counts
        are SUM all-reduced as one int64 tensor over self.group (on the device for an NCCL / RCCL group)."""
        mine = microbatches
        if self.enabled:
            start, end = partition(len(microbatches), self.world)[self.rank]
            mine = microbatches[start:end]
        edits = labels = 0
        for mb in mine:
            e, n = _label_errors(engine, mb, beam_width, lm, label_topk, rescore_paths)
            edits += e
            labels += n
        if not self.enabled:
            return edits, labels
        import torch
        import torch.distributed as dist
        counts = torch.tensor([edits, labels], dtype=torch.int64)
        if dist.get_backend(self.group) == "nccl":
            counts = counts.cuda(engine.cfg.device)
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.group)
        counts = counts.cpu()
        return int(counts[0]), int(counts[1])

    def eval_own(self, engine, mine):
        """validation loss from THIS rank's micro-batches (all of them in a single-process run)"""
        _eval_accumulate_all(engine, mine)
        if not self.enabled:
            return engine.eval_finish()
        if not mine:  # nothing on this rank: contribute physical zeros (the accumulators reset lazily)
            engine.zero_accumulators()
        return self.reducer(engine).eval_finish(engine, self)
