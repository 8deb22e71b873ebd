"""Streaming CTC decoding on the device (tfk_ctc_stream_*, csrc/ctc.hip): whatever way a lane's frames are cut into pushes, the
result is the one-shot search's on the frames so far -- tfk_ctc_beam_logits / _lm_logits / _graph_logits / _topk_logits with the
same beam width, model, weight, bonus and flags on the SAME logits -- in labels, lengths and the bit patterns of score and
am_score.  Nothing here has a tolerance: the one-shot entries are themselves tested against the float64 restatement
(tests/test_gpu_ctc_beam*.py).  One line is printed per case (profiles/ctc_stream_edges.txt is such a run's table).

Shapes: dense (O, W) = (4, 1), (9, 8), (64, 128) -- one slot, a few, the full key table; pruned (O, K, W) = (9, 3, 8), (300, 5, 16)
-- K < O - 1 below and above 64 outputs.  Three lanes of 37, 20 and 0 frames, so that every push mixes lanes that move, lanes that
have ended and a lane that never gets a frame."""
from ctypes import byref, c_float, c_void_p

import numpy as np
import pytest

from util import make_pair

from tfkaldi_amd import _lib
from tfkaldi_amd.neuralNetworks.ctc_lm import GraphLM, NgramLM
from tfkaldi_amd.processing.feature_reader import StreamSplicer, splice

pytestmark = pytest.mark.gpu

LENS = (37, 20, 0)
KW = dict(input_dim=20, num_layers=2, num_units=32, output_dim=9, nonlin="tanh", batch_norm=True,
          init_learning_rate=1e-3, num_steps=50)


# ---- models, logits, schedules ----

def _log_softmax(x):
    x = x - x.max(axis=1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)


def _model(kind, O, seed=3, eos=False):
    rng = np.random.default_rng(seed)
    if kind == "am":
        return None
    if kind == "ngram":
        return NgramLM(_log_softmax(1.5 * rng.standard_normal((O, O))), 2, weight=0.6, label_bonus=0.4, end_of_sequence=eos)
    # a lexicon: most arcs are missing, and only word ends are final
    L = O - 1
    sep = L - 1
    words = {tuple(int(c) for c in rng.integers(0, max(sep, 1), size=n)) for n in (1, 2, 2, 3, 3, 4) for _ in range(3)}
    words = [np.array(w) for w in sorted(words)] if sep > 0 else [np.array([0])]
    return GraphLM.from_lexicon(words, L, separator=sep if sep > 0 else None, word_logprob=-0.3 * np.arange(len(words)),
                                weight=0.7, label_bonus=0.2, end_of_sequence=eos)


def _logits(kind, O, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return [(2.0 * rng.standard_normal((n, O))).astype(np.float32) for n in LENS]
    return [rng.integers(-2, 3, size=(n, O)).astype(np.float32) for n in LENS]  # ties in most frames


def _schedules():
    """name -> list of pushes, a push = the chunk length of every lane"""
    def pair(c0):  # lane 1 follows lane 0's cut positions until its own frames run out
        out, done = [], [0, 0]
        for c in c0:
            c1 = min(c, LENS[1] - done[1])
            out.append([c, c1, 0])
            done[0] += c
            done[1] += c1
        assert done == [LENS[0], LENS[1]]
        return out
    rng = np.random.default_rng(11)
    cuts = sorted(rng.integers(0, LENS[0] + 1, size=5).tolist())
    sizes = np.diff([0] + cuts + [LENS[0]]).tolist()
    random = [0]
    for s in sizes:
        random += [s, 0]
    step, done1 = [], 0
    for i, c in enumerate([5] * 7 + [2]):  # lane 1 idles on every second push and catches up in larger chunks
        c1 = 0 if i % 2 else min(9, LENS[1] - done1)
        done1 += c1
        step.append([c, c1, 0])
    assert done1 == LENS[1] and sum(p[0] for p in step) == LENS[0]
    return {"one chunk": pair([LENS[0]]), "37 x 1": pair([1] * LENS[0]), "[1, 36]": pair([1, 36]), "[36, 1]": pair([36, 1]),
            "random + empty": pair(random), "out of step": step}


# ---- the device: the one-shot entries and a stream ----

_tables = {}


def _dev_tables(lm):
    """(weight / table, next or None) on the device, kept for the module's lifetime (a lane's binding names their addresses)"""
    import torch
    if id(lm) not in _tables:
        nxt = getattr(lm, "next", None)
        _tables[id(lm)] = (lm, torch.from_numpy(np.ascontiguousarray(lm.table, dtype=np.float32)).cuda(),
                           None if nxt is None else torch.from_numpy(np.ascontiguousarray(nxt, dtype=np.int32)).cuda())
    return _tables[id(lm)][1:]


def _oneshot(zs, W, P, lm, eos=False, K=0):
    """the matching one-shot entry on the utterances zs: (hyps[u][n], score bits [U, P], am_score bits [U, P] or None)"""
    import torch
    lib = _lib.load()
    utt = [z.shape[0] for z in zs]
    O = zs[0].shape[1]
    z = np.ascontiguousarray(np.concatenate(zs), dtype=np.float32)
    T, U = z.shape[0], len(utt)
    seg = np.concatenate([[0], np.cumsum(utt)]).astype(np.int32)
    d_z, d_seg = torch.from_numpy(z).cuda(), torch.from_numpy(seg).cuda()
    hyp = torch.full((P, max(T, 1)), -7, dtype=torch.int32, device="cuda")
    hyp_len = torch.full((P, U), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    am = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    st = c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (st, c_void_p(d_z.data_ptr()), O, O, T, c_void_p(d_seg.data_ptr()), U, W, P)
    outs = (c_void_p(hyp.data_ptr()), c_void_p(hyp_len.data_ptr()), c_void_p(score.data_ptr()))
    flags = _lib.CTC_LM_EOS if eos else 0
    has_am = True
    if lm is None:
        if K:
            _lib.check(lib.tfk_ctc_beam_topk_logits(*head, K, c_void_p(None), 0, c_float(0), c_float(0), 0, *outs, c_void_p(am.data_ptr())))
        else:
            has_am = False
            _lib.check(lib.tfk_ctc_beam_logits(*head, *outs))
    else:
        d_w, d_n = _dev_tables(lm)
        model = (c_float(lm.weight), c_float(lm.label_bonus), flags, *outs, c_void_p(am.data_ptr()))
        if d_n is not None:
            _lib.check(lib.tfk_ctc_beam_graph_logits(*head, K, c_void_p(d_w.data_ptr()), c_void_p(d_n.data_ptr()), lm.num_states,
                                                     lm.start, *model))
        elif K:
            _lib.check(lib.tfk_ctc_beam_topk_logits(*head, K, c_void_p(d_w.data_ptr()), lm.order, *model))
        else:
            _lib.check(lib.tfk_ctc_beam_lm_logits(*head, c_void_p(d_w.data_ptr()), lm.order, *model))
    torch.cuda.synchronize()
    hyp, hyp_len, score, am = hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy(), am.cpu().numpy()
    hyps = [[hyp[n, seg[u]:seg[u] + hyp_len[n, u]].copy() for n in range(P)] for u in range(U)]
    return hyps, score.T.copy().view(np.uint32), am.T.copy().view(np.uint32) if has_am else None


class _Stream(object):
    """tfk_ctc_stream_* on host logits, on torch's current stream"""

    def __init__(self, O, lanes, W, max_frames, K=0):
        import torch
        self.lib = _lib.load()
        self.lanes, self.O = lanes, O
        self.st = c_void_p(torch.cuda.current_stream().cuda_stream)
        self.h = c_void_p()
        _lib.check(self.lib.tfk_ctc_stream_create(O, lanes, W, max_frames, K, byref(self.h)))

    def push_rc(self, chunks, lm, O=None, chunk_len=None, T=None):
        """chunks: the rows of every lane's chunk; returns the entry's return code"""
        import torch
        rows = np.ascontiguousarray(np.concatenate(chunks), dtype=np.float32).reshape(-1, O or self.O)
        lens = np.array([c.shape[0] for c in chunks] if chunk_len is None else chunk_len, dtype=np.int32)
        d_z = torch.from_numpy(rows).cuda() if rows.shape[0] else torch.zeros(1, device="cuda")
        args = (c_void_p(None), 0, c_void_p(None), 0, 0, c_float(0), c_float(0))
        if lm is not None:
            d_w, d_n = _dev_tables(lm)
            args = (c_void_p(d_w.data_ptr()), getattr(lm, "order", 0), c_void_p(None if d_n is None else d_n.data_ptr()),
                    getattr(lm, "num_states", 0) if d_n is not None else 0, lm.start if d_n is not None else 0,
                    c_float(lm.weight), c_float(lm.label_bonus))
        return self.lib.tfk_ctc_stream_push_logits(self.h, self.st, c_void_p(d_z.data_ptr()), rows.shape[1],
                                                   rows.shape[0] if T is None else T, lens.ctypes.data_as(c_void_p), *args)

    def push(self, chunks, lm):
        _lib.check(self.push_rc(chunks, lm))

    def result_rc(self, P, eos=False, cap=None):
        cap = max(int(self.frames().max()), 1) if cap is None else cap
        hyp = np.full((P, self.lanes, max(cap, 1)), -7, dtype=np.int32)
        hyp_len = np.full((P, self.lanes), -7, dtype=np.int32)
        score = np.zeros((P, self.lanes), dtype=np.float32)
        am = np.zeros((P, self.lanes), dtype=np.float32)
        rc = self.lib.tfk_ctc_stream_result(self.h, self.st, P, _lib.CTC_LM_EOS if eos else 0, hyp.ctypes.data_as(c_void_p), cap,
                                            hyp_len.ctypes.data_as(c_void_p), score.ctypes.data_as(c_void_p),
                                            am.ctypes.data_as(c_void_p))
        return rc, hyp, hyp_len, score, am

    def result(self, P, eos=False):
        rc, hyp, hyp_len, score, am = self.result_rc(P, eos)
        _lib.check(rc)
        for n in range(P):  # the entries past a hypothesis are -1
            for l in range(self.lanes):
                assert np.all(hyp[n, l, hyp_len[n, l]:] == -1)
        hyps = [[hyp[n, l, :hyp_len[n, l]].copy() for n in range(P)] for l in range(self.lanes)]
        return hyps, score.T.copy().view(np.uint32), am.T.copy().view(np.uint32)

    def reset(self, lane=-1):
        _lib.check(self.lib.tfk_ctc_stream_reset(self.h, self.st, lane))

    def frames(self):
        out = np.zeros(self.lanes, dtype=np.int32)
        _lib.check(self.lib.tfk_ctc_stream_frames(self.h, out.ctypes.data_as(c_void_p)))
        return out

    def close(self):
        import torch
        torch.cuda.synchronize()
        _lib.check(self.lib.tfk_ctc_stream_destroy(self.h))


def _same(got, want, what):
    """labels and lengths exactly, scores (and the acoustic scores, where the one-shot entry reports them) by their bits"""
    hyps, score, am = got
    w_hyps, w_score, w_am = want
    assert len(hyps) == len(w_hyps), what
    for l, (a, b) in enumerate(zip(hyps, w_hyps)):
        for n, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y), (what, "lane", l, "path", n, x, y)
    assert np.array_equal(score, w_score), (what, score, w_score)
    if w_am is not None:
        assert np.array_equal(am, w_am), (what, am, w_am)
    else:
        assert np.array_equal(am, score), what  # without a model the acoustic score is the score


def _run(st, zs, pushes, lm, after_push=None):
    at = [0] * len(zs)
    for i, push in enumerate(pushes):
        st.push([zs[l][at[l]:at[l] + c] for l, c in enumerate(push)], lm)
        at = [a + c for a, c in zip(at, push)]
        if after_push:
            after_push(i, list(at))
    return at


DENSE = [(4, 0, 1), (9, 0, 8), (64, 0, 128)]
PRUNED = [(9, 3, 8), (300, 5, 16)]
CASES = [(O, K, W, m) for O, K, W in DENSE for m in ("am", "ngram", "graph")] + \
        [(O, K, W, m) for O, K, W in PRUNED for m in ("am", "ngram")]


# ---- A. any chunking equals one search ----
@pytest.mark.parametrize("O,K,W,kind", CASES)
def test_any_chunking_equals_one_search(gpu, O, K, W, kind):
    P = min(W, 5)
    lm = _model(kind, O)
    flags = (False, True) if lm is not None else (False,)
    st = _Stream(O, len(LENS), W, max(LENS), K)
    for logit_kind in ("gauss", "integer"):
        zs = _logits(logit_kind, O, 5 + O)
        want = {eos: _oneshot(zs, W, P, lm, eos, K) for eos in flags}
        assert any(h[0].size for h in want[False][0]) or kind == "graph"
        for name, pushes in _schedules().items():
            st.reset()
            assert _run(st, zs, pushes, lm) == list(LENS) and st.frames().tolist() == list(LENS)
            for eos in flags:
                _same(st.result(P, eos), want[eos], (O, K, W, kind, logit_kind, name, eos))
            print("A O=%d K=%d W=%d %-5s %-7s %-14s %2d pushes: labels, lengths, score bits equal the one-shot search%s"
                  % (O, K, W, kind, logit_kind, name, len(pushes), " (with and without the end term)" if lm is not None else ""))
    st.close()


# ---- B. partial results ----
@pytest.mark.parametrize("O,K,W,kind", [(9, 0, 8, "ngram"), (64, 0, 128, "am"), (9, 3, 8, "am"), (9, 0, 8, "graph")])
def test_partial_results_equal_the_search_so_far(gpu, O, K, W, kind):
    P = min(W, 5)
    lm = _model(kind, O)
    eos = lm is not None
    zs = _logits("integer", O, 21)
    # every prefix of every lane as one batch of utterances: ONE one-shot call gives what every partial result must be
    index, prefixes = {}, []
    for l, z in enumerate(zs):
        for t in range(z.shape[0] + 1):
            index[(l, t)] = len(prefixes)
            prefixes.append(z[:t])
    h, s, a = _oneshot(prefixes, W, P, lm, eos, K)
    pushes = _schedules()["out of step"]
    st = _Stream(O, len(LENS), W, max(LENS), K)

    def check(i, at):
        got = st.result(P, eos)
        again = st.result(P, eos)
        rows = [index[(l, t)] for l, t in enumerate(at)]
        _same(got, ([h[r] for r in rows], s[rows], None if a is None else a[rows]), (O, K, W, kind, "after push", i, at))
        _same(again, got, "two results in a row")
    _run(st, zs, pushes, lm, check)
    final = st.result(P, eos)
    st.reset()
    _run(st, zs, pushes, lm)
    _same(st.result(P, eos), final, "a run that never asked")
    print("B O=%d K=%d W=%d %-5s: %d partial results equal the search of the frames so far; asking changes nothing"
          % (O, K, W, kind, len(pushes)))
    st.close()


# ---- C. reset ----
def test_reset_of_one_lane(gpu):
    O, W, P = 9, 8, 5
    lm, other = _model("ngram", O), _model("graph", O)
    zs, ys = _logits("gauss", O, 31), _logits("integer", O, 32)
    st = _Stream(O, len(LENS), W, max(LENS))
    # lane 0 takes 11 frames of ys, is reset, and decodes zs[0] from the start; lanes 1 and 2 run through undisturbed
    st.push([ys[0][:11], zs[1][:7], zs[2]], lm)
    st.reset(0)
    assert st.frames().tolist() == [0, 7, 0]
    st.push([zs[0][:30], zs[1][7:], zs[2]], lm)
    st.push([zs[0][30:], zs[1][:0], zs[2]], lm)
    _same(st.result(P, True), _oneshot(zs, W, P, lm, True), "lane 0 reset in mid-utterance and reused")
    print("C a lane reset in mid-utterance and reused equals a fresh stream; the other lanes are unaffected")
    # after a reset of every lane the stream binds to another model
    st.reset()
    _run(st, zs, _schedules()["[1, 36]"], other)
    _same(st.result(P, True), _oneshot(zs, W, P, other, True), "bound to a graph after the reset")
    # and a lane that only ever received empty chunks under one model takes another: lane 2 here, with every lane at 0 frames
    st.reset()
    st.push([z[:0] for z in zs], lm)
    _run(st, zs, _schedules()["[36, 1]"], None)
    _same(st.result(P), _oneshot(zs, W, P, None), "zero-frame binding replaced")
    print("C after a reset a lane binds to a different model (n-gram -> graph -> none)")
    st.close()


# ---- D. refusals ----
def test_refusals_leave_the_stream_as_it_was(gpu):
    O, W, P = 9, 8, 5
    lm, other = _model("ngram", O), _model("ngram", O, seed=4)
    zs = _logits("gauss", O, 41)
    st = _Stream(O, len(LENS), W, 30)
    lib = st.lib
    rc, *_ = st.result_rc(P, eos=True)
    assert rc != 0 and b"TFK_CTC_LM_EOS, and lane 0 is not bound to a model" in lib.tfk_last_error()
    st.push([zs[0][:25], zs[1][:20], zs[2]], lm)
    before = st.result(P, True)

    def refused(rc, *parts):
        msg = lib.tfk_last_error()
        assert rc != 0 and all(p in msg for p in parts), (rc, msg)
        assert st.frames().tolist() == [25, 20, 0]
        _same(st.result(P, True), before, msg)
        print("D refused: %s" % msg.decode())
    refused(st.push_rc([zs[0][25:31], zs[1][:0], zs[2]], lm), b"lane 0 would hold 31 frames (max_frames 30)")
    refused(st.push_rc([zs[0][25:27], zs[1][:0], zs[2]], other), b"lane 0 holds 25 frames decoded with an n-gram table")
    refused(st.push_rc([zs[0][25:27], zs[1][:0], zs[2]], None), b"lane 0 holds 25 frames", b"no model")
    refused(st.push_rc([zs[0][25:27], zs[1][:0], zs[2]], lm, chunk_len=[1, 0, 0]), b"the chunk lengths sum to 1, expected T = 2")
    refused(st.push_rc([zs[0][25:27], zs[1][:0], zs[2]], lm, chunk_len=[3, -1, 0]), b"lane 1 has a negative chunk length")
    refused(lib.tfk_ctc_stream_push_logits(st.h, st.st, c_void_p(None), O, 0, c_void_p(None), c_void_p(None), 0, c_void_p(None),
                                           0, 0, c_float(0), c_float(0)), b"chunk_len is NULL")
    rc, *_ = st.result_rc(W + 1)
    refused(rc, b"top_paths 9 outside [1, beam_width = 8]")
    rc, *_ = st.result_rc(1, cap=-1)
    refused(rc, b"hyp_cap -1 < 0")
    st.push([zs[0][25:30], zs[1][:0], zs[2]], lm)  # the stream goes on from where it was
    _same(st.result(P, True), _oneshot([zs[0][:30], zs[1], zs[2]], W, P, lm, True), "after the refusals")
    st.close()
    # a wrong output_dim: the engine's differs from the stream's
    eng, _ = make_pair(np.random.default_rng(5), max_frames=64, **KW)
    handle = c_void_p()
    _lib.check(lib.tfk_ctc_stream_create(KW["output_dim"] + 1, 1, W, 30, 0, byref(handle)))
    X = np.zeros((4, KW["input_dim"]), dtype=np.float32)
    rc = lib.tfk_ctc_stream_push(eng._h, handle, X.ctypes.data_as(c_void_p), X.shape[1], 4, np.array([4], np.int32).ctypes.data_as(c_void_p),
                                 c_float(0), c_float(0), 0)
    assert rc != 0 and b"output_dim 9 differs from the stream's O = 10" in lib.tfk_last_error()
    print("D refused: %s" % lib.tfk_last_error().decode())
    frames = np.ones(1, dtype=np.int32)
    _lib.check(lib.tfk_ctc_stream_frames(handle, frames.ctypes.data_as(c_void_p)))
    assert frames[0] == 0
    _lib.check(lib.tfk_ctc_stream_destroy(handle))
    eng.close()
    for args, part in (((9, 0, 8, 30, 0), b"lanes 0 outside [1, 1024]"), ((65, 1, 8, 30, 0), b"output_dim 65 outside [2, 64]"),
                       ((9, 1, 8, 0, 0), b"max_frames 0 outside [1, 524286]"), ((9, 1, 129, 30, 0), b"beam_width 129 outside [1, 128]"),
                       ((9, 1, 8, 30, 64), b"label_topk 64 outside [0, 63]")):
        assert lib.tfk_ctc_stream_create(*args, byref(handle)) != 0 and part in lib.tfk_last_error(), (args, lib.tfk_last_error())


# ---- E. the table of a lane filled to max_frames ----
def test_full_table(gpu):
    O, W, P, T = 64, 128, 5, 64
    z = (0.01 * np.random.default_rng(51).standard_normal((T + 1, O))).astype(np.float32)  # near-uniform: new prefixes win slots
    want = _oneshot([z[:T]], W, P, None)
    st = _Stream(O, 1, W, T)
    for chunk in (T, 7):
        st.reset()
        for t in range(0, T, chunk):
            st.push([z[t:min(t + chunk, T)]], None)
        got = st.result(P)
        _same(got, want, ("full table", chunk))
        assert st.push_rc([z[T:]], None) != 0 and b"lane 0 would hold 65 frames (max_frames 64)" in st.lib.tfk_last_error()
        _same(st.result(P), got, "after the refused frame 65")
    print("E max_frames = 64 frames at O = 64, W = 128 (best path %d labels): equals the one-shot search in chunks of 64 and 7; "
          "frame 65 is refused" % want[0][0][0].size)
    st.close()


# ---- F. through the engine and the Decoder ----
def _decoder(eng, max_length):
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    dec = Decoder.__new__(Decoder)  # (the Decoder's methods on a toy engine: no model files)
    dec.engine, dec.max_length = eng, max_length
    return dec


@pytest.mark.parametrize("with_lm", [False, True])
def test_through_the_engine(gpu, with_lm):
    rng = np.random.default_rng(61)
    eng, _ = make_pair(np.random.default_rng(5), max_frames=256, **KW)
    dec = _decoder(eng, 256)
    O, c, W, P = KW["output_dim"], 2, 8, 5
    D = KW["input_dim"] // (2 * c + 1)
    lm = _model("ngram", O, eos=True) if with_lm else None
    xs = [(1.5 * rng.standard_normal((n, D))).astype(np.float32) for n in (50, 33)]
    # unspliced chunks of 7 and 5 frames; the reference splices the same chunks and takes the logits of the same row batches
    stream = dec.ctc_stream(lanes=2, beam_width=W, max_frames=64, lm=lm, context_width=c)
    mirror = [StreamSplicer(D, c) for _ in xs]
    zs = [[], []]

    def logits_of(rows):
        flat = np.concatenate(rows)
        if flat.shape[0]:
            z = eng.posteriors(flat, raw_logits=True)
            for l, part in enumerate(np.split(z, np.cumsum([r.shape[0] for r in rows])[:-1])):
                zs[l].append(part.copy())
    at = [0, 0]
    while at[0] < 50 or at[1] < 33:
        chunks = [xs[0][at[0]:at[0] + 7], xs[1][at[1]:at[1] + 5] if at[1] < 33 else None]
        stream.push(chunks)
        logits_of([m.push(ch) if ch is not None else np.zeros((0, KW["input_dim"]), np.float32) for m, ch in zip(mirror, chunks)])
        at = [at[0] + 7, at[1] + 5]
    got = []
    for lane in range(2):
        got.append(stream.finish(lane, top_paths=P))
        logits_of([m.flush() if l == lane else np.zeros((0, KW["input_dim"]), np.float32) for l, m in enumerate(mirror)])
    assert stream.frames().tolist() == [50, 33]
    want = _oneshot([np.concatenate(z) for z in zs], W, P, lm, with_lm)
    # lane 0's final result was taken before lane 1's tail was pushed: lane 0 did not move in between
    hyps = [got[0][0], got[1][0]]
    score = np.stack([got[0][1], got[1][1]]).view(np.uint32)
    am = np.stack([g[2] for g in got]).view(np.uint32) if with_lm else score
    _same((hyps, score, am), want, "Decoder.ctc_stream on unspliced chunks")
    stream.close()
    # one chunk per lane of spliced rows: the forward sees the rows Decoder.ctc_beam_search sees
    rows = [splice(x, c) for x in xs]
    stream = dec.ctc_stream(lanes=2, beam_width=W, max_frames=64, lm=lm)
    stream.push(rows)
    if with_lm:
        one = dec.ctc_beam_search_lm(rows, lm, beam_width=W, top_paths=P)
        fin = [stream.finish(l, top_paths=P) for l in range(2)]
        _same(([f[0] for f in fin], np.stack([f[1] for f in fin]).view(np.uint32), np.stack([f[2] for f in fin]).view(np.uint32)),
              (one[0], one[1].view(np.uint32), one[2].view(np.uint32)), "single chunk, with the model")
    else:
        one = dec.ctc_beam_search(rows, beam_width=W, top_paths=P)
        part = stream.partial(top_paths=P)
        _same((part[0], part[1].view(np.uint32), part[1].view(np.uint32)), (one[0], one[1].view(np.uint32), None), "single chunk")
    print("F Decoder.ctc_stream%s: unspliced chunks of 7 / 5 frames equal the one-shot search on the logits of those chunks; "
          "one chunk equals Decoder.ctc_beam_search%s bit for bit" % ((" with an n-gram", "_lm") if with_lm else ("", "")))
    stream.close()
    eng.close()
