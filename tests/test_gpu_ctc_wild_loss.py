"""The CTC loss with wildcard gaps on the device (tfk_accumulate_ctc_wild and its variants, tfk_ctc_wild_loss_logits;
ctc_gather_kernel and ctc_grad_kernel<true> in csrc/ctc.hip) against the float64 restatement of
tests/test_ctc_wild_loss_host.py applied to the SAME logits.

Bounds: the project's own for these kernels (tests/test_gpu_ctc.py, tests/test_gpu_ctc_edges.py).
  loss per utterance   |got - want| <= 2e-5 max(|want|, L_plain) + 1e-6 max(Tn, 1), L_plain = the float64 plain CTC loss of the
                       same labels without flags (finite exactly when want is): the wildcard loss can sit near 0, where a
                       relative bound means nothing, while the sweep is the plain loss's and its error scales with that loss
  dLogits              rtol 1e-4 + atol 2e-5 below 200 frames per batch, atol 2e-4 from there on (those files' own figures)
  row sums of dLogits  within 2e-5 of 0
Every comparison prints one "ctc_wild_loss_edges:" line, the device's error beside its bound; profiles/ctc_wild_loss_edges.txt
is the table of those lines."""
from ctypes import c_float, c_void_p

import numpy as np
import pytest

from oracle.ctc_oracle import ctc_loss_and_grad_vec
from test_ctc_wild_loss_host import wild_bounds, wild_loss_grad64
from test_gpu_ctc_edges import PEAKY, _frames, _labels, _make, _min_frames
from test_gpu_ctc_wild import _dev, _flags, _p
from util import assert_close, engine_grads, engine_params, make_pair

pytestmark = pytest.mark.gpu

PAD = 3          # ld = O + 3, NaN in the padding columns
UNTOUCHED = 777.0


def _device_loss(z, utt, seqs, flags, penalty, lead=3, tail=5, grad=True, inplace=False, ldd=None):
    """tfk_ctc_wild_loss_logits on host logits [sum(utt), O], laid out with ld = O + PAD (NaN in the padding columns) and junk
    rows around the utterances: (utt_loss [U], dLogits [sum(utt), O] or None, the raw bytes of both).  Checked on the way: the
    element after utt_loss[U] and every row outside [seg[0], seg[U]) keep their sentinel, columns [O, ldd) are zero."""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    T, O, U = z.shape[0], z.shape[1], len(utt)
    ld = O + PAD
    ldd = ld if (ldd is None or inplace) else ldd
    full = np.full((lead + T + tail, ld), 50.0, np.float32)  # (what surrounds the utterances must not matter)
    full[:, O:] = np.nan
    full[lead:lead + T, :O] = z
    seg = (lead + np.concatenate([[0], np.cumsum(utt)])).astype(np.int32)
    lab_off = np.concatenate([[0], np.cumsum([len(r) for r in seqs])]).astype(np.int32)
    labels = np.concatenate([np.asarray(r, np.int32) for r in seqs] + [np.zeros(1, np.int32)])
    d_z, d_seg, d_lab, d_off = _dev(full), _dev(seg), _dev(labels), _dev(lab_off)
    d_wild = None if flags is None else _dev(np.concatenate([np.asarray(f).astype(np.uint8) for f in flags] + [np.zeros(1, np.uint8)]))
    loss = torch.full((U + 1,), 12345.0, dtype=torch.float32, device="cuda")
    dlog = d_z if inplace else torch.full((full.shape[0], ldd), UNTOUCHED, dtype=torch.float32, device="cuda") if grad else None
    _lib.check(lib.tfk_ctc_wild_loss_logits(c_void_p(torch.cuda.current_stream().cuda_stream), _p(d_z), ld, O, full.shape[0],
                                            _p(d_seg), U, _p(d_lab), _p(d_off), _p(d_wild), c_float(penalty), _p(loss), _p(dlog),
                                            ldd))
    torch.cuda.synchronize()
    loss = loss.cpu().numpy()
    assert loss[U] == 12345.0  # nothing is written past the utterances
    if dlog is None:
        return loss[:U], None, loss[:U].tobytes()
    dlog = dlog.cpu().numpy()
    outside = np.concatenate([dlog[:lead], dlog[lead + T:]])
    if inplace:
        assert np.array_equal(outside, np.concatenate([full[:lead], full[lead + T:]]), equal_nan=True)
    else:
        assert np.all(outside == UNTOUCHED)
    assert not dlog[lead:lead + T, O:].any()
    inner = dlog[lead:lead + T, :O].copy()
    return loss[:U], inner, loss[:U].tobytes() + inner.tobytes()


def _reference(z, utt, seqs, flags, penalty):
    """per utterance (loss, gradient, plain CTC loss of the same labels) in float64"""
    zs = np.split(np.asarray(z, np.float64), np.cumsum(utt)[:-1])
    out = []
    for zu, s, f in zip(zs, seqs, flags if flags is not None else [None] * len(seqs)):
        loss, grad = wild_loss_grad64(zu, s, f, penalty)
        out.append((loss, grad, ctc_loss_and_grad_vec(zu, s)[0]))
    return out


def _compare(name, got_loss, got_dlog, ref, utt):
    """the bounds of this file's docstring; one ctc_wild_loss_edges line, printed before anything is asserted"""
    T = int(np.sum(utt))
    want_grad = np.concatenate([r[1] for r in ref]) if T else np.zeros((0, 0))
    worst_loss = worst_ratio = 0.0
    bad = []
    for u, (want, _, plain) in enumerate(ref):
        assert np.isfinite(want) == np.isfinite(plain), (name, u, want, plain)
        if not np.isfinite(want):
            if got_loss[u] != want:
                bad.append((u, got_loss[u], want))
            continue
        bound = wild_bounds(want, plain, utt[u], T)[0]
        err = abs(float(got_loss[u]) - want)
        worst_loss, worst_ratio = max(worst_loss, err), max(worst_ratio, err / bound)
        if err > bound:
            bad.append((u, got_loss[u], want, bound))
    _, rtol, atol = wild_bounds(0.0, 0.0, 0, T)
    derr = float(np.abs(got_dlog - want_grad).max()) if T else 0.0
    rows = float(np.abs(got_dlog.astype(np.float64).sum(axis=1)).max()) if T else 0.0
    finite = [r[0] for r in ref if np.isfinite(r[0])]
    print("ctc_wild_loss_edges: %-34s U %2d T %4d | loss %10.4f .. %10.4f, inf %d | device: loss err %.1e (%.2f of its bound) | "
          "dlogits err %.1e bound %.0e + %.0e |want| | row sums %.1e bound 2e-05"
          % (name, len(utt), T, min(finite, default=np.nan), max(finite, default=np.nan), len(ref) - len(finite), worst_loss,
             worst_ratio, derr, atol, rtol, rows))
    assert not bad, (name, bad)
    if T:
        assert_close(name + ": dlogits", got_dlog, want_grad, rtol=rtol, atol=atol)
        assert rows <= 2e-5, (name, rows)
    r0 = 0
    for u, (want, _, _) in enumerate(ref):  # an infinite loss: zero rows
        if not np.isfinite(want):
            assert not got_dlog[r0:r0 + utt[u]].any(), (name, u)
        r0 += utt[u]


def _case(name, z, utt, seqs, flags, penalty):
    got_loss, got_dlog, _ = _device_loss(z, utt, seqs, flags, penalty)
    ref = _reference(z, utt, seqs, flags, penalty)
    _compare("%s S<=%d" % (name, max(len(s) for s in seqs)), got_loss, got_dlog, ref, utt)
    return got_loss, got_dlog, ref


def _logits(rng, T, O, scale=2.0):
    return (scale * rng.standard_normal((T, O))).astype(np.float32)


# ---- through tfk_ctc_wild_loss_logits ----

@pytest.mark.parametrize("penalty", [0.0, 0.7])
@pytest.mark.parametrize("mode", ["ends", "all", "random"])
def test_frame_counts_around_the_prefetch_ring(gpu, mode, penalty):
    """every Tn in 0 .. 10 and 15, 16, 17 (the edges of the 8-frame prefetch ring), random labels with S <= Tn / 2, in ONE batch
    of mixed S -- so the `+ u` of the flag offset matters -- with S = 0 both flagged and unflagged"""
    O = 9
    rng = np.random.default_rng(9000)
    utt, seqs = [], []
    for Tn in list(range(11)) + [15, 16, 17]:
        utt.append(Tn)
        seqs.append(_labels(rng, int(rng.integers(0, Tn // 2 + 1)), O, repeat=0.3))
    utt += [5, 5, 0, 0]
    seqs += [np.zeros(0, np.int32)] * 4
    flags = _flags(rng, mode, seqs)
    flags[-4][0], flags[-3][0], flags[-2][0], flags[-1][0] = 1, 0, 1, 0
    assert len({len(s) for s in seqs}) >= 5
    got, _, ref = _case("frames %s pen %.1f" % (mode, penalty), _logits(rng, sum(utt), O), utt, seqs, flags, penalty)
    assert all(np.isfinite(r[0]) for r in ref)
    assert got[-2] == 0.0 and got[-1] == 0.0 and got[0] == 0.0  # no frames, no labels
    assert abs(ref[-4][0] - 5 * penalty) <= 1e-12 and got[-3] > 0.0  # S = 0: all wild costs the penalty alone, plain the blanks


@pytest.mark.parametrize("S", [1, 63, 64, 127, 128, 255, 256, 511])
def test_every_register_tile(gpu, S):
    """R = 2 / 4 / 8 / 16, the last states in lane 63 or straddling two lanes; Tn = the shortest alignment + 3; random flags;
    a second, short utterance keeps the wave of the first from being alone"""
    O = 36
    rng = np.random.default_rng(9100 + S)
    seqs = [_labels(rng, S, O, repeat=0.25), _labels(rng, 3, O)]
    utt = [_min_frames(seqs[0]) + 3, 11]
    flags = _flags(rng, "random", seqs)
    _, _, ref = _case("tile S=%d random pen 0.3" % S, _logits(rng, sum(utt), O), utt, seqs, flags, 0.3)
    assert all(np.isfinite(r[0]) for r in ref)


def test_repeats_at_and_below_the_minimum_frame_count(gpu):
    """equal neighbours with the gap between them flagged and unflagged, at the exact minimum frame count and one below it:
    a wildcard gap between two equal labels still needs its frame, so one below gives +inf and zero rows either way"""
    O = 9
    rng = np.random.default_rng(9200)
    lab = np.array([2, 2, 5, 5, 5, 1], np.int32)
    need = _min_frames(lab)
    assert need == 9
    between = np.array([0, 1, 0, 1, 1, 0, 0], np.uint8)  # the gaps between equal neighbours
    utt, seqs, flags = [], [], []
    for Tn in (need, need - 1):
        for f in (between, np.zeros(7, np.uint8), np.ones(7, np.uint8)):
            utt.append(Tn)
            seqs.append(lab)
            flags.append(f)
    for pen in (0.0, 0.7):
        got, _, ref = _case("repeats pen %.1f" % pen, _logits(rng, sum(utt), O), utt, seqs, flags, pen)
        assert [np.isfinite(r[0]) for r in ref] == [True] * 3 + [False] * 3
        assert np.all(got[3:] == np.inf)


def test_known_answers(gpu):
    O = 4
    rng = np.random.default_rng(9300)
    pen, Tw = 0.7, 10
    peaked = np.full((Tw, O), -40.0, np.float32)
    peaked[:, 0] = 40.0
    z = np.concatenate([_logits(rng, 7 + 2 + 3, O), peaked])
    utt = [7, 2, 3, Tw]
    seqs = [np.zeros(0, np.int32), np.array([1, 1], np.int32), np.array([1, 1], np.int32), np.array([0], np.int32)]
    flags = [np.array([1], np.uint8), np.array([0, 1, 0], np.uint8), np.array([0, 1, 0], np.uint8), np.array([1, 1], np.uint8)]
    got, dlog, ref = _case("known answers pen 0.7", z, utt, seqs, flags, pen)
    lp = z.astype(np.float64) - np.log(np.exp(z.astype(np.float64)).sum(axis=1, keepdims=True))
    # (the device is held to the restatement by _case; here the restatement is held to the closed forms)
    assert abs(ref[0][0] - 7 * pen) <= 1e-12 and np.abs(dlog[:7]).max() <= 1e-6  # (x * (1 / x) need not be exactly 1)
    assert ref[1][0] == np.inf and got[1] == np.inf and not dlog[7:9].any()
    assert abs(ref[2][0] - (-(lp[9, 1] + lp[11, 1]) + pen)) <= 1e-12
    got, dlog, ref = _case("known answers pen 0.0", z, utt, seqs, flags, 0.0)
    assert ref[0][0] == 0.0 and np.abs(dlog[:7]).max() <= 1e-6
    assert abs(ref[3][0] + np.log(Tw * (Tw + 1) / 2)) <= 1e-12 and got[3] < 0  # the negative loss: 55 paths of value 1


def test_long_and_peaky(gpu):
    """1500 frames through the peaky model of test_gpu_ctc_edges.py (logit scale 12, blank bias 3), S = 5, both ends wild: the
    workload's own shape, few labels in a long recording; the offsets carry thousands"""
    O, T = 36, 1500
    rng = np.random.default_rng(9400)
    eng = _make(O, PEAKY)[0]
    z = eng.posteriors(_frames(rng, T), raw_logits=True)
    eng.close()
    seqs = [_labels(rng, 5, O, distinct=True)]
    _, _, ref = _case("long peaky ends pen 0.0", z, [T], seqs, _flags(rng, "ends", seqs), 0.0)
    assert np.isfinite(ref[0][0]) and ref[0][2] > 1000.0


def test_bits(gpu):
    """two calls give the same bits; in place equals out of place; a narrower dLogits (ldd = O) holds the same values; the
    loss-only call (dlogits NULL) gives the same losses; NULL flags are all-zero flags"""
    O = 9
    rng = np.random.default_rng(9500)
    utt = [40, 0, 17, 9]
    seqs = [_labels(rng, n, O, repeat=0.3) for n in (12, 0, 5, 4)]
    flags = _flags(rng, "random", seqs)
    z = _logits(rng, sum(utt), O)
    first = _device_loss(z, utt, seqs, flags, 0.5)
    assert _device_loss(z, utt, seqs, flags, 0.5)[2] == first[2]
    assert _device_loss(z, utt, seqs, flags, 0.5, inplace=True)[2] == first[2]
    assert _device_loss(z, utt, seqs, flags, 0.5, ldd=O)[2] == first[2]
    assert _device_loss(z, utt, seqs, flags, 0.5, grad=False)[2] == first[0].tobytes()
    assert _device_loss(z, utt, seqs, None, 0.5)[2] == _device_loss(z, utt, seqs, _flags(rng, "none", seqs), 0.0)[2]
    print("ctc_wild_loss_edges: bits: two calls, in place, ldd = O, loss only and NULL flags agree byte for byte")


# ---- through the engine ----

def _engine_case(dtype, seed=9600):
    """the 4 x 64 net of tests/test_gpu_ctc_mmi.py (tanh, batch norm; "bfloat16": its relu chain without batch norm, for the
    reason stated there), three utterances, random gap flags"""
    from test_gpu_ctc_mmi import KW4
    rng = np.random.default_rng(seed)
    kw = dict(KW4, nonlin="relu", batch_norm=False) if dtype == "bfloat16" else KW4
    eng, oracle = make_pair(rng, max_frames=512, compute_dtype=dtype, **kw)
    utt = [60, 35, 48]
    refs = [_labels(rng, n, KW4["output_dim"], repeat=0.2) for n in (7, 1, 9)]
    X = (rng.standard_normal((sum(utt), KW4["input_dim"])) * 1.5).astype(np.float32)
    flags = [np.array([1, 0, 0, 1, 0, 0, 0, 1], np.uint8), np.array([1, 1], np.uint8), rng.integers(0, 2, size=10).astype(np.uint8)]
    labels, lab = np.concatenate(refs).astype(np.int32), np.array([r.size for r in refs], np.int32)
    return eng, oracle, utt, X, refs, flags, labels, lab


def _sums(eng, T):
    from tfkaldi_amd import _lib
    return eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES), eng.debug_fetch(_lib.DBG_LOGITS, 0, T).tobytes()


def test_no_flags_is_accumulate_ctc_bit_for_bit(gpu):
    """wild=None and wild = zeros at penalty 0.5 against accumulate_ctc: BATCH_LOSS, NUM_FRAMES and the bytes of DBG_LOGITS
    (dLogits after a training pass, the logits after an evaluation pass), train and eval"""
    eng, _, utt, X, _, flags, labels, lab = _engine_case("float32")
    zeros = np.zeros(int(lab.sum()) + lab.size, np.uint8)
    T = sum(utt)
    for train in (True, False):
        out = []
        for how in ("plain", "none", "zeros", "flags"):
            eng.eval_finish()
            if how == "plain":
                (eng.accumulate_ctc if train else eng.eval_accumulate_ctc)(X, utt, labels, lab)
            else:
                wild = {"none": None, "zeros": zeros, "flags": np.concatenate(flags)}[how]
                eng.accumulate_ctc_wild(X, utt, labels, lab, wild=wild, penalty=0.5, train=train)
            out.append(_sums(eng, T))
        assert out[0] == out[1] == out[2] and np.isfinite(out[0][0]) and out[0][1] == lab.sum()
        assert out[3][0] != out[0][0] and out[3][1] == lab.sum()  # (and real flags are another criterion)
    eng.eval_finish()
    eng.close()


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_training_call(gpu, dtype):
    """tests/test_gpu_ctc_mmi.py::test_training_call with this criterion: batch_loss, num_frames, dLogits and the parameter
    gradients against the restatement on the oracle's train-mode logits, run through the oracle's backward pass; fp32 and bf16
    at that test's own tolerances"""
    from tfkaldi_amd import _lib
    eng, oracle, utt, X, refs, flags, labels, lab = _engine_case(dtype)
    pen, T = 0.3, sum(utt)
    eng.accumulate_ctc_wild(X, utt, labels, lab, wild=np.concatenate(flags), penalty=pen)
    ref = _reference(oracle.forward_logits(X), utt, refs, flags, pen)
    loss, dlog = sum(r[0] for r in ref), np.concatenate([r[1] for r in ref])
    oracle.backward_from_dlogits(dlog, loss, int(lab.sum()))
    got_loss, got_n = eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES)
    got_dlog, got = eng.debug_fetch(_lib.DBG_LOGITS, 0, T), engine_grads(eng)
    keys = [k for k in oracle.G if not (oracle.bn and k.startswith("b") and not k.startswith("beta") and k != "b%d" % oracle.L)]
    fro = lambda g, w: float(np.linalg.norm(np.asarray(g, np.float64) - w) / max(np.linalg.norm(w), 1e-30))
    print("ctc_wild_loss_edges: training %-9s loss %.4f err %.1e (rel) | dlogits max %.1e fro %.1e | gradients fro %s"
          % (dtype, loss, abs(got_loss - loss) / abs(loss), np.abs(got_dlog - dlog).max(), fro(got_dlog, dlog),
             " ".join("%s %.1e" % (k, fro(got[k], oracle.G[k])) for k in keys)))
    assert got_n == lab.sum() and np.abs(dlog).max() > 1e-2 and loss > 0
    if dtype == "bfloat16":
        np.testing.assert_allclose(got_loss, loss, rtol=5e-4)
        assert fro(got_dlog, dlog) <= 2e-3
        for k in keys:
            assert fro(got[k], oracle.G[k]) <= 2e-3, (k, fro(got[k], oracle.G[k]))
    else:
        assert_close("batch_loss", got_loss, loss, 2e-5, 0)
        assert_close("dlogits", got_dlog, dlog, rtol=1e-4, atol=4e-5)
        for k in keys:
            w = oracle.G[k]
            assert_close("G[%s]" % k, got[k], w, rtol=2e-4, atol=2e-5 * max(np.abs(w).max(), 1e-3))
    avg = eng.apply()
    np.testing.assert_allclose(avg, got_loss / got_n, rtol=1e-6)
    eng.close()


def test_raw_entries_equal_the_plain_ones_bit_for_bit(gpu):
    from test_gpu_ctc_mmi import KW4
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(9700)
    D, C = 4, 2
    eng, _ = make_pair(rng, max_frames=256, **dict(KW4, input_dim=D * (2 * C + 1)))
    _, _, _, _, _, flags, labels, lab = _engine_case("float32")
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 25, 63)]
    lens = [u.shape[0] for u in utts]
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)
    spliced = np.concatenate([u.spliced() for u in utts])
    wild = np.concatenate(flags)
    out = []
    for train in (True, False):
        for how in ("plain", "raw"):
            eng.eval_finish()
            if how == "plain":
                eng.accumulate_ctc_wild(spliced, lens, labels, lab, wild=wild, penalty=0.4, train=train)
            else:
                eng.accumulate_ctc_wild_raw(raw, lens, C, labels, lab, wild=wild, penalty=0.4, cmvn=cmvn_table(utts), train=train)
            out.append(_sums(eng, sum(lens)))
        assert out[-1] == out[-2] and np.isfinite(out[-1][0]) and out[-1][1] == lab.sum()
    assert out[0][2] != out[2][2]  # (training left dLogits, evaluation the logits)
    eng.eval_finish()
    eng.close()


def test_eval_variant_inside_an_open_step(gpu):
    """the loss on evaluation-mode logits; the engine's state untouched; inside a step the step finishes as if nothing had
    been evaluated"""
    from test_gpu_ctc_beam_topk import _engine_state
    eng, _, utt, X, refs, flags, labels, lab = _engine_case("float32", 9800)
    twin = _engine_case("float32", 9800)[0]
    wild, pen = np.concatenate(flags), 0.3
    state0 = _engine_state(eng)
    eng.eval_accumulate_ctc_wild(X, utt, labels, lab, wild, pen)
    ref = _reference(eng.posteriors(X, raw_logits=True), utt, refs, flags, pen)
    loss, plain = sum(r[0] for r in ref), sum(r[2] for r in ref)
    got = eng.eval_finish() * lab.sum()
    print("ctc_wild_loss_edges: eval entry: loss %.6f, restated %.6f (plain %.3f), err %.1e bound %.1e"
          % (got, loss, plain, abs(got - loss), 2e-5 * max(abs(loss), plain)))
    assert abs(got - loss) <= 2e-5 * max(abs(loss), plain)
    state1 = _engine_state(eng)
    assert sorted(state0) == sorted(state1) and all(state0[k] == state1[k] for k in state0)
    for e in (eng, twin):
        e.accumulate_ctc_wild(X, utt, labels, lab, wild, pen)
        if e is eng:
            e.eval_accumulate_ctc_wild(X[:utt[0]], utt[:1], refs[0], lab[:1], flags[0], 1.0)
            assert np.isfinite(e.eval_finish())
        e.accumulate_ctc_wild(X, utt, labels, lab, wild, 0.0, last=True)
    assert eng.apply() == twin.apply()
    pa, pb = engine_params(eng), engine_params(twin)
    assert all(pa[k].tobytes() == pb[k].tobytes() for k in pa)
    eng.close()
    twin.close()


def test_refusals_leave_the_engine_usable(gpu):
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    eng, _, utt, X, _, flags, labels, lab = _engine_case("float32", 9900)
    wild, T = np.concatenate(flags), sum(utt)
    eng.accumulate_ctc_wild(X, utt, labels, lab, wild, 0.3)
    before = engine_grads(eng), eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES)
    ptr = lambda a: a.ctypes.data_as(c_void_p)
    ul = np.asarray(utt, np.int32)

    def call(fn, w, pen):
        _lib.check(fn(eng._h, ptr(X), X.shape[1], T, ptr(ul), len(utt), ptr(labels), ptr(lab), ptr(w), c_float(pen), 0))
    two = wild.copy()
    two[int(lab[0]) + 1 + 1] = 2  # utterance 1's flags start at lab_off[1] + 1: its gap 1
    for fn in (eng.lib.tfk_accumulate_ctc_wild, eng.lib.tfk_eval_accumulate_ctc_wild):
        with pytest.raises(EngineError, match=r"utterance 1, gap 1.*2"):
            call(fn, two, 0.3)
        with pytest.raises(EngineError, match="penalty"):
            call(fn, wild, -1.0)
        with pytest.raises(EngineError, match="penalty"):
            call(fn, wild, float("nan"))
        with pytest.raises(EngineError, match=r"label .* outside"):  # what tfk_accumulate_ctc refuses is refused here
            bad = labels.copy()
            bad[0] = eng.O - 1
            _lib.check(fn(eng._h, ptr(X), X.shape[1], T, ptr(ul), len(utt), ptr(bad), ptr(lab), ptr(wild), c_float(0.3), 0))
        after = engine_grads(eng), eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES)
        assert after[1:] == before[1:] and all((after[0][k] == before[0][k]).all() for k in before[0])
    with pytest.raises(EngineError, match="gap"):  # the Python entry passes a uint8 flag through; the engine refuses it
        eng.accumulate_ctc_wild(X, utt, labels, lab, two, 0.3)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="penalty"):
            eng.accumulate_ctc_wild(X, utt, labels, lab, wild, bad)
    with pytest.raises(ValueError, match="gap flags"):
        eng.accumulate_ctc_wild(X, utt, labels, lab, wild[:-1], 0.3)
    eng.accumulate_ctc_wild(X, utt, labels, lab, wild, 0.3, last=True)  # the engine still works: the step goes on
    assert eng.scalar(_lib.NUM_FRAMES) == 2 * lab.sum()
    np.testing.assert_allclose(eng.scalar(_lib.BATCH_LOSS), 2 * before[1], rtol=1e-6)
    assert np.isfinite(eng.apply())
    eng.close()


def test_update_wild_descends(gpu, tmp_path):
    """_toy_ctc with the first and last label of every transcript dropped: 20 plain steps on the full transcripts, then 30
    update_wild(wild="ends") steps on the truncated ones lower evaluate_wild.  Printed, not asserted: the greedy label errors
    against the FULL transcripts beside those of a twin trainer given 30 plain update steps on the truncated transcripts."""
    from test_gpu_ctc_decode import _toy_ctc
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer

    def run(kind):
        where = tmp_path / kind
        where.mkdir()
        dnn, disp, coder, F, maxlen = _toy_ctc(where)
        tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
        tr.initialize()
        xs, ys = disp.get_batch()
        cut = [np.asarray(y)[1:-1] for y in ys]
        assert all(len(c) >= 1 for c in cut)
        for _ in range(20):
            tr.update(xs, ys)
        before, err0 = tr.evaluate_wild(xs, cut, wild="ends"), tr.label_errors(xs, ys)
        step = (lambda: tr.update_wild(xs, cut, wild="ends")) if kind == "wild" else (lambda: tr.update(xs, cut))
        losses = [step() for _ in range(30)]
        after, err1 = tr.evaluate_wild(xs, cut, wild="ends"), tr.label_errors(xs, ys)
        with pytest.raises(ValueError, match="wild"):
            tr.update_wild(xs, cut, wild="middle")
        tr.close()
        return before, after, err0, err1, losses
    wild, plain = run("wild"), run("plain")
    print("ctc_wild_loss_edges: descent: evaluate_wild %.5f -> %.5f over 30 update_wild steps (first / last step %.5f / %.5f); "
          "greedy label errors against the FULL transcripts %s -> %s; twin with 30 plain update steps on the truncated "
          "transcripts: evaluate_wild %.5f -> %.5f, label errors %s -> %s"
          % (wild[0], wild[1], wild[4][0], wild[4][-1], wild[2], wild[3], plain[0], plain[1], plain[2], plain[3]))
    assert all(np.isfinite(wild[4])) and np.isfinite(wild[0]) and wild[1] < wild[0]
