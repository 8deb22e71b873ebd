"""The CTC loss with wildcard gaps, CPU tier: the float64 restatement the GPU tests check the device against (the contract
stated in include/tfkaldi_hip.h at tfk_accumulate_ctc_wild: the lattice and transitions of the plain loss, a flagged gap
state emitting exp(-penalty) whatever the frame holds, loss = -log of the lattice's value, gradient = softmax * (1 - W_t) -
the other states' posteriors folded onto their classes), pinned four ways -- by enumeration of all state paths, by central
finite differences, by the identity with oracle/ctc_oracle.py at zero flags and by known answers; a float32 run of the same
restatement beside the bounds the GPU tests use; and CTCTrainer.update_wild / evaluate_wild over a numpy stand-in engine."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ctc_oracle import ctc_loss_and_grad_vec  # noqa: E402
from test_ctc_align_wild_host import enumerate_paths, gap_flags  # noqa: E402


def _sweep(e, skip):
    """forward variables of the lattice over the log emissions e [T, n] in e's dtype: per frame the vector relative to its
    own maximum, and the running sum of those maxima in float64 (the device keeps its offsets in double too).  skip[s]: the
    step s - 2 -> s is allowed.  Returns (values [T, n], offsets [T])."""
    T, n = e.shape
    dt = e.dtype.type
    ninf = dt(-np.inf)
    vals, offs = np.full((T, n), ninf, dtype=e.dtype), np.zeros(T)
    a = np.full(n, ninf, dtype=e.dtype)
    a[:2] = e[0, :2]
    off = 0.0
    for t in range(T):
        if t:
            p1 = np.concatenate([[ninf], a[:-1]]).astype(e.dtype)
            p2 = np.where(skip, np.concatenate([[ninf, ninf], a[:-2]])[:n], ninf).astype(e.dtype)
            m = np.maximum(a, np.maximum(p1, p2))
            ok = np.isfinite(m)
            ms = np.where(ok, m, dt(0))
            with np.errstate(divide="ignore", invalid="ignore"):
                a = np.where(ok, ms + np.log(np.exp(a - ms) + np.exp(p1 - ms) + np.exp(p2 - ms)) + e[t], ninf).astype(e.dtype)
        m = a.max()
        if np.isfinite(m):
            off += float(m)
            a = (a - m).astype(e.dtype)
        vals[t], offs[t] = a, off
    return vals, offs


def wild_loss_grad64(z, labels, flags=None, penalty=0.0, dtype=np.float64):
    """(loss, dL/dz [T, O] in float64) of ONE utterance with logits z [T, O], blank = the LAST class; flags: None, "ends",
    "all" or the S + 1 gap flags.  dtype=np.float32 runs every per-state value in float32 (offsets, log Z and the exponent's
    shift stay in float64): the device's arithmetic, for the error model."""
    z = np.asarray(z, dtype=dtype)
    T, O = z.shape
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    S, n = labels.size, 2 * labels.size + 1
    if T == 0:
        return (0.0 if S == 0 else np.inf), np.zeros((0, O))
    ext = np.full(n, O - 1, dtype=np.int64)
    ext[1::2] = labels
    w = np.zeros(n, dtype=bool)
    w[0::2] = gap_flags(labels, flags)
    skip = np.zeros(n, dtype=bool)
    skip[3::2] = labels[1:] != labels[:-1]
    m = z.max(axis=1, keepdims=True)
    lp = (z - m - np.log(np.exp(z - m).sum(axis=1, keepdims=True, dtype=dtype))).astype(dtype)
    e = lp[:, ext]
    e[:, w] = dtype(-penalty)
    al, offa = _sweep(e, skip)
    # the backward variables are the forward variables of the mirrored problem (n is odd: label states stay label states)
    rskip = np.zeros(n, dtype=bool)
    rskip[3::2] = labels[::-1][1:] != labels[::-1][:-1]
    be, offb = _sweep(np.ascontiguousarray(e[::-1, ::-1]), rskip)
    be, offb = be[::-1, ::-1], offb[::-1]
    # (in log space: with wildcards the end states can lie thousands below the frame's largest state)
    logz = offa[T - 1] + np.logaddexp.reduce(al[T - 1, max(n - 2, 0):].astype(np.float64))
    if not np.isfinite(logz):
        return np.inf, np.zeros((T, O))
    with np.errstate(invalid="ignore"):
        v = (al + be - e).astype(dtype)
    ok = np.isfinite(v)
    g = np.exp(np.where(ok, np.where(ok, v, 0).astype(np.float64) + (offa + offb - logz)[:, None], -np.inf))  # posteriors [T, n]
    if dtype is not np.float64:  # the device divides a frame's posteriors by their sum -- over ALL states -- where it is near one
        tot = g.sum(axis=1, keepdims=True)
        g = np.where(np.abs(tot - 1.0) < 1e-2, g / tot, g)
    grad = np.exp(lp.astype(np.float64)) * (1.0 - g[:, w].sum(axis=1))[:, None]
    keep = np.flatnonzero(~w)
    np.subtract.at(grad, (np.arange(T)[:, None], ext[None, keep]), g[:, keep])
    return float(-logz), grad


def brute_loss(z, labels, flags, penalty):
    """-log of the sum over every valid state path of the product of its emissions, path by path"""
    z = np.asarray(z, dtype=np.float64)
    T, O = z.shape
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    n = 2 * labels.size + 1
    ext = np.full(n, O - 1, dtype=np.int64)
    ext[1::2] = labels
    w = np.zeros(n, dtype=bool)
    w[0::2] = gap_flags(labels, flags)
    skip = np.zeros(n, dtype=bool)
    skip[3::2] = labels[1:] != labels[:-1]
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    total = sum(np.exp(sum(-penalty if w[s] else lp[t, ext[s]] for t, s in enumerate(p))) for p in enumerate_paths(T, n, skip))
    return -np.log(total) if total > 0 else np.inf


def _small_cases(seed, count):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        T, O, S = int(rng.integers(1, 6)), int(rng.integers(2, 5)), int(rng.integers(0, 4))
        z = 2.0 * rng.standard_normal((T, O))
        lab = rng.integers(0, O - 1, size=S)
        yield z, lab, rng.integers(0, 2, size=S + 1).astype(bool), float(rng.choice([0.0, 0.7]))


def test_restatement_equals_enumeration_of_all_state_paths():
    """T <= 5, O <= 4, S <= 3 (repeats occur: O - 1 labels to draw from), random flags, penalty 0 and 0.7, 200 cases"""
    feasible = 0
    for z, lab, flags, pen in _small_cases(800, 200):
        loss, grad = wild_loss_grad64(z, lab, flags, pen)
        want = brute_loss(z, lab, flags, pen)
        if np.isinf(want):
            assert loss == np.inf and not grad.any()
            continue
        feasible += 1
        assert abs(loss - want) <= 1e-10, (lab, flags, pen, loss, want)
        assert np.abs(grad.sum(axis=1)).max() <= 1e-12  # every row sums to zero
    assert feasible >= 100


def test_gradient_equals_central_finite_differences():
    done = 0
    for z, lab, flags, pen in _small_cases(801, 60):
        loss, grad = wild_loss_grad64(z, lab, flags, pen)
        if np.isinf(loss):
            continue
        num = np.zeros_like(z)
        for i in range(z.shape[0]):
            for j in range(z.shape[1]):
                zp, zm = z.copy(), z.copy()
                zp[i, j] += 1e-6
                zm[i, j] -= 1e-6
                num[i, j] = (wild_loss_grad64(zp, lab, flags, pen)[0] - wild_loss_grad64(zm, lab, flags, pen)[0]) / 2e-6
        assert np.abs(num - grad).max() <= 1e-6, (lab, flags, pen)
        done += 1
    assert done >= 30


def test_zero_flags_is_the_ctc_oracle_at_any_penalty():
    rng = np.random.default_rng(802)
    for T, O, S in ((40, 9, 7), (1, 3, 1), (12, 4, 6), (200, 36, 63), (5, 6, 0)):
        z = 2.0 * rng.standard_normal((T, O))
        lab = rng.integers(0, O - 1, size=S)
        want_loss, want_grad = ctc_loss_and_grad_vec(z, lab)
        for flags, pen in ((None, 0.0), (np.zeros(S + 1, bool), 0.5)):
            loss, grad = wild_loss_grad64(z, lab, flags, pen)
            assert abs(loss - want_loss) <= 1e-11 * max(1.0, abs(want_loss)) and np.abs(grad - want_grad).max() <= 1e-11
    # too short for its labels: +inf and a zero gradient, wildcards or not (the transitions are the plain loss's)
    assert wild_loss_grad64(z[:3], [0, 0, 1], "all")[0] == np.inf == ctc_loss_and_grad_vec(z[:3], [0, 0, 1])[0]
    assert wild_loss_grad64(np.zeros((0, 4)), [], [1])[0] == 0.0 and wild_loss_grad64(np.zeros((0, 4)), [2], "all")[0] == np.inf


def test_known_answers():
    rng = np.random.default_rng(803)
    O = 4
    z = 2.0 * rng.standard_normal((7, O))
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    # S = 0 with its one gap flagged: one path, every frame costs the penalty; nothing depends on the logits
    for pen in (0.0, 0.7):
        loss, grad = wild_loss_grad64(z, [], [1], pen)
        assert abs(loss - 7 * pen) <= 1e-12 and np.abs(grad).max() <= 1e-12
    # [a, a] with only the middle gap flagged: the gap still takes a frame
    assert wild_loss_grad64(z[:2], [1, 1], [0, 1, 0], 0.3)[0] == np.inf
    loss, grad = wild_loss_grad64(z[:3], [1, 1], [0, 1, 0], 0.3)  # exactly one path: a, the gap, a
    assert abs(loss - (-(lp[0, 1] + lp[2, 1]) + 0.3)) <= 1e-12
    want = np.exp(lp[:3])
    want[1] = 0.0  # the middle frame sits in the wildcard with posterior 1: it pulls on no class
    want[0, 1] -= 1.0
    want[2, 1] -= 1.0
    assert np.abs(grad - want).max() <= 1e-12
    # [wild, a, wild] on T frames that put all mass on a: T (T + 1) / 2 paths of value 1 -- the loss is NEGATIVE, because a
    # frame labelling that several lattice paths reach is counted once per path
    for T in (1, 4, 10):
        peaked = np.full((T, 3), -40.0)
        peaked[:, 0] = 40.0
        loss, grad = wild_loss_grad64(peaked, [0], "ends")
        assert abs(loss + np.log(T * (T + 1) / 2)) <= 1e-12 and np.abs(grad).max() <= 1e-12
        assert loss < 0 or T == 1


def wild_bounds(want_loss, plain_loss, Tn, T_batch):
    """the GPU tests' bounds (the project's own for these kernels, tests/test_gpu_ctc.py and tests/test_gpu_ctc_edges.py):
    (loss bound, dLogits rtol, dLogits atol).  The loss bound scales with the plain loss of the same labels, because the
    sweep is the plain loss's and the wildcard loss itself can sit near 0."""
    scale = max(abs(want_loss), plain_loss) if np.isfinite(want_loss) else 0.0
    return 2e-5 * scale + 1e-6 * max(Tn, 1), 1e-4, (2e-5 if T_batch < 200 else 2e-4)


def test_float32_run_of_the_restatement_beside_the_bounds():
    """every per-state value in float32, offsets in float64: |f32 - f64| printed beside the bounds of the GPU tests, which
    it must fit inside with room to spare (the device adds in another order; a float32 run that already filled the bound
    would leave it none)"""
    rng = np.random.default_rng(804)
    for name, T, O, S, scale, flags, pen in (("short", 17, 9, 4, 2.0, "ends", 0.0), ("random flags", 90, 36, 30, 2.0, "random", 0.7),
                                             ("tile 255", 2 * 255 + 40, 36, 255, 2.0, "random", 0.0),
                                             ("long peaky", 1500, 36, 5, 12.0, "ends", 0.0)):
        z = (scale * rng.standard_normal((T, O))).astype(np.float32)
        if name == "long peaky":
            z[:, -1] += 3.0
        lab = rng.integers(0, O - 1, size=S)
        fl = rng.integers(0, 2, size=S + 1).astype(bool) if flags == "random" else flags
        l64, g64 = wild_loss_grad64(z, lab, fl, pen)
        l32, g32 = wild_loss_grad64(z, lab, fl, pen, dtype=np.float32)
        plain = ctc_loss_and_grad_vec(z, lab)[0]
        bound, rtol, atol = wild_bounds(l64, plain, T, T)
        dg = np.abs(g32 - g64)
        print("ctc_wild_loss_edges: f32 restatement %-12s T %4d S %3d | loss %.6f (plain %.3f) |f32 - f64| %.1e bound %.1e | "
              "dlogits |f32 - f64| %.1e bound %.1e + %.0e |want| | row sums %.1e"
              % (name, T, S, l64, plain, abs(l32 - l64), bound, dg.max(), atol, rtol, np.abs(g32.sum(axis=1)).max()))
        assert np.isfinite(l64) and np.isfinite(plain)
        assert abs(l32 - l64) <= bound
        assert (dg <= atol + rtol * np.abs(g64)).all()
        assert np.abs(g64.sum(axis=1)).max() <= 1e-10  # (float64 sums over up to 511 states)


# ---- CTCTrainer.update_wild / evaluate_wild over a numpy stand-in engine ----
F, O = 6, 5


class NumpyWildLossEngine(object):
    """stand-in for Engine's wildcard-loss entries: logits = X @ W of a fixed seeded matrix, the loss by the restatement;
    apply / eval_finish return the accumulated loss per reference label, as the engine does"""

    def __init__(self):
        self.W = 3.0 * np.random.default_rng(13).standard_normal((F, O)).astype(np.float32)
        self.calls, self.loss, self.labels = [], 0.0, 0

    def _accumulate(self, kind, X, utt_lens, labels, label_lens, wild, penalty, last, train):
        z = np.asarray(X, dtype=np.float32) @ self.W
        label_lens = np.asarray(label_lens, dtype=np.int64)
        assert z.shape[0] == sum(utt_lens) > 0 and len(labels) == label_lens.sum()
        seqs = np.split(np.asarray(labels), np.cumsum(label_lens)[:-1])
        if wild is None:
            flags = [None] * len(seqs)
        else:  # the layout of tfk_accumulate_ctc_wild: utterance u's flags start at lab_off[u] + u
            assert wild.dtype == np.uint8 and wild.size == label_lens.sum() + label_lens.size and wild.max(initial=0) <= 1
            lab_off = np.concatenate([[0], np.cumsum(label_lens)])
            flags = [wild[lab_off[u] + u:lab_off[u] + u + label_lens[u] + 1] for u in range(label_lens.size)]
        self.calls.append((kind, len(utt_lens), None if wild is None else wild.tolist(), penalty, bool(last), bool(train)))
        for zu, s, f in zip(np.split(z, np.cumsum(utt_lens)[:-1]), seqs, flags):
            self.loss += wild_loss_grad64(zu, s, f, penalty)[0]
        self.labels += int(label_lens.sum())

    def accumulate_ctc_wild(self, X, utt_lens, labels, label_lens, wild=None, penalty=0.0, last=False, train=True):
        self._accumulate("wild", X, utt_lens, labels, label_lens, wild, penalty, last, train)

    def accumulate_ctc_wild_raw(self, raw, utt_lens, context_width, labels, label_lens, wild=None, penalty=0.0, last=False,
                                cmvn=None, train=True):
        assert context_width == 0
        self._accumulate("wild_raw", raw, utt_lens, labels, label_lens, wild, penalty, last, train)

    def _finish(self):
        out = self.loss / self.labels if self.labels else float("nan")
        self.loss, self.labels = 0.0, 0
        return out

    apply = eval_finish = _finish


def _trainer(engine, per_minibatch):
    from tfkaldi_amd.dataparallel import DataParallel
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    tr = CTCTrainer.__new__(CTCTrainer)  # (the constructor creates a device engine)
    tr.engine, tr.dp, tr.numutterances_per_minibatch = engine, DataParallel(), per_minibatch
    tr.loss_kind, tr.summarywriter = "ctc", None
    return tr


def test_trainer_update_wild_over_a_stand_in_engine():
    from tfkaldi_amd.processing.feature_reader import Unspliced
    rng = np.random.default_rng(805)
    lens = [12, 9, 5, 14, 7, 10]
    sizes = [3, 0, 2, 5, 0, 1]  # micro-batches of 2 utterances with different S, S = 0 included
    xs = [rng.standard_normal((n, F)).astype(np.float32) for n in lens]
    ys = [rng.integers(0, O - 1, size=k) for k in sizes]
    eng = NumpyWildLossEngine()
    tr = _trainer(eng, 2)
    forms = {"ends": "ends", "all": "all", "none": None,
             "arrays": [rng.integers(0, 2, size=k + 1).astype(bool) for k in sizes]}
    for name, wild in forms.items():
        for pen in (0.0, 0.5):
            per_utt = [wild[u] if name == "arrays" else wild for u in range(6)]
            want = sum(wild_loss_grad64(x @ eng.W, y, f, pen)[0] for x, y, f in zip(xs, ys, per_utt)) / sum(sizes)
            eng.calls = []
            got = tr.update_wild(xs, ys, wild=wild, penalty=pen)
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (name, pen)
            assert [c[0] for c in eng.calls] == ["wild"] * 3 and [c[4] for c in eng.calls] == [False, False, True]
            assert all(c[3] == pen and c[5] for c in eng.calls)
            for k, c in enumerate(eng.calls):  # the flags are cut per micro-batch
                if wild is None:
                    assert c[2] is None
                else:
                    cut = np.concatenate([gap_flags(ys[u], per_utt[u]) for u in (2 * k, 2 * k + 1)])
                    assert c[2] == cut.astype(np.uint8).tolist(), (name, k)
            eng.calls = []
            assert abs(tr.evaluate_wild(xs, ys, wild=wild, penalty=pen) - want) <= 1e-12 * max(1.0, abs(want))
            assert [c[4:] for c in eng.calls] == [(False, False)] * 3
    assert tr.update_wild(xs, ys) == tr.update_wild(xs, ys, wild="ends", penalty=0.0)  # the defaults
    assert tr.evaluate_wild(None, None) is None
    # all Unspliced: the device-splice entry
    eng.calls = []
    raw = tr.update_wild([Unspliced(x, 0) for x in xs], ys, wild=forms["arrays"], penalty=0.5)
    assert [c[0] for c in eng.calls] == ["wild_raw"] * 3
    assert raw == tr.update_wild(xs, ys, wild=forms["arrays"], penalty=0.5)
    # a bad wild or penalty raises before the step starts
    eng.calls = []
    for bad in (dict(wild="middle"), dict(wild=forms["arrays"][:-1]), dict(wild=[np.zeros(k + 2, bool) for k in sizes]),
                dict(penalty=-1.0), dict(penalty=float("nan")), dict(penalty=float("inf")), dict(penalty="soft")):
        for fn in (tr.update_wild, tr.evaluate_wild):
            with pytest.raises(ValueError):
                fn(xs, ys, **bad)
    with pytest.raises(ValueError):
        tr.update_wild(xs, ys[:-1])
    with pytest.raises(ValueError, match=r"CTCTrainer\.update_wild: the batch holds no frames"):
        tr.update_wild([np.zeros((0, F), np.float32)] * 2, [np.zeros(0, np.int32)] * 2)
    assert eng.calls == [] and eng.labels == 0
