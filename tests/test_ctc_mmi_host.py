"""The MMI criterion against a denominator graph (CTC-CRF; include/tfkaldi_hip.h at tfk_accumulate_ctc_mmi) on the host: a
float64 restatement of the contract (mmi_loss_grad64) and the fp32 error model the GPU tests hold the device to (mmi_tol);
log Z against exhaustive enumeration of the accepted label sequences, the gradient against central differences of the
restatement's own loss, known answers, and the Python plumbing (GraphLM.num_arcs / composed_states, the ValueError of
CTCTrainer.update_mmi for a rejected reference, the dispatch of a CtcMmiMicroBatch) with a stub engine.  No GPU."""
import numpy as np
import pytest

from oracle.ctc_oracle import ctc_loss_and_grad_vec
from test_ctc_beam_host import enumerate_labellings
from tfkaldi_amd.neuralNetworks.ctc_lm import GraphLM, NgramLM

E = np.zeros(0, np.int32)


def graph_arcs(graph):
    """(src, label, dst, weight) of every arc, and the final weights, as float64 arrays"""
    S, O = graph.table.shape
    src, c = np.nonzero(graph.table[:, :O - 1] > -np.inf)
    return src, c, graph.next[src, c].astype(np.int64), graph.table[src, c].astype(np.float64), \
        graph.table[:, O - 1].astype(np.float64)


def graph_score(graph, labels):
    """G(y) in float64, UNSCALED: the arc weights along y plus the final weight of the state it reaches; -inf: rejected"""
    s, total = graph.start, 0.0
    for c in np.asarray(labels, dtype=np.int64).reshape(-1):
        w = float(graph.table[s, c])
        if w == -np.inf:
            return -np.inf
        total += w
        s = int(graph.next[s, c])
    return total + float(graph.table[s, -1])


def _others(M):
    """[S, O] -> for every (g, c) the sum over c' != c of M[g, c'], formed by ADDING a prefix and a suffix"""
    zero = np.zeros((M.shape[0], 1), dtype=M.dtype)
    pre = np.concatenate([zero, np.cumsum(M, axis=1, dtype=M.dtype)[:, :-1]], axis=1)  # (exclusive: shifted, not "- M")
    suf = np.concatenate([np.cumsum(M[:, ::-1], axis=1, dtype=M.dtype)[:, ::-1][:, 1:], zero], axis=1)
    return pre + suf


def den_forward_backward(z, graph, lam, dtype=np.float64, backward=True):
    """The denominator's sweeps of ONE utterance as the contract states them, in the probability domain in `dtype`, every
    frame's vector scaled by the exact power of two that brings its maximum into [1, 2) (what the device does: the scaling
    itself rounds nothing) with the exponents kept in float64.  Returns (log Z, occ_den [T, O] or None)."""
    z = np.asarray(z).astype(dtype)
    T, O = z.shape
    S = graph.num_states
    src, c, dst, w, fin = graph_arcs(graph)
    wa = np.exp(lam * w).astype(dtype)
    with np.errstate(invalid="ignore"):
        f = np.where(fin > -np.inf, np.exp(lam * np.where(fin > -np.inf, fin, 0.0)), 0.0).astype(dtype)
    if T == 0:
        return (lam * fin[graph.start] if f[graph.start] > 0 else -np.inf), np.zeros((0, O))
    mx = z.max(axis=1, keepdims=True)
    ez = np.exp(z - mx).astype(dtype)
    p = (ez / ez.sum(axis=1, keepdims=True, dtype=dtype)).astype(dtype)
    blank = O - 1
    key = dst * O + c  # the (target state, label) group of an arc
    skey = src * O + c

    def grid(v, k):
        return np.bincount(k, weights=v.astype(np.float64), minlength=S * O).reshape(S, O).astype(dtype)

    aB = np.zeros(S, dtype=dtype)
    aL = np.zeros(src.size, dtype=dtype)
    aB[graph.start] = 1
    la = 0.0
    AB, AL, LA = [], [], []
    for t in range(T):
        G = grid(aL, key)
        tot = G.sum(axis=1, dtype=dtype)
        oth = _others(G)
        nB = p[t, blank] * (aB + tot)
        nL = p[t, c] * (aL + wa * (aB[src] + oth[src, c]))
        m = max(nB.max(), nL.max() if nL.size else 0)
        if m > 0:
            e = int(np.frexp(np.float64(m))[1]) - 1  # the exact power of two that brings the maximum into [1, 2)
            nB, nL, la = np.ldexp(nB, -e).astype(dtype), np.ldexp(nL, -e).astype(dtype), la + e * np.log(2.0)
        aB, aL = nB.astype(dtype), nL.astype(dtype)
        AB.append(aB), AL.append(aL), LA.append(la)
    G = grid(aL, key)
    Z = float((f.astype(np.float64) * (aB + G.sum(axis=1, dtype=dtype)).astype(np.float64)).sum())
    if not Z > 0:
        return -np.inf, np.zeros((T, O))
    logz = la + np.log(Z)
    if not backward:
        return logz, None
    occ = np.zeros((T, O))
    bB, bL, lb = f.copy(), np.zeros(src.size, dtype=dtype), 0.0
    for t in range(T - 1, -1, -1):
        G = grid(wa * bL, skey)  # the out-arcs of a state: one per label
        tot = G.sum(axis=1, dtype=dtype)
        oth = _others(G)
        nB = p[t, blank] * (bB + tot)
        nL = p[t, c] * (bL + bB[dst] + oth[dst, c])
        m = max(nB.max(), nL.max() if nL.size else 0)
        if m > 0:
            e = int(np.frexp(np.float64(m))[1]) - 1  # (as above)
            nB, nL, lb = np.ldexp(nB, -e).astype(dtype), np.ldexp(nL, -e).astype(dtype), lb + e * np.log(2.0)
        bB, bL = nB.astype(dtype), nL.astype(dtype)
        sc = np.exp(LA[t] + lb - logz)
        with np.errstate(divide="ignore", invalid="ignore"):
            gB = (AB[t].astype(np.float64) * bB.astype(np.float64)).sum() * sc / np.float64(p[t, blank])
            gL = np.bincount(c, weights=AL[t].astype(np.float64) * bL.astype(np.float64), minlength=O) * sc / p[t].astype(
                np.float64)
        occ[t] = np.where(p[t] > 0, gL, 0.0)
        occ[t, blank] = gB if p[t, blank] > 0 else 0.0
        # the contract: a frame's occupancies are divided by their sum where that is within 1e-2 of one (in float64 the sum
        # is one to 1e-12; in float32 this takes out what the frame's states share -- the offsets' and log Z's round-off)
        tot = occ[t].sum()
        if abs(tot - 1.0) < 1e-2:
            occ[t] /= tot
    return logz, occ


def mmi_loss_grad64(z, ref, graph, lam=1.0, ctc_weight=0.0):
    """float64 statement of the criterion for ONE utterance: logits z [T, O], reference `ref`, denominator `graph` (a GraphLM;
    only table / next / start are read, the final weights always), scale lam.  Returns (loss, grad [T, O], log Z, occ_den):
      loss = -(log p_ctc(ref | z) + lam G(ref)) + log Z  (+ ctc_weight * -log p_ctc(ref | z)),
      grad = occ_den - occ_num + ctc_weight (softmax - occ_num),  occ_num = softmax - (the CTC oracle's gradient);
    +inf and a zero gradient when Z = 0, the graph rejects ref, or ref does not fit the frames."""
    z = np.asarray(z, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.int64).reshape(-1)
    logz, occ = den_forward_backward(z, graph, lam)
    ctc, g = ctc_loss_and_grad_vec(z, ref)
    gy = graph_score(graph, ref)
    if not (np.isfinite(ctc) and logz > -np.inf and gy > -np.inf):
        return np.inf, np.zeros_like(z), logz, np.zeros_like(z)
    with np.errstate(over="ignore"):
        soft = np.exp(z - z.max(axis=1, keepdims=True)) if z.shape[0] else z
        soft = soft / soft.sum(axis=1, keepdims=True) if z.shape[0] else z
    loss = -(-ctc + lam * gy) + logz + ctc_weight * ctc
    return loss, occ - soft + (1.0 + ctc_weight) * g, logz, occ


def mmi_tol(z, graph, lam=1.0, ctc_weight=0.0, ctc_loss=0.0):
    """The fp32 error model of the device for ONE utterance, from the restatement alone (as rescore_tol): the sweeps are run
    a second time with every value in float32 (offsets in float64, as the device keeps them), and the device is allowed 4 x
    the largest |float32 run - float64 run|, floored at 8 ulp of fp32 at the value's size (the device adds in another order
    than numpy, so a difference of zero is no bound): 1e-6 max(1, |log Z|) for log Z and 1e-6 for an occupancy (<= 1).
    The gradient and the loss also carry the NUMERATOR, the CTC loss's own kernels, at the tolerances tests/test_gpu_ctc.py
    holds them to: 2e-5 absolute on a gradient entry (times 1 + ctc_weight), 2e-5 relative on the CTC loss.
    Returns {"logz", "occ", "grad", "loss"}."""
    l64, o64 = den_forward_backward(z, graph, lam)
    l32, o32 = den_forward_backward(np.asarray(z, dtype=np.float32), graph, lam, dtype=np.float32)
    assert np.isfinite(l64) == np.isfinite(l32)
    dl = abs(l64 - l32) if np.isfinite(l64) else 0.0
    do = float(np.abs(o64 - o32).max()) if o64.size else 0.0
    tol_logz = max(4.0 * dl, 1e-6 * max(1.0, abs(l64) if np.isfinite(l64) else 0.0))
    tol_occ = max(4.0 * do, 1e-6)
    return {"logz": tol_logz, "occ": tol_occ, "grad": tol_occ + (1.0 + ctc_weight) * 2e-5,
            "loss": tol_logz + (1.0 + ctc_weight) * 2e-5 * abs(ctc_loss) + 1e-6}


def random_graph(rng, S, O, p_arc=0.7, p_final=0.7):
    """a random deterministic acceptor: some arcs missing, some states not final, self-loops and states entered by several
    labels all occur"""
    w = np.where(rng.random((S, O)) < p_arc, rng.normal(-1.0, 1.0, (S, O)), -np.inf)
    nxt = rng.integers(0, S, size=(S, O))
    nxt[np.isinf(w)] = -1
    w[:, O - 1] = np.where(rng.random(S) < p_final, rng.normal(-0.5, 0.5, S), -np.inf)
    if np.all(np.isinf(w[:, O - 1])):
        w[int(rng.integers(0, S)), O - 1] = 0.0
    nxt[:, O - 1] = -1
    return GraphLM(w, nxt, start=int(rng.integers(0, S)))


def free_graph(O):
    """one state, every arc at weight 0, final at weight 0: no constraint at all"""
    w = np.zeros((1, O), dtype=np.float32)
    return GraphLM(w, np.zeros((1, O), dtype=np.int64), start=0)


def _enumerated_logz(z, graph, lam):
    terms = [lp + lam * graph_score(graph, lab) for lab, lp in enumerate_labellings(z).items()
             if graph_score(graph, lab) > -np.inf]
    return float(np.logaddexp.reduce(np.array(terms))) if terms else -np.inf


def test_log_z_equals_exhaustive_enumeration():
    rng = np.random.default_rng(4200)
    seen_multi, seen_loop, seen_inf = 0, 0, 0
    for k in range(40):
        S, O, T = int(rng.integers(1, 4)), int(rng.integers(2, 5)), int(rng.integers(1, 6))
        g = random_graph(rng, S, O)
        src, c, dst, _, _ = graph_arcs(g)
        seen_loop += int(np.any(src == dst))
        seen_multi += int(any(len(set(c[dst == s])) >= 2 for s in range(S)))
        z = 2.0 * rng.standard_normal((T, O))
        for lam in (1.0, 0.5):
            want = _enumerated_logz(z, g, lam)
            got, _ = den_forward_backward(z, g, lam)
            if want == -np.inf:
                seen_inf += 1
                assert got == -np.inf
            else:
                assert abs(got - want) < 1e-12, (k, lam, got, want)
    assert seen_multi >= 5 and seen_loop >= 5


def test_gradient_equals_central_differences():
    rng = np.random.default_rng(4201)
    done = 0
    for k in range(30):
        S, O, T = int(rng.integers(1, 4)), int(rng.integers(2, 5)), int(rng.integers(2, 6))
        g = random_graph(rng, S, O, p_arc=0.85, p_final=0.9)
        z = rng.standard_normal((T, O))
        accepted = [lab for lab in enumerate_labellings(z) if graph_score(g, lab) > -np.inf and len(lab) > 0]
        if not accepted:
            continue
        ref = np.array(accepted[int(rng.integers(0, len(accepted)))])
        lam, cw = (1.0, 0.5)[k % 2], (0.0, 0.3)[k % 3 == 0]
        loss, grad, _, _ = mmi_loss_grad64(z, ref, g, lam, cw)
        assert np.isfinite(loss)
        num = np.zeros_like(z)
        h = 1e-6
        for i in range(T):
            for j in range(O):
                zp, zm = z.copy(), z.copy()
                zp[i, j] += h
                zm[i, j] -= h
                num[i, j] = (mmi_loss_grad64(zp, ref, g, lam, cw)[0] - mmi_loss_grad64(zm, ref, g, lam, cw)[0]) / (2 * h)
        assert np.abs(num - grad).max() < 1e-7, (k, np.abs(num - grad).max())
        done += 1
    assert done >= 15


def test_free_graph_is_the_plain_ctc_loss():
    rng = np.random.default_rng(4202)
    z = 2.0 * rng.standard_normal((9, 5))
    ref = np.array([1, 1, 3])
    for lam in (1.0, 0.3):
        loss, grad, logz, occ = mmi_loss_grad64(z, ref, free_graph(5), lam)
        ctc, g = ctc_loss_and_grad_vec(z, ref)
        assert abs(logz) < 1e-12
        assert abs(loss - ctc) < 1e-12
        assert np.abs(grad - g).max() < 1e-12
        assert np.abs(occ.sum(axis=1) - 1.0).max() < 1e-12


def test_loss_is_nonnegative_for_accepted_references():
    rng = np.random.default_rng(4203)
    n = 0
    for k in range(40):
        S, O, T = int(rng.integers(1, 4)), int(rng.integers(2, 5)), int(rng.integers(1, 6))
        g = random_graph(rng, S, O)
        z = 2.0 * rng.standard_normal((T, O))
        for lab in enumerate_labellings(z):
            if graph_score(g, lab) > -np.inf:
                loss = mmi_loss_grad64(z, np.array(lab, dtype=np.int64), g, 0.5)[0]
                assert loss >= -1e-12
                n += 1
    assert n > 50


def test_the_language_aa():
    # start -a-> 1 -a-> 2 (final): the repeated label needs a blank in between
    w = np.full((3, 3), -np.inf)
    nxt = np.full((3, 3), -1)
    w[0, 0], nxt[0, 0] = 0.0, 1
    w[1, 0], nxt[1, 0] = 0.0, 2
    w[2, 2] = 0.0
    g = GraphLM(w, nxt, start=0)
    rng = np.random.default_rng(4204)
    z2, z3 = rng.standard_normal((2, 3)), rng.standard_normal((3, 3))
    assert den_forward_backward(z2, g, 1.0)[0] == -np.inf
    loss, grad, _, _ = mmi_loss_grad64(z2, [0, 0], g)
    assert loss == np.inf and not grad.any()
    logz, occ = den_forward_backward(z3, g, 1.0)
    lp = z3 - np.log(np.exp(z3).sum(axis=1, keepdims=True))
    assert abs(logz - (lp[0, 0] + lp[1, 2] + lp[2, 0])) < 1e-12  # the one alignment a, blank, a
    assert np.allclose(occ, np.array([[1, 0, 0], [0, 0, 1], [1, 0, 0.0]]), atol=1e-12)
    assert abs(mmi_loss_grad64(z3, [0, 0], g)[0]) < 1e-12
    # no frames: only the empty sequence, accepted if the start is final
    assert mmi_loss_grad64(np.zeros((0, 3)), E, g)[0] == np.inf
    assert mmi_loss_grad64(np.zeros((0, 3)), E, free_graph(3))[0] == 0.0


def test_mmi_tol_is_a_bound_from_the_formats():
    rng = np.random.default_rng(4205)
    z = 3.0 * rng.standard_normal((30, 4))
    g = random_graph(rng, 3, 4, p_arc=0.9, p_final=1.0)
    tol = mmi_tol(z, g, 1.0, ctc_loss=50.0)
    assert 1e-6 <= tol["logz"] < 1e-3 and 1e-6 <= tol["occ"] < 1e-4
    assert tol["grad"] > tol["occ"] and tol["loss"] > tol["logz"]


def test_graphlm_counts():
    lex = GraphLM.from_lexicon([[0, 1], [0, 2], [3]], num_labels=5, separator=4)
    S = lex.num_states
    assert S == 5 and lex.num_arcs == 4 + 3 and lex.composed_states == S + 7
    assert free_graph(6).num_arcs == 5 and free_graph(6).composed_states == 6
    lm = NgramLM.from_label_sequences([[0, 1, 2], [2, 1]], num_labels=35, order=3)
    g = GraphLM.from_ngram(lm)
    assert g.num_states == 36 * 36 and g.num_arcs == 36 * 36 * 35 and g.composed_states == 46656


class _StubDP(object):
    def __init__(self):
        self.train, self.evals = [], []

    def train_step(self, engine, mbs):
        self.train.append(mbs)
        return 1.5

    def eval_step(self, engine, mbs):
        self.evals.append(mbs)
        return 2.5


def _stub_trainer():
    from tfkaldi_amd.dataparallel import CtcMicroBatch
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    t = CTCTrainer.__new__(CTCTrainer)
    t.dp, t.engine = _StubDP(), object()
    t._summarise = lambda loss: None

    def microbatches(inputs, targets):
        X = np.concatenate(inputs)
        lab = np.concatenate([np.asarray(x, dtype=np.int32) for x in targets])
        return [CtcMicroBatch(X, np.array([len(x) for x in inputs], np.int32), lab,
                              np.array([len(x) for x in targets], np.int32))]
    t._microbatches = microbatches
    return t


def test_update_mmi_rejects_a_reference_the_graph_does_not_accept():
    t = _stub_trainer()
    lex = GraphLM.from_lexicon([[0, 1], [2]], num_labels=4, separator=3)
    X = [np.zeros((6, 2), np.float32), np.zeros((5, 2), np.float32)]
    with pytest.raises(ValueError, match="utterance 1"):
        t.update_mmi(X, [[0, 1], [1]], lex)          # no arc
    with pytest.raises(ValueError, match="utterance 0.*not final"):
        t.update_mmi(X, [[0], [2]], lex)             # ends inside a word
    with pytest.raises(ValueError, match="lm_scale"):
        t.update_mmi(X, [[0, 1], [2]], lex, lm_scale=-1.0)
    with pytest.raises(ValueError, match="GraphLM"):
        t.update_mmi(X, [[0, 1], [2]], NgramLM.from_label_sequences([[0]], 4, 2))
    assert not t.dp.train
    assert t.update_mmi(X, [[0, 1], [2, 3, 0, 1]], lex, lm_scale=0.5, ctc_weight=0.1) == 1.5
    mb, = t.dp.train[0]
    assert mb.graph is lex and mb.lm_scale == 0.5 and mb.ctc_weight == 0.1
    assert t.evaluate_mmi(X, [[0, 1], [2]], lex) == 2.5 and t.evaluate_mmi(None, None, lex) is None


class _StubEngine(object):
    def __init__(self):
        self.calls = []

    def ctc_set_den(self, graph):
        self.calls.append(("den", graph))

    def accumulate_ctc_mmi(self, X, utt_lens, labels, label_lens, **kw):
        self.calls.append(("mmi", kw))

    def accumulate_ctc_mmi_raw(self, X, utt_lens, context_width, labels, label_lens, **kw):
        self.calls.append(("mmi_raw", context_width, kw))


def test_dispatch_of_a_mmi_microbatch():
    from tfkaldi_amd.dataparallel import CtcMmiMicroBatch, _accumulate, _eval_accumulate
    g = free_graph(4)
    X, ul, lab, ll = np.zeros((4, 2), np.float32), np.array([4], np.int32), np.array([1], np.int32), np.array([1], np.int32)
    eng = _StubEngine()
    _accumulate(eng, CtcMmiMicroBatch(X, ul, lab, ll, g, lm_scale=0.5, ctc_weight=0.2), True)
    assert eng.calls == [("den", g), ("mmi", dict(lm_scale=0.5, ctc_weight=0.2, last=True, train=True))]
    eng = _StubEngine()
    _eval_accumulate(eng, CtcMmiMicroBatch(X, ul, lab, ll, g, context_width=3, cmvn=None))
    assert eng.calls == [("den", g), ("mmi_raw", 3, dict(lm_scale=1.0, ctc_weight=0.0, last=False, cmvn=None, train=False))]
    with pytest.raises(ValueError):
        CtcMmiMicroBatch(X, ul, lab, ll, None)
