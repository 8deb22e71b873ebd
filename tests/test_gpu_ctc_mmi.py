"""MMI against a denominator graph on the device (include/tfkaldi_hip.h at tfk_accumulate_ctc_mmi): tfk_ctc_mmi_logits
against the float64 restatement of tests/test_ctc_mmi_host.py (mmi_loss_grad64) within its fp32 error model (mmi_tol) at the
kernel's own edges -- composed-state counts around the wave, the workgroup sizes and the LDS / global residences, frame counts
around the prefetch ring, graph shapes that exercise the exclusion sums -- against the CTC loss (a graph without constraint),
against tfk_ctc_score_logits (a finite language), its refusals, and the engine entries up to CTCTrainer.update_mmi.  Every
comparison prints its worst error beside its bound (recorded in profiles/ctc_mmi_edges.txt)."""
from ctypes import c_void_p

import numpy as np
import pytest

from oracle.ctc_oracle import ctc_loss_and_grad_vec
from test_ctc_mmi_host import free_graph, graph_arcs, graph_score, mmi_loss_grad64, mmi_tol, random_graph
from test_ctc_score_host import rescore_tol
from test_gpu_ctc_beam_topk import _engine_state
from test_gpu_ctc_score import _device_score_logits
from tfkaldi_amd.neuralNetworks.ctc_lm import GraphLM, NgramLM
from util import assert_close, engine_grads, engine_params, make_pair

pytestmark = pytest.mark.gpu

E = np.zeros(0, np.int32)
SENT = 12345.0


def _device_mmi(z, utt, refs, graph, lam=1.0, cw=0.0, grad=True, pad=3, dpad=2, in_place=False):
    """tfk_ctc_mmi_logits on host logits [sum(utt), O] laid out with ld = O + pad (NaN in the padding columns); returns
    (utt_loss [U], logz [U], dlogits [T, O] or None).  The element after each output must come back untouched, the padding
    columns of dlogits as zeros, and the logits unchanged (unless dlogits is the logits: in_place)."""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    T, O = z.shape
    U = len(utt)
    if in_place:
        dpad = pad
    full = np.full((T, O + pad), np.nan, np.float32)
    full[:, :O] = z
    seg = np.concatenate([[0], np.cumsum(utt)]).astype(np.int32)
    rflat = [np.asarray(r, np.int32).reshape(-1) for r in refs]
    lab_off = np.concatenate([[0], np.cumsum([r.size for r in rflat])]).astype(np.int32)
    labels = np.concatenate(rflat + [np.zeros(1, np.int32)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_z, d_seg, d_off, d_lab = dev(full), dev(seg), dev(lab_off), dev(labels)
    d_w, d_n = dev(graph.table), dev(graph.next)
    loss = torch.full((U + 1,), SENT, dtype=torch.float32, device="cuda")
    logz = torch.full((U + 1,), SENT, dtype=torch.float32, device="cuda")
    dlog = (d_z if in_place else torch.full((T, O + dpad), SENT, dtype=torch.float32, device="cuda")) if grad else None
    _lib.check(lib.tfk_ctc_mmi_logits(c_void_p(torch.cuda.current_stream().cuda_stream), c_void_p(d_z.data_ptr()), O + pad, O, T,
                                      c_void_p(d_seg.data_ptr()), U, c_void_p(d_lab.data_ptr()), c_void_p(d_off.data_ptr()),
                                      c_void_p(d_w.data_ptr()), c_void_p(d_n.data_ptr()), graph.num_states, graph.start,
                                      float(lam), float(cw), c_void_p(loss.data_ptr()), c_void_p(logz.data_ptr()),
                                      c_void_p(dlog.data_ptr() if grad else None), O + dpad))
    torch.cuda.synchronize()
    loss, logz = loss.cpu().numpy(), logz.cpu().numpy()
    assert loss[U] == SENT and logz[U] == SENT
    if not in_place:
        assert np.array_equal(d_z.cpu().numpy(), full, equal_nan=True)
    if grad:
        dlog = dlog.cpu().numpy()
        assert np.all(dlog[:, O:] == 0.0)
        dlog = dlog[:, :O]
    return loss[:U], logz[:U], dlog


def _check(name, z, utt, refs, graph, lam=1.0, cw=0.0, **kw):
    """every utterance against mmi_loss_grad64 within mmi_tol; prints the worst error beside its bound"""
    loss, logz, dlog = _device_mmi(z, utt, refs, graph, lam, cw, **kw)
    zs = np.split(np.asarray(z, np.float32), np.cumsum(utt)[:-1])
    ds = np.split(dlog, np.cumsum(utt)[:-1])
    worst = {"logz": (0.0, 0.0), "loss": (0.0, 0.0), "grad": (0.0, 0.0)}
    for u, (zu, du) in enumerate(zip(zs, ds)):
        w_loss, w_grad, w_logz, _ = mmi_loss_grad64(zu, refs[u], graph, lam, cw)
        ctc = ctc_loss_and_grad_vec(zu.astype(np.float64), np.asarray(refs[u], np.int64).reshape(-1))[0]
        tol = mmi_tol(zu, graph, lam, cw, ctc if np.isfinite(ctc) else 0.0)
        if np.isfinite(w_loss):
            w_loss -= cw * ctc  # (utt_loss is loss_u alone: the ctc_weight term joins in the batch's sum)
        assert np.isfinite(w_logz) == np.isfinite(logz[u]), (name, u, w_logz, logz[u])
        assert np.isfinite(w_loss) == np.isfinite(loss[u]), (name, u, w_loss, loss[u])
        errs = {"logz": abs(logz[u] - w_logz) if np.isfinite(w_logz) else 0.0,
                "loss": abs(loss[u] - w_loss) if np.isfinite(w_loss) else 0.0,
                "grad": float(np.abs(du - w_grad).max()) if du.size else 0.0}
        if not np.isfinite(w_loss):
            assert loss[u] == np.inf and not du.any(), (name, u)
        for k, e in errs.items():
            # (the outputs are float32: half an ulp of the value on top of the model's bound)
            bound = tol[k] + (6e-8 * abs(w_logz if k == "logz" else w_loss) if k != "grad" and np.isfinite(w_loss) else 0.0)
            if e / bound >= worst[k][0] / max(worst[k][1], 1e-300):
                worst[k] = (e, bound)
            assert e <= bound, (name, u, k, e, bound)
    print("ctc-mmi edge %-44s N %6d  logz %.1e / %.1e  loss %.1e / %.1e  grad %.1e / %.1e"
          % (name, graph.composed_states, worst["logz"][0], worst["logz"][1], worst["loss"][0], worst["loss"][1],
             worst["grad"][0], worst["grad"][1]))
    return loss, logz, dlog


def _logits(rng, T, O, scale=2.0):
    return (scale * rng.standard_normal((T, O))).astype(np.float32)


def _sample_ref(rng, graph, maxlen):
    """a label sequence the graph accepts: a random walk from the start that stops in a final state (None: found none)"""
    for _ in range(200):
        s, out = graph.start, []
        for _ in range(maxlen + 1):
            if graph.table[s, -1] > -np.inf and (len(out) == maxlen or rng.random() < 0.3):
                return np.array(out, np.int32)
            arcs = np.flatnonzero(graph.table[s, :-1] > -np.inf)
            if arcs.size == 0 or len(out) == maxlen:
                break
            c = int(rng.choice(arcs))
            out.append(c)
            s = int(graph.next[s, c])
    return None


def _sized_graph(rng, S, O, N):
    """S states, all final, and exactly N - S arcs with random weights and targets"""
    A = N - S
    assert 0 <= A <= S * (O - 1)
    w = np.full((S, O), -np.inf)
    nxt = np.full((S, O), -1, dtype=np.int64)
    pick = rng.permutation(S * (O - 1))[:A]
    s, c = pick // (O - 1), pick % (O - 1)
    w[s, c] = rng.normal(-1.0, 0.7, A)
    nxt[s, c] = rng.integers(0, S, A)
    w[:, O - 1] = rng.normal(-0.5, 0.3, S)
    return GraphLM(w, nxt, start=0)


def _residence(graph):
    """where the library keeps the sweeps' data for this graph (tfk_ctc_den_info): "global", "lds" or "lds+tables"""
    from tfkaldi_amd import _lib
    from tfkaldi_amd.engine import Engine
    eng = Engine(_lib.make_config(4, 1, 8, graph.num_classes, max_frames=8))
    eng.ctc_set_den(graph)
    info = eng.ctc_den_info()
    eng.close()
    assert info["composed_states"] == graph.composed_states and info["num_arcs"] == graph.num_arcs
    return info["residence"], info


def _boundary_pair(rng, S, O, N0, leaves):
    """(last graph that is still `leaves`' residence, first that is not, their infos) along ONE family: a graph of N0 composed
    states, then arcs added one at a time in a fixed order, each on a label its target is already entered by (so an arc adds
    ONE composed state and no group: one float of the vector, six words with the tables).  The library says on which side a
    graph is; the boundary is found by bisection over the number of added arcs."""
    base = _sized_graph(rng, S, O, N0)
    w, nxt = base.table.astype(np.float64), base.next.astype(np.int64)
    nxt[~(w > -np.inf)] = -1
    entered = {}
    for s, c in zip(*np.nonzero(w[:, :O - 1] > -np.inf)):
        entered.setdefault(int(c), []).append(int(nxt[s, c]))
    free = [(int(s), int(c)) for s, c in zip(*np.nonzero(~(w[:, :O - 1] > -np.inf))) if int(c) in entered]
    free = [free[i] for i in rng.permutation(len(free))]
    adds = [(s, c, entered[c][int(rng.integers(0, len(entered[c])))], float(rng.normal(-1.0, 0.7))) for s, c in free]

    def graph(k):
        w2, n2 = w.copy(), nxt.copy()
        for s, c, d, x in adds[:k]:
            w2[s, c], n2[s, c] = x, d
        return GraphLM(w2, n2, start=0)
    lo, hi = 0, len(adds)
    assert _residence(graph(lo))[0] == leaves and _residence(graph(hi))[0] != leaves
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _residence(graph(mid))[0] == leaves:
            lo = mid
        else:
            hi = mid
    return graph(lo), graph(hi)


def _two_refs(rng, graph, maxlen):
    a, b = _sample_ref(rng, graph, maxlen), _sample_ref(rng, graph, max(maxlen // 2, 1))
    assert a is not None and b is not None
    return [a, b]


# ---- a graph without constraint is the CTC loss ----
@pytest.mark.parametrize("lam", [1.0, 0.3])
def test_identity_with_the_ctc_loss(gpu, lam):
    rng = np.random.default_rng(6000)
    O, utt = 9, [40, 7, 150]
    refs = [rng.integers(0, O - 1, 9).astype(np.int32), np.array([2, 2, 5], np.int32), rng.integers(0, 2, 40).astype(np.int32)]
    z = _logits(rng, sum(utt), O)
    loss, logz, dlog = _device_mmi(z, utt, refs, free_graph(O), lam)
    zs, ds = np.split(z, np.cumsum(utt)[:-1]), np.split(dlog, np.cumsum(utt)[:-1])
    for u in range(3):
        ctc, g = ctc_loss_and_grad_vec(zs[u].astype(np.float64), refs[u].astype(np.int64))
        tol = mmi_tol(zs[u], free_graph(O), lam)
        print("ctc-mmi identity lam %.1f utt %d: |logz| %.1e / %.1e  loss %.1e rel  grad %.1e"
              % (lam, u, abs(logz[u]), tol["logz"], abs(loss[u] - ctc) / ctc, np.abs(ds[u] - g).max()))
        assert abs(logz[u]) <= tol["logz"]
        assert_close("loss", loss[u], ctc, 2e-5, 0)
        assert_close("dlogits", ds[u], g, rtol=1e-4, atol=2e-5)


# ---- a finite language: log Z is the log-sum over its words of the exact scores ----
def test_finite_language_against_the_rescoring_entry(gpu):
    rng = np.random.default_rng(6001)
    O = 7
    words = [np.array(w, np.int32) for w in ([0, 1], [0, 2, 2], [3], [1, 0, 3, 4], [5, 5])]
    logp = np.array([-0.5, -2.0, -1.0, -0.3, -1.5])
    utt = [12, 6, 30]
    z = _logits(rng, sum(utt), O)
    for lam in (1.0, 0.4):
        g = GraphLM.from_lexicon(words, O - 1, None, word_logprob=logp)
        _, logz, _ = _device_mmi(z, utt, [words[0], words[2], words[3]], g, lam, grad=False)
        scores = _device_score_logits(z, utt, [words] * 3)
        zs = np.split(z, np.cumsum(utt)[:-1])
        for u in range(3):
            s = np.asarray(scores[u], np.float64)
            want = float(np.logaddexp.reduce(s + lam * logp.astype(np.float32).astype(np.float64)))
            _, rt = rescore_tol([zs[u]] * len(words), words)
            bound = float(np.sum(np.where(np.isfinite(s), rt, 0.0))) + mmi_tol(zs[u], g, lam)["logz"] + 6e-8 * abs(want)
            print("ctc-mmi finite language lam %.1f utt %d: logz %.6f, from the scores %.6f, |diff| %.1e / %.1e"
                  % (lam, u, logz[u], want, abs(logz[u] - want), bound))
            assert abs(logz[u] - want) <= bound


# ---- the kernel's own edges ----
@pytest.mark.parametrize("N", [2, 63, 64, 65, 257, 2048, 2049])
def test_composed_state_counts(gpu, N):
    """around the wave (63, 64, 65), one more than the small workgroup's 256 threads, and the switch to 1024 threads (N > 2048)"""
    rng = np.random.default_rng(6100 + N)
    S, O = (1, 2) if N == 2 else (3, 33) if N <= 65 else (9, 40) if N == 257 else (60, 40)
    g = _sized_graph(rng, S, O, N)
    assert g.composed_states == N
    utt = [9, 14]
    _check("N = %d" % N, _logits(rng, sum(utt), O), utt, _two_refs(rng, g, 4), g, lam=0.7, cw=0.2)


@pytest.mark.parametrize("N", [400, 1024, 1025])
def test_more_classes_than_the_small_workgroup(gpu, N):
    """O > 256 takes the 1024-thread form whatever N is: below its thread count, at it, and one more (its own tail)"""
    rng = np.random.default_rng(6150 + N)
    g = _sized_graph(rng, 4, 300, N)
    _check("O = 300, N = %d" % N, _logits(rng, 11, 300), [11], [_sample_ref(rng, g, 3)], g)


def test_first_graph_that_leaves_lds(gpu):
    """the last N whose vector and sums fit the workgroup's LDS and the first that does not: one arc, one float apart"""
    rng = np.random.default_rng(6160)
    O = 36
    inside, outside = _boundary_pair(rng, 800, O, 23000, "lds")
    assert outside.composed_states == inside.composed_states + 1
    for g in (inside, outside):
        where, info = _residence(g)
        utt = [6, 9]
        _check("%s residence, N + S + K = %d" % (where, info["composed_states"] + info["num_states"] + info["num_groups"]),
               _logits(rng, sum(utt), O), utt, _two_refs(rng, g, 3), g, lam=0.5)


def test_last_graph_whose_tables_fit_lds(gpu):
    """the same pair for the second residence: the index tables and arc weights beside the vector, or read from global memory"""
    rng = np.random.default_rng(6161)
    O = 40
    inside, outside = _boundary_pair(rng, 150, O, 150 + 3700, "lds+tables")
    assert outside.composed_states == inside.composed_states + 1 and _residence(outside)[0] == "lds"
    for g in (inside, outside):
        where, info = _residence(g)
        utt = [7, 5]
        _check("%s, S %d A %d K %d" % (where, info["num_states"], info["num_arcs"], info["num_groups"]),
               _logits(rng, sum(utt), O), utt, _two_refs(rng, g, 3), g, lam=0.5)


def test_order_3_ngram_over_36_outputs(gpu):
    rng = np.random.default_rng(6170)
    seqs = [rng.integers(0, 35, 30) for _ in range(20)]
    g = GraphLM.from_ngram(NgramLM.from_label_sequences(seqs, 35, 3))
    assert g.composed_states == 46656
    _check("order-3 n-gram, T = 40", _logits(rng, 40, 36), [40], [seqs[0][:12].astype(np.int32)], g, lam=0.8)


def test_frame_counts(gpu):
    """1 frame; 2 frames with a repeated label (infeasible: it needs a blank); every count around the 4-row prefetch ring (the
    re-centring period is ONE frame, so 1, 2 and 3 frames are the counts that straddle it)"""
    rng = np.random.default_rng(6200)
    O = 6
    g = random_graph(rng, 4, O, p_arc=0.9, p_final=1.0)
    utt = [1, 2, 3, 4, 5, 7, 8, 9]
    a = int(np.flatnonzero(g.table[g.start, :-1] > -np.inf)[0])
    refs = [np.array([a], np.int32), np.array([0, 0], np.int32)] + [_sample_ref(rng, g, 2) for _ in utt[2:]]
    loss, _, _ = _check("T = 1 .. 9", _logits(rng, sum(utt), O), utt, refs, g, lam=1.0)
    assert loss[1] == np.inf and np.isfinite(loss[0])


def test_1500_peaked_frames(gpu):
    """the double offsets: log Z runs into the thousands"""
    rng = np.random.default_rng(6210)
    O, T = 8, 1500
    g = random_graph(rng, 5, O, p_arc=0.6, p_final=1.0)
    z = _logits(rng, T, O, 1.0)
    z[np.arange(T), rng.integers(0, O, T)] += 14.0
    ref = _sample_ref(rng, g, 60)
    _, logz, _ = _check("T = 1500, peaked", z, [T], [ref], g, lam=1.0)
    assert abs(logz[0]) > 100.0


def test_batch_with_zero_frame_and_infeasible_utterances(gpu):
    rng = np.random.default_rng(6220)
    O = 6
    g = random_graph(rng, 3, O, p_arc=0.9, p_final=1.0)
    utt = [12, 0, 3, 0, 20]
    refs = [_sample_ref(rng, g, 4), E, np.arange(5, dtype=np.int32) % (O - 1), np.array([1], np.int32), _sample_ref(rng, g, 6)]
    loss, logz, _ = _check("zero-frame / infeasible / ordinary", _logits(rng, sum(utt), O), utt, refs, g, lam=0.6)
    assert loss[1] == 0.0 and loss[2] == np.inf and loss[3] == np.inf and np.isfinite(loss[[0, 4]]).all()
    # a start that is not final: the zero-frame utterance has no accepted sequence
    lex = GraphLM.from_lexicon([[0, 1]], O - 1, None)
    loss, logz, _ = _check("zero frames, start not final", _logits(rng, 8, O), [8, 0], [np.array([0, 1], np.int32), E], lex)
    assert loss[1] == np.inf and logz[1] == -np.inf


def _exclusion_graph():
    """state 1 is entered on labels 0, 1 and 2 (two arcs on 0) and leaves on each of them; state 2 has a self-loop; state 3 is
    a dead end that is not final; state 4 cannot be reached"""
    O, S = 5, 5
    w = np.full((S, O), -np.inf)
    nxt = np.full((S, O), -1, dtype=np.int64)
    for s, c, d, x in [(0, 0, 1, -0.1), (0, 1, 1, -0.7), (0, 2, 2, -0.3), (2, 0, 1, -0.2), (2, 2, 2, -0.9), (2, 1, 3, -0.4),
                       (1, 0, 2, -0.5), (1, 1, 0, -0.6), (1, 2, 1, -0.8), (1, 3, 3, -1.0), (4, 0, 0, -0.1), (4, 3, 4, -0.2)]:
        w[s, c], nxt[s, c] = x, d
    w[[0, 1, 2, 4], O - 1] = [-0.3, 0.0, -1.2, -0.5]
    return GraphLM(w, nxt, start=0)


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_graph_shapes(gpu, lam):
    rng = np.random.default_rng(6300)
    g = _exclusion_graph()
    utt = [15, 9]
    refs = [np.array([0, 2, 2, 1], np.int32), np.array([2, 2, 0], np.int32)]
    assert all(graph_score(g, r) > -np.inf for r in refs)
    _check("exclusion / self-loop / dead end / unreachable, lam %.1f" % lam, _logits(rng, sum(utt), 5), utt, refs, g, lam, cw=0.1)
    seqs = [rng.integers(0, 7, 12) for _ in range(6)]
    bi = GraphLM.from_ngram(NgramLM.from_label_sequences(seqs, 7, 2))
    _check("order-2 n-gram, lam %.1f" % lam, _logits(rng, 26, 8), [26], [seqs[0][:8].astype(np.int32)], bi, lam)


def _lexicon(rng, O=36, words=50):
    seen, out = set(), []
    while len(out) < words:
        w = tuple(rng.integers(0, O - 2, int(rng.integers(2, 7))).tolist())
        if w not in seen:
            seen.add(w)
            out.append(np.array(w, np.int32))
    return out, GraphLM.from_lexicon(out, O - 1, O - 2, word_logprob=rng.normal(-3.0, 1.0, words))


def test_lexicon_trie_with_the_separator_arc(gpu):
    rng = np.random.default_rng(6310)
    words, g = _lexicon(rng)
    sep = np.array([34], np.int32)
    ref = np.concatenate([words[3], sep, words[17], sep, words[3]])
    _check("50-word lexicon trie", _logits(rng, 60, 36), [60], [ref], g, lam=0.3, cw=0.5)


def test_two_calls_give_the_same_bits_and_in_place_is_the_same(gpu):
    rng = np.random.default_rng(6400)
    g = _exclusion_graph()
    utt, refs = [15, 9], [np.array([0, 2, 2, 1], np.int32), np.array([2, 2, 0], np.int32)]
    z = _logits(rng, sum(utt), 5)
    a = _device_mmi(z, utt, refs, g, 0.7, 0.2)
    b = _device_mmi(z, utt, refs, g, 0.7, 0.2)
    c = _device_mmi(z, utt, refs, g, 0.7, 0.2, in_place=True)
    for x, y, w in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == w.tobytes()


def test_refusals(gpu):
    """65537 composed states, no denominator, a refused tfk_ctc_den_set: a message, and what was there goes on working"""
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    from tfkaldi_amd.engine import Engine
    rng = np.random.default_rng(6500)
    O = 36
    big = _sized_graph(rng, 1900, O, 65537)
    with pytest.raises(EngineError, match="65537 composed states, limit 65536"):
        _device_mmi(_logits(rng, 4, O), [4], [E], big, grad=False)
    ok = _sized_graph(rng, 1900, O, 65536)
    loss, logz, _ = _device_mmi(_logits(rng, 4, O), [4], [E], ok, grad=False)
    assert np.isfinite(logz[0])
    kw = dict(input_dim=10, num_layers=1, num_units=16, output_dim=O, nonlin="relu", batch_norm=False,
              init_learning_rate=1e-3, num_steps=10)
    eng = Engine(_lib.make_config(max_frames=64, **kw))
    X, utt, lab, ll = rng.standard_normal((20, 10)).astype(np.float32), [20], np.array([1, 2], np.int32), np.array([2], np.int32)
    with pytest.raises(EngineError, match="no denominator graph"):
        eng.accumulate_ctc_mmi(X, utt, lab, ll)
    small = _sized_graph(rng, 4, O, 4 + 4 * 35)
    eng.ctc_set_den(small)
    eng.accumulate_ctc_mmi(X, utt, lab, ll, train=False)
    want = eng.eval_finish()
    with pytest.raises(EngineError, match="limit 65536"):
        eng.ctc_set_den(big)
    bad = small.next.copy()
    bad[0, 0] = 99
    with pytest.raises(EngineError, match="next"):
        _lib.check(eng.lib.tfk_ctc_den_set(eng._h, small.table.ctypes.data_as(c_void_p), bad.ctypes.data_as(c_void_p), 4, 0))
    for kind, args in (("lm_scale", (-1.0, 0.0)), ("ctc_weight", (1.0, float("nan")))):
        with pytest.raises(EngineError, match=kind):
            ptr = lambda a: a.ctypes.data_as(c_void_p)
            ul = np.asarray(utt, np.int32)
            _lib.check(eng.lib.tfk_accumulate_ctc_mmi(eng._h, ptr(X), 10, 20, ptr(ul), 1, ptr(lab), ptr(ll), args[0], args[1], 0))
    assert eng.ctc_den_info()["num_states"] == 4  # (the refused calls left the old model in force, here and in Python)
    eng.ctc_set_den(small)  # (nothing to upload: it is the model in force)
    eng.accumulate_ctc_mmi(X, utt, lab, ll, train=False)
    assert eng.eval_finish() == want and np.isfinite(want)
    eng.ctc_set_den(None)
    with pytest.raises(EngineError, match="no denominator graph"):
        eng.accumulate_ctc_mmi(X, utt, lab, ll)
    with pytest.raises(EngineError, match="no denominator graph"):
        eng.ctc_den_info()
    eng.close()


# ---- through the engine ----
KW4 = dict(input_dim=20, num_layers=4, num_units=64, output_dim=9, nonlin="tanh", batch_norm=True, init_learning_rate=1e-3,
           num_steps=50)


def _engine_case(dtype, seed=6600):
    """the 4 x 64 net (tanh, batch norm), three utterances and a lexicon with a separator.  "bfloat16": the same depth on the
    relu chain of tests/test_gpu_bf16_mode.py without batch norm -- that file's bound (2e-3) says "a handful of flipped
    operands", and at four layers WITH batch norm the engine's bf16 backward pass is already 2.3e-3 from the bf16 oracle under
    the plain CTC loss (W0; tools/ctc_mmi_bf16_depth.py measures it, profiles/ctc_mmi_edges.txt records it), a property of
    that path and not of the criterion.  "bfloat16-bn2": tanh and batch norm at TWO layers of 64, where that path is inside
    the bound: the gradient kernel's bf16 twin feeding a batch-norm backward pass.  "bfloat16-bn4": the four-layer net itself
    in bf16 mode, for test_training_call_links_at_four_layers (the whole-network bound cannot hold there, the links do)."""
    rng = np.random.default_rng(seed)
    kw = {"bfloat16": dict(KW4, nonlin="relu", batch_norm=False), "bfloat16-bn2": dict(KW4, num_layers=2),
          "bfloat16-bn4": KW4}.get(dtype, KW4)
    eng, oracle = make_pair(rng, max_frames=512, compute_dtype=dtype.split("-")[0], **kw)
    words = [np.array(w, np.int32) for w in ([0, 1, 2], [0, 3], [4, 4, 5], [6], [2, 1])]
    lex = GraphLM.from_lexicon(words, 8, 7, word_logprob=[-1.0, -0.5, -2.0, -1.5, -0.7])
    sep = np.array([7], np.int32)
    refs = [np.concatenate([words[0], sep, words[2]]), words[3], np.concatenate([words[4], sep, words[1], sep, words[3]])]
    utt = [60, 35, 48]
    X = (rng.standard_normal((sum(utt), KW4["input_dim"])) * 1.5).astype(np.float32)
    return eng, oracle, utt, X, refs, lex


def _restated_batch(z, utt, refs, lex, lam, cw):
    zs = np.split(np.asarray(z, np.float64), np.cumsum(utt)[:-1])
    want = [mmi_loss_grad64(zs[u], refs[u], lex, lam, cw) for u in range(len(utt))]
    return sum(w[0] for w in want), np.concatenate([w[1] for w in want])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "bfloat16-bn2"])
def test_training_call(gpu, dtype):
    """batch_loss, num_frames, dLogits and the parameter gradients against the restatement on the oracle's train-mode logits,
    run through the oracle's backward pass; fp32 at the tolerances of tests/test_gpu_ctc_mwer.py's engine test, bf16 at those
    of tests/test_gpu_bf16_mode.py (relative Frobenius error <= 2e-3, loss rtol 5e-4)"""
    from tfkaldi_amd import _lib
    eng, oracle, utt, X, refs, lex = _engine_case(dtype)
    lam, cw, T = 0.6, 0.3, sum(utt)
    labels, lab = np.concatenate(refs).astype(np.int32), np.array([r.size for r in refs], np.int32)
    eng.ctc_set_den(lex)
    eng.accumulate_ctc_mmi(X, utt, labels, lab, lm_scale=lam, ctc_weight=cw)
    z = oracle.forward_logits(X)
    loss, dlog = _restated_batch(z, utt, refs, lex, lam, cw)
    oracle.backward_from_dlogits(dlog, loss, int(lab.sum()))
    got_loss, got_n = eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES)
    got_dlog, got = eng.debug_fetch(_lib.DBG_LOGITS, 0, T), engine_grads(eng)
    keys = [k for k in oracle.G if not (oracle.bn and k.startswith("b") and not k.startswith("beta") and k != "b%d" % oracle.L)]
    fro = lambda g, w: float(np.linalg.norm(np.asarray(g, np.float64) - w) / max(np.linalg.norm(w), 1e-30))
    print("ctc-mmi training %-12s loss %.1e dlogits max %.1e fro %.1e | gradients fro %s"
          % (dtype, abs(got_loss - loss) / loss, np.abs(got_dlog - dlog).max(), fro(got_dlog, dlog),
             " ".join("%s %.1e" % (k, fro(got[k], oracle.G[k])) for k in keys)))
    assert got_n == lab.sum() and np.abs(dlog).max() > 1e-2 and loss > 0
    if dtype.startswith("bfloat16"):
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


def test_training_call_links_at_four_layers(gpu):
    """The four-layer tanh + batch-norm net in bf16 mode, the case test_training_call could not keep under its whole-network
    2e-3: every LINK of the step on the engine's own operands instead (tests/test_gpu_bf16_links.py; oracle/dnn_oracle.py:
    bf16_links) -- each contraction, the statistics, the MMI gradient under mmi_tol on the engine's own logits and its bf16
    twin bit for bit, batch norm backward, every gradient sum.  The deviation from the oracle is printed beside them: it is the
    rounding cascade of two correct computations, not a defect of a link."""
    from test_gpu_bf16_links import mmi_criterion
    from tfkaldi_amd import _lib
    from util import assert_links, engine_link_taps
    eng, oracle, utt, X, refs, lex = _engine_case("bfloat16-bn4")
    lam, cw = 0.6, 0.3
    labels, lab = np.concatenate(refs).astype(np.int32), np.array([r.size for r in refs], np.int32)
    eng.ctc_set_den(lex)
    eng.debug_capture(True)
    eng.accumulate_ctc_mmi(X, utt, labels, lab, lm_scale=lam, ctc_weight=cw)
    assert eng.scalar(_lib.NUM_FRAMES) == lab.sum()
    ratios = assert_links("ctc-mmi training bfloat16-bn4", oracle, engine_link_taps(eng, oracle, X), mmi_criterion(utt, refs, lex, lam, cw))
    z = oracle.forward_logits(X)
    loss, dlog = _restated_batch(z, utt, refs, lex, lam, cw)
    oracle.backward_from_dlogits(dlog, loss, int(lab.sum()))
    got = engine_grads(eng)
    fro = lambda g, w: float(np.linalg.norm(np.asarray(g, np.float64) - w) / max(np.linalg.norm(w), 1e-30))
    print("ctc-mmi training bfloat16-bn4: worst link %.3f | whole-network gradients fro %s" % (
        max(ratios.values()), " ".join("%s %.1e" % (k, fro(got[k], oracle.G[k])) for k in sorted(oracle.G) if k.startswith("W"))))
    np.testing.assert_allclose(eng.scalar(_lib.BATCH_LOSS), loss, rtol=5e-4)
    eng.close()


def test_raw_entries_equal_the_plain_ones_bit_for_bit(gpu):
    from tfkaldi_amd import _lib
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(6700)
    D, C = 4, 2
    eng, _ = make_pair(rng, max_frames=256, **dict(KW4, input_dim=D * (2 * C + 1)))
    _, _, _, _, refs, lex = _engine_case("float32")
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 25, 63)]
    lens = [u.shape[0] for u in utts]
    labels, lab = np.concatenate(refs).astype(np.int32), np.array([r.size for r in refs], np.int32)
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)
    spliced = np.concatenate([u.spliced() for u in utts])
    eng.ctc_set_den(lex)
    out = []
    for train in (True, False):
        for how in ("plain", "raw"):
            eng.eval_finish()
            if how == "plain":
                eng.accumulate_ctc_mmi(spliced, lens, labels, lab, lm_scale=0.5, ctc_weight=0.2, train=train)
            else:
                eng.accumulate_ctc_mmi_raw(raw, lens, C, labels, lab, lm_scale=0.5, ctc_weight=0.2, cmvn=cmvn_table(utts),
                                           train=train)
            out.append((eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES),
                        eng.debug_fetch(_lib.DBG_LOGITS, 0, sum(lens)).tobytes()))
        assert out[-1] == out[-2] and np.isfinite(out[-1][0]) and out[-1][1] == lab.sum()
    assert out[0][2] != out[2][2]  # (training left dLogits, evaluation the logits)
    eng.close()


def test_eval_variant_inside_an_open_step(gpu):
    """the loss on evaluation-mode logits; the engine's state untouched; inside a step the step finishes as if nothing had
    been evaluated"""
    eng, _, utt, X, refs, lex = _engine_case("float32", 6800)
    twin, _, _, _, _, _ = _engine_case("float32", 6800)
    lam, cw = 0.6, 0.3
    labels, lab = np.concatenate(refs).astype(np.int32), np.array([r.size for r in refs], np.int32)
    eng.ctc_set_den(lex)
    twin.ctc_set_den(lex)
    state0 = _engine_state(eng)
    eng.eval_accumulate_ctc_mmi(X, utt, labels, lab, lam, cw)
    z = eng.posteriors(X, raw_logits=True)
    loss, _ = _restated_batch(z, utt, refs, lex, lam, cw)
    got = eng.eval_finish() * lab.sum()
    print("ctc-mmi eval: loss %.6f, restated %.6f" % (got, loss))
    np.testing.assert_allclose(got, loss, rtol=2e-5)
    state1 = _engine_state(eng)
    assert sorted(state0) == sorted(state1) and all(state0[k] == state1[k] for k in state0)
    for e in (eng, twin):
        e.accumulate_ctc_mmi(X, utt, labels, lab, lam, cw)
        if e is eng:
            e.eval_accumulate_ctc_mmi(X[:utt[0]], utt[:1], refs[0], lab[:1], 1.0, 1.0)
            assert np.isfinite(e.eval_finish())
        e.accumulate_ctc_mmi(X, utt, labels, lab, lam, 0.0, last=True)
    assert eng.apply() == twin.apply()
    pa, pb = engine_params(eng), engine_params(twin)
    assert all(pa[k].tobytes() == pb[k].tobytes() for k in pa)
    eng.close()
    twin.close()


def test_update_mmi_descends(gpu, tmp_path):
    """30 steps of CTCTrainer.update_mmi against the isolated-word lexicon of the batch's transcriptions lower evaluate_mmi and
    do not raise the label errors of the beam search constrained by that lexicon"""
    from test_gpu_ctc_decode import _toy_ctc
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    texts = sorted({tuple(np.asarray(y).astype(np.int64).tolist()) for y in ys})
    lex = GraphLM.from_lexicon([np.array(t) for t in texts], coder.num_labels, separator=None, end_of_sequence=True)
    for _ in range(20):
        tr.update(xs, ys)
    before, err0 = tr.evaluate_mmi(xs, ys, lex), tr.label_errors(xs, ys, beam_width=8, lm=lex)
    losses = [tr.update_mmi(xs, ys, lex, lm_scale=1.0, ctc_weight=0.1) for _ in range(30)]
    after, err1 = tr.evaluate_mmi(xs, ys, lex), tr.label_errors(xs, ys, beam_width=8, lm=lex)
    print("ctc-mmi descent: evaluate_mmi %.5f -> %.5f, label errors %s -> %s, first / last step %.5f / %.5f"
          % (before, after, err0, err1, losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and after < before and after >= 0.0
    assert err1[0] <= err0[0] and err1[1] == err0[1]
    with pytest.raises(ValueError, match="utterance 0"):
        tr.update_mmi(xs, [np.asarray(ys[0])[:1]] + list(ys[1:]), lex)
    tr.close()
