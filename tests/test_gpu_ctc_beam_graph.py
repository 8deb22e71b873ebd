"""CTC prefix beam search constrained by a finite-state grammar on the device (tfk_ctc_graph_set /
tfk_ctc_beam_graph_logits and tfk_ctc_beam_lm / tfk_ctc_beam_topk with a graph set, csrc/ctc.hip) against the float64 numpy
restatement of tests/test_ctc_beam_graph_host.py applied to the SAME logits and the same graph, and bit for bit against the
n-gram and the acoustic search where the contract says they coincide.

Tolerance and hypothesis band are those of tests/test_gpu_ctc_beam_lm.py, applied to the COMBINED score: `tol` = 4 x the
largest |float32 run - float64 run| of the restatement's best score on the same inputs, floored at 1e-6 x |score|; the
device's best path must be one of the restatement's hypotheses within 2 tol of its best; that this band holds a single
hypothesis for at least 75 % of a test's utterances, and that every best restatement score is finite, is asserted on the
restatement alone, before the device is consulted.  Under `pytest -s` the `ctc-graph` lines are the per-case table
(recorded in profiles/ctc_graph_edges.txt)."""
from ctypes import c_float, c_void_p

import numpy as np
import pytest

from test_ctc_beam_graph_host import enumeration_graph, lexicon_inputs, prefix_beam_search_graph, single_word_inputs
from test_ctc_beam_host import ctc_log_prob, enumeration_cases, log_softmax, prefix_beam_search
from test_ctc_beam_lm_host import enumeration_lm
from test_ctc_decode_host import levenshtein
from test_gpu_ctc_beam import _device_beam_logits
from test_gpu_ctc_beam_lm import _device_beam_lm_logits, _random_lm, _zero_weight_cases
from test_gpu_ctc_beam_topk import _device_topk_logits
from test_gpu_ctc_decode import _toy_ctc

from tfkaldi_amd.neuralNetworks.ctc_lm import GraphLM, NgramLM

pytestmark = pytest.mark.gpu


def _device_graph_logits(z, utt, W, P, lm, K=0):
    """tfk_ctc_beam_graph_logits on host logits (K = label_topk, 0: the unpruned search): (hyps[u][n], scores [U, P],
    am_scores [U, P])"""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    T, O = z.shape
    assert O == lm.num_classes
    U = len(utt)
    seg = np.concatenate([[0], np.cumsum(utt)]).astype(np.int32)
    d_z, d_seg = torch.from_numpy(z).cuda(), torch.from_numpy(seg).cuda()
    d_w, d_n = torch.from_numpy(lm.table).cuda(), torch.from_numpy(lm.next).cuda()
    hyp = torch.full((P, max(T, 1)), -7, dtype=torch.int32, device="cuda")
    hyp_len = torch.full((P, U), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    am = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tfk_ctc_beam_graph_logits(
        c_void_p(stream), c_void_p(d_z.data_ptr()), O, O, T, c_void_p(d_seg.data_ptr()), U, W, P, K,
        c_void_p(d_w.data_ptr()), c_void_p(d_n.data_ptr()), lm.num_states, lm.start, c_float(lm.weight),
        c_float(lm.label_bonus), _lib.CTC_LM_EOS if lm.end_of_sequence else 0,
        c_void_p(hyp.data_ptr()), c_void_p(hyp_len.data_ptr()), c_void_p(score.data_ptr()), c_void_p(am.data_ptr())))
    torch.cuda.synchronize()
    hyp, hyp_len, score, am = hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy(), am.cpu().numpy()
    for n in range(P):  # the rows past a hypothesis are -1
        for u in range(U):
            assert np.all(hyp[n, seg[u] + hyp_len[n, u]:seg[u + 1]] == -1)
    hyps = [[hyp[n, seg[u]:seg[u] + hyp_len[n, u]].copy() for n in range(P)] for u in range(U)]
    return hyps, score.T.copy(), am.T.copy()


def _same(a, b):
    """hypotheses, scores and acoustic scores, bit for bit"""
    return (all(np.array_equal(p, q) for x, y in zip(a[0], b[0]) for p, q in zip(x, y))
            and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes())


def _restatement(z, utt, W, lm, P=8, K=None):
    """float64 N-best of the restatement and the per-utterance tol from its own float32 run"""
    P = min(P, W)
    h64, s64, a64 = prefix_beam_search_graph(z, utt, W, P, lm, label_topk=K)
    _, s32, _ = prefix_beam_search_graph(z, utt, W, 1, lm, dtype=np.float32, label_topk=K)
    assert np.all(np.isfinite(s64[:, 0])) and np.all(np.isfinite(s32[:, 0])), "a best restatement score is not finite"
    tol = np.maximum(4.0 * np.abs(s32[:, 0] - s64[:, 0]).max(), 1e-6 * np.abs(s64[:, 0]))
    band = [[n for n in range(s64.shape[1]) if s64[u, n] >= s64[u, 0] - 2 * tol[u]] for u in range(len(utt))]
    crowded = sum(len(b) > 1 for b in band)
    assert 4 * crowded <= len(utt), "%d of %d utterances have rivals within 2 tol of the best" % (crowded, len(utt))
    return h64, s64, a64, tol, band


def _check_best(name, z, utt, lm, rest, hyps, scores, am):
    """every utterance's best path: combined score within tol of the restatement's, the hypothesis inside its 2-tol band and
    accepted by the graph, score - am_score = the graph's value of the labels, am_score no more than the labels' exact
    log-probability; every listed path with a finite score is accepted"""
    h64, s64, a64, tol, band = rest
    seg = np.concatenate([[0], np.cumsum(utt)])
    worst = 0.0
    for u in range(len(utt)):
        got, sc, ac = hyps[u][0], float(scores[u, 0]), float(am[u, 0])
        err = abs(sc - s64[u, 0])
        assert err <= tol[u], (name, u, sc, s64[u, 0], tol[u])
        assert any(np.array_equal(got, h64[u][n]) for n in band[u]), (name, u, got, h64[u][0])
        for h, s in zip(hyps[u], scores[u]):
            assert not np.isnan(s) and (s == -np.inf or lm.accepts(h)), (name, u, h, s)
        ulps = 0.5 * (np.spacing(np.float32(abs(sc))) + np.spacing(np.float32(abs(ac))))
        assert abs((sc - ac) - lm.score(got)) <= tol[u] + ulps, (name, u, sc, ac, lm.score(got))
        assert ac <= ctc_log_prob(z[seg[u]:seg[u + 1]], got) + tol[u], (name, u, ac)
        worst = max(worst, err)
    print("ctc-graph %-32s U %2d T %4d O %2d S %4d | worst |device - float64| %.2e smallest tol %.2e largest band %d"
          % (name, len(utt), sum(utt), z.shape[1], lm.num_states, worst, tol.min(), max(len(b) for b in band)))


# ---- 1. identity (a): a graph whose states are an n-gram's contexts is the n-gram search, bit for bit ----
def _ngram_cases():
    cases = enumeration_cases()
    for order in (2, 3):
        yield "enumeration order %d" % order, np.concatenate(cases).astype(np.float32), [6] * len(cases), 128, order, None
    z = (2.0 * np.random.default_rng(90).standard_normal((4 * 40, 9))).astype(np.float32)
    yield "O9 W10 order2", z, [40] * 4, 10, 2, 4
    yield "O9 W100 order3", z, [40] * 4, 100, 3, 4
    # nb * O = 128 * 64 candidates: the key table is full
    yield "O64 W128 order2", (2.0 * np.random.default_rng(64).standard_normal((4 * 30, 64))).astype(np.float32), [30] * 4, 128, 2, 63


@pytest.mark.parametrize("eos", [False, True])
def test_graph_of_an_ngram_equals_the_ngram_search_bit_for_bit(gpu, eos):
    for name, z, utt, W, order, K in _ngram_cases():
        O = z.shape[1]
        lm = enumeration_lm(order, eos) if O == 3 else _random_lm(np.random.default_rng(91), O, order, eos=eos)
        graph = GraphLM.from_ngram(lm)
        P = min(3, W)
        want = _device_beam_lm_logits(z, utt, W, P, lm)
        got = _device_graph_logits(z, utt, W, P, graph)
        assert _same(got, want), name
        assert sum(h[0].size for h in got[0]) > 0
        ks = [O - 1] if K is None else [K, O - 1] if K < O - 1 else [K]
        for k in ks:  # the pruned search with the table against the pruned search with the graph
            assert _same(_device_graph_logits(z, utt, W, P, graph, K=k), _device_topk_logits(z, utt, W, P, k, lm)), (name, k)
        print("ctc-graph identity (a) %-22s eos %d W %3d label_topk %s: bit-identical to the n-gram search"
              % (name, eos, W, ks))


# ---- 2. identity (b): one state, every arc, weight 0 is the acoustic search, bit for bit ----
def test_one_state_zero_weight_graph_equals_the_acoustic_search_bit_for_bit(gpu):
    for name, z, utt, W, _ in _zero_weight_cases():
        O = z.shape[1]
        graph = GraphLM(np.zeros((1, O)), np.zeros((1, O), dtype=np.int64), weight=0.0, label_bonus=0.0)
        P = min(3, W)
        want_h, want_s = _device_beam_logits(z, utt, W, P)
        hyps, scores, am = _device_graph_logits(z, utt, W, P, graph)
        assert all(np.array_equal(a, b) for x, y in zip(hyps, want_h) for a, b in zip(x, y)), name
        assert scores.tobytes() == want_s.tobytes() and am.tobytes() == scores.tobytes(), name
        assert sum(h[0].size for h in hyps) > 0
        print("ctc-graph identity (b) %-22s W %3d: bit-identical to the acoustic search" % (name, W))


# ---- 3. the enumeration cases under the constraint ----
@pytest.mark.parametrize("eos", [False, True])
def test_enumeration_cases_under_the_constraint(gpu, eos):
    lm = enumeration_graph(eos)
    cases = enumeration_cases()
    z = np.concatenate(cases).astype(np.float32)
    utt = [6] * len(cases)
    P = 8
    h64, s64, a64, tol, band = _restatement(z, utt, 128, lm, P)
    hyps, scores, am = _device_graph_logits(z, utt, 128, P, lm)
    worst = 0.0
    for u in range(len(utt)):
        assert np.array_equal(hyps[u][0], h64[u][0]), (u, hyps[u][0], h64[u][0])
        clear = [n for n in range(P) if (n == 0 or s64[u, n - 1] - s64[u, n] > 2 * tol[u])
                 and (n == P - 1 or s64[u, n] - s64[u, n + 1] > 2 * tol[u])]
        assert 0 in clear and len(clear) >= 4
        for n in clear:
            assert np.array_equal(hyps[u][n], h64[u][n]), (u, n)
            assert lm.accepts(hyps[u][n])
            tol_n = max(tol[u], 1e-6 * abs(s64[u, n]))
            assert abs(scores[u, n] - s64[u, n]) <= tol_n, (u, n, scores[u, n], s64[u, n], tol_n)
            assert abs(am[u, n] - a64[u, n]) <= max(tol[u], 1e-6 * abs(a64[u, n])), (u, n, am[u, n], a64[u, n])
            worst = max(worst, abs(scores[u, n] - s64[u, n]))
    print("ctc-graph %-32s U %2d T %4d O %2d S %4d | worst |device - float64| %.2e smallest tol %.2e largest band %d"
          % ("enumeration eos %d" % eos, len(utt), sum(utt), 3, lm.num_states, worst, tol.min(), max(len(b) for b in band)))


# ---- 4. a lexicon ----
@pytest.mark.parametrize("K", [None, 8])
def test_lexicon_search_equals_restatement(gpu, K):
    z, utt, refs, lm = lexicon_inputs()
    W = 32
    rest = _restatement(z, utt, W, lm, K=K)
    h64 = rest[0]
    assert all(lm.accepts(h[0]) for h in h64)
    plain = prefix_beam_search(z, utt, W, 1)[0]
    assert not any(np.array_equal(p[0], h[0]) for p, h in zip(plain, h64))  # the constraint changes every best path
    errs_plain = sum(levenshtein(p[0], r) for p, r in zip(plain, refs))
    errs_rest = sum(levenshtein(h[0], r) for h, r in zip(h64, refs))
    assert errs_rest < errs_plain, (errs_rest, errs_plain)
    hyps, scores, am = _device_graph_logits(z, utt, W, 3, lm, K=K or 0)
    name = "lexicon W=32" + ("" if K is None else " label_topk %d" % K)
    _check_best(name, z, utt, lm, rest, hyps, scores, am)
    assert np.all(scores[:, :-1] >= scores[:, 1:])  # best first, by the combined score
    errs = sum(levenshtein(h[0], r) for h, r in zip(hyps, refs))
    dev_plain = sum(levenshtein(h[0], r) for h, r in zip(_device_beam_logits(z, utt, W, 1)[0], refs))
    found = sum(np.array_equal(h[0], r) for h, r in zip(hyps, refs))
    print("ctc-graph %s: label errors %d with the lexicon, %d by acoustic score (of %d labels); %d of %d references found"
          % (name, errs, dev_plain, sum(r.size for r in refs), found, len(refs)))
    assert errs < dev_plain


# ---- 5. fewer live candidates than the beam ----
@pytest.mark.parametrize("W", [8, 128])
def test_fewer_live_candidates_than_the_beam(gpu, W):
    z, utt, word = single_word_inputs()
    lm = GraphLM.from_lexicon([word], 6, separator=5, weight=0.5, label_bonus=0.3)
    live = []
    prefix_beam_search_graph(z, utt, W, 1, lm, live=live)
    assert min(min(c) for c in live) <= 2 and all(min(c) < W for c in live)
    rest = _restatement(z, utt, W, lm)
    P = min(4, W)
    first = _device_graph_logits(z, utt, W, P, lm)
    _check_best("single word W=%d" % W, z, utt, lm, rest, *first)
    assert _same(first, _device_graph_logits(z, utt, W, P, lm))  # the call returns, and twice with the same bytes
    assert _same(first, _device_graph_logits(z, utt, W, P, lm, K=6))  # keeping every label is the unpruned search


# ---- 6. endings in a non-final state, weight 0, zero frames ----
@pytest.mark.parametrize("weight", [0.5, 0.0])
def test_non_final_endings_and_zero_weight(gpu, weight):
    z, _, word = single_word_inputs()
    utt = [6, 0, 6, 6]
    z = z[:sum(utt)]
    for start_final in (False, True):
        lm = GraphLM.from_lexicon([word], 6, separator=5, weight=weight, label_bonus=0.3, end_of_sequence=True)
        if start_final:
            table = lm.table.copy()
            table[0, -1] = -0.75
            lm = GraphLM(table, np.where(np.isneginf(table), -1, lm.next), weight=weight, label_bonus=0.3, end_of_sequence=True)
        P = 4
        h64, s64, a64 = prefix_beam_search_graph(z, utt, 8, P, lm)
        hyps, scores, am = _device_graph_logits(z, utt, 8, P, lm)
        assert not np.any(np.isnan(scores)) and not np.any(np.isnan(am))
        for u in (0, 2, 3):  # 6 frames cannot spell 12 labels: only the empty prefix can be final
            listed = np.isfinite(a64[u])
            assert listed.sum() >= 2 and np.array_equal(np.isfinite(am[u]), listed)
            assert [h.size for h in hyps[u]] == [h.size for h in h64[u]]
            assert np.array_equal(scores[u] == -np.inf, s64[u] == -np.inf)
            assert np.all(scores[u, 1:] == -np.inf) and (scores[u, 0] > -np.inf) == start_final
            for h, a in zip(hyps[u], am[u]):
                assert a == -np.inf or lm.state(h) is not None  # still constrained, also at weight 0
        end = np.float32(weight) * np.float32(-0.75) if start_final else -np.inf  # zero frames: the start state's end weight
        assert hyps[1][0].size == 0 and scores[1].tolist() == [float(end)] + [-np.inf] * (P - 1)
        assert am[1].tolist() == [0.0] + [-np.inf] * (P - 1)
        print("ctc-graph non-final endings weight %.1f start final %d: %d listed paths with score -inf, none NaN"
              % (weight, start_final, int((np.isfinite(am) & (scores == -np.inf)).sum())))


# ---- 7. the engine's entries and the Python layers ----
def test_engine_decoder_and_trainer_with_a_graph(gpu, tmp_path):
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    from tfkaldi_amd.processing.feature_reader import Unspliced
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    for _ in range(60):
        tr.update(xs, ys)
    eng, O = tr.engine, coder.num_labels + 1
    # the grammar: the batch's transcriptions as an isolated-word lexicon; without the end flag every prefix of one is a path
    texts = sorted({tuple(np.asarray(y).astype(np.int64).tolist()) for y in ys})
    lm = GraphLM.from_lexicon([np.array(t) for t in texts], coder.num_labels, separator=None, weight=0.5, label_bonus=1.0)
    ngram = NgramLM.from_label_sequences(ys, coder.num_labels, 2, weight=0.5, label_bonus=1.0)
    flat = np.ascontiguousarray(np.concatenate([x.spliced() if isinstance(x, Unspliced) else np.asarray(x) for x in xs]),
                                dtype=np.float32)
    lens = [len(x) for x in xs]
    good = eng.ctc_beam_lm(flat, lens, lm, beam_width=10, top_paths=2)
    assert all(lm.accepts(h) for hs in good[0] for h in hs) and sum(h[0].size for h in good[0]) > 0
    with_ngram = eng.ctc_beam_lm(flat, lens, ngram, beam_width=10, top_paths=2)  # tfk_ctc_lm_set replaces the graph
    assert not _same(good, with_ngram)
    assert _same(good, eng.ctc_beam_lm(flat, lens, lm, beam_width=10, top_paths=2))  # and the graph the table
    pruned = eng.ctc_beam_lm(flat, lens, lm, beam_width=10, top_paths=2, label_topk=O - 1)  # tfk_ctc_beam_topk, every label
    assert _same(good, pruned)

    # tfk_ctc_graph_set's rejections: each leaves the model in force
    ptr = lambda x: x.ctypes.data_as(c_void_p)
    table, nxt, S = lm.table, lm.next, lm.num_states
    arc = int(np.flatnonzero(np.isfinite(table[:, :O - 1]).reshape(-1))[3])  # an arc, as an index into [S, O - 1]
    arc = (arc // (O - 1)) * O + arc % (O - 1)
    hole = int(np.flatnonzero(np.isneginf(table).reshape(-1))[5])
    def rejected(word, t=table, n=nxt, states=S, start=0):
        rc = eng.lib.tfk_ctc_graph_set(eng._h, ptr(t) if t is not None else c_void_p(None), ptr(n) if n is not None else
                                       c_void_p(None), states, start)
        assert rc != 0 and word in eng.lib.tfk_last_error(), (word, rc, eng.lib.tfk_last_error())
        assert _same(good, eng.ctc_beam_lm(flat, lens, lm, beam_width=10, top_paths=2)), word
    for bad, where in ((np.nan, arc), (np.inf, arc), (np.nan, hole), (np.inf, hole)):
        t = table.copy()
        t.reshape(-1)[where] = bad
        rejected(b"entry %d of weight" % where, t=t)
    for bad in (-1, S):
        n = nxt.copy()
        n.reshape(-1)[arc] = bad
        rejected(b"entry %d of next" % arc, n=n)
    n = nxt.copy()
    n.reshape(-1)[hole] = -5  # (where there is no arc next is not read)
    assert eng.lib.tfk_ctc_graph_set(eng._h, ptr(table), ptr(n), S, 0) == 0
    assert _same(good, eng.ctc_beam_lm(flat, lens, lm, beam_width=10, top_paths=2))
    rejected(b"start", start=S)
    rejected(b"start", start=-1)
    rejected(b"num_states", states=0)
    rejected(b"33554432", states=(1 << 25) // O + 1)  # the limit is in the message; nothing is read
    rejected(b"next is NULL", n=None)
    # weight == NULL drops the graph, tfk_ctc_lm_set(NULL) as well: the model entries then refuse
    h, hl = np.empty((1, flat.shape[0]), np.int32), np.empty((1, len(lens)), np.int32)
    s, a, ulen = np.empty((1, len(lens)), np.float32), np.empty((1, len(lens)), np.float32), np.array(lens, np.int32)
    null = c_void_p(None)
    call = lambda: eng.lib.tfk_ctc_beam_lm(eng._h, ptr(flat), flat.shape[1], flat.shape[0], ptr(ulen), len(lens), 4, 1,
                                           c_float(0.5), c_float(1.0), null, null, ptr(h), ptr(hl), ptr(s), ptr(a), null, 0)
    assert call() == 0
    assert eng.lib.tfk_ctc_graph_set(eng._h, null, null, 0, 0) == 0
    assert call() != 0 and b"no language model" in eng.lib.tfk_last_error()
    eng._lm_table = None  # (the model was dropped behind the binding's back: its record of the upload goes too)
    assert _same(good, eng.ctc_beam_lm(flat, lens, lm, beam_width=10, top_paths=2))
    eng.ctc_set_lm(None)
    assert call() != 0 and b"no language model" in eng.lib.tfk_last_error()

    # Trainer.label_errors against the restatement on the engine's logits
    z = eng.posteriors(flat, raw_logits=True)
    h64, s64, _, tol, band = _restatement(z, lens, 10, lm)
    refs = [np.asarray(y).astype(np.int64) for y in ys]
    want = sum(levenshtein(h[0], r) for h, r in zip(h64, refs))
    got = tr.label_errors(xs, ys, beam_width=10, lm=lm)
    plain = tr.label_errors(xs, ys, beam_width=10)
    print("ctc-graph toy model after 60 updates: label errors beam %d, beam + grammar %d of %d" % (plain[0], got[0], got[1]))
    assert got == (want, sum(r.size for r in refs))

    # Decoder: spliced and unspliced utterances agree; the rescoring pass takes the graph
    tr.save_model(str(tmp_path / "model"))
    dec = Decoder(dnn, F, maxlen)
    dec.restore(str(tmp_path / "model"))
    got_h, got_s, got_am = dec.ctc_beam_search_lm(xs, lm, beam_width=10, top_paths=2)
    assert _same((got_h, got_s, got_am), good)
    rng = np.random.default_rng(5)
    D, C = F // 5, 2
    raw = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                     np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 5, 63)]
    a = dec.ctc_beam_search_lm(raw, lm, beam_width=10, top_paths=3)
    b = dec.ctc_beam_search_lm([u.spliced() for u in raw], lm, beam_width=10, top_paths=3)
    assert _same(a, b) and all(lm.accepts(h) for hs in a[0] for h in hs)
    hyps, scores, am, rank, post = dec.ctc_rescore(xs, beam_width=10, top_paths=4, lm=lm)
    for hs, sc, ac in zip(hyps, scores, am):
        assert len(hs) >= 1 and np.all(sc[:-1] >= sc[1:])
        assert np.abs(sc - (ac.astype(np.float64) + np.array([lm.score(h) for h in hs]))).max() <= 1e-9
    assert dec.ctc_beam_search_lm([], lm)[0] == []
    dec.close()

    loss = tr.update_mwer(xs, ys, beam_width=4, lm=lm)
    assert np.isfinite(loss)
    tr.close()
