"""CTC prefix beam search with per-frame label pruning on the device (tfk_ctc_beam_topk / _raw / _logits, csrc/ctc.hip:
ctc_row_topk_kernel + ctc_beam_topk_kernel) against (a) the existing logits entries, bit for bit, where label_topk prunes
nothing, and (b) the float64 numpy restatement of tests/test_ctc_beam_topk_host.py on the SAME logits (and table).

Tolerance and hypothesis band are those of tests/test_gpu_ctc_beam.py: `tol` = 4 x the largest |float32 run - float64 run| of
the restatement's best score on the same inputs, floored at 1e-6 x |score|; the device's best path must be one of the
restatement's hypotheses within 2 tol of its best; that this band holds a single hypothesis for at least 75 % of a test's
utterances is asserted on the restatement alone, before the device is consulted."""
import os
import socket
import sys
from ctypes import c_float, c_void_p

import numpy as np
import pytest

from test_ctc_beam_host import ctc_log_prob, enumeration_cases, log_softmax, peaky_logits, prefix_beam_search
from test_ctc_beam_lm_host import enumeration_lm
from test_ctc_beam_topk_host import known_answer_rows, prefix_beam_search_topk, wide_logits
from test_ctc_decode_host import levenshtein
from test_gpu_ctc_beam import KW, _device_beam_logits, _dp_data, _sharpen
from test_gpu_ctc_beam_lm import _device_beam_lm_logits, _random_lm
from test_gpu_ctc_decode import _refs, _split, _toy_ctc
from util import engine_grads, engine_params, make_pair

from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_topk_logits(z, utt, W, P, K, lm=None, ld=None, check=True):
    """tfk_ctc_beam_topk_logits on host logits (rows padded to ld with a poison value): (hyps[u][n], scores [U, P],
    am_scores [U, P]); check False: (return code, message) instead"""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    T, O = z.shape
    ld = O if ld is None else ld
    if ld > O:  # what lies between O and ld must never be read: it would win every max
        z = np.concatenate([z, np.full((T, ld - O), 1e30, np.float32)], axis=1)
    U = len(utt)
    seg = np.concatenate([[0], np.cumsum(utt)]).astype(np.int32)
    d_z, d_seg = torch.from_numpy(z).cuda(), torch.from_numpy(seg).cuda()
    d_lm = torch.from_numpy(lm.table).cuda() if lm is not None else None
    hyp = torch.full((P, max(T, 1)), -7, dtype=torch.int32, device="cuda")
    hyp_len = torch.full((P, U), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    am = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.tfk_ctc_beam_topk_logits(
        c_void_p(stream), c_void_p(d_z.data_ptr()), ld, O, T, c_void_p(d_seg.data_ptr()), U, W, P, K,
        c_void_p(d_lm.data_ptr() if lm is not None else None), lm.order if lm is not None else 0,
        c_float(lm.weight if lm is not None else 0.0), c_float(lm.label_bonus if lm is not None else 0.0),
        _lib.CTC_LM_EOS if lm is not None and lm.end_of_sequence else 0,
        c_void_p(hyp.data_ptr()), c_void_p(hyp_len.data_ptr()), c_void_p(score.data_ptr()), c_void_p(am.data_ptr()))
    if not check:
        return rc, lib.tfk_last_error()
    _lib.check(rc)
    torch.cuda.synchronize()
    hyp, hyp_len, score, am = hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy(), am.cpu().numpy()
    for n in range(P):  # the rows past a hypothesis are -1
        for u in range(U):
            assert np.all(hyp[n, seg[u] + hyp_len[n, u]:seg[u + 1]] == -1)
    hyps = [[hyp[n, seg[u]:seg[u] + hyp_len[n, u]].copy() for n in range(P)] for u in range(U)]
    return hyps, score.T.copy(), am.T.copy()


def _same_hyps(a, b):
    return all(np.array_equal(p, q) for x, y in zip(a, b) for p, q in zip(x, y))


_RESTATED = {}


def _restatement(key, z, utt, W, K, lm, P=4):
    """float64 N-best of the restatement and the per-utterance tol from its own float32 run (computed once per key)"""
    if key not in _RESTATED:
        P = min(P, W)
        h64, s64, a64 = prefix_beam_search_topk(z, utt, W, P, K, lm)
        _, s32, _ = prefix_beam_search_topk(z, utt, W, 1, K, lm, dtype=np.float32)
        tol = np.maximum(4.0 * np.abs(s32[:, 0] - s64[:, 0]).max(), 1e-6 * np.abs(s64[:, 0]))
        _RESTATED[key] = (h64, s64, a64, tol)
    return _RESTATED[key]


def _check_best(name, z, utt, W, K, lm, hyps, scores, am, crowded_ok=True):
    """every utterance's best path: score within tol of the restatement's, the hypothesis inside its 2-tol band; the acoustic
    part no more than the labels' exact log-probability; with a model score - am_score = the model's value of the labels,
    without one am_score == score"""
    h64, s64, a64, tol = _restatement(name, z, utt, W, K, lm)
    U = len(utt)
    band = [[n for n in range(s64.shape[1]) if s64[u, n] >= s64[u, 0] - 2 * tol[u]] for u in range(U)]
    crowded = sum(len(b) > 1 for b in band)
    if crowded_ok:
        assert 4 * crowded <= U, "%s: %d of %d utterances have rivals within 2 tol of the best" % (name, crowded, U)
    seg = np.concatenate([[0], np.cumsum(utt)])
    worst = 0.0
    for u in range(U):
        got, sc, ac = hyps[u][0], float(scores[u, 0]), float(am[u, 0])
        err = abs(sc - s64[u, 0])
        print("%s utt %d: T %d labels %d device %.6f float64 %.6f am %.6f |diff| %.2e tol %.2e band %d"
              % (name, u, utt[u], got.size, sc, s64[u, 0], ac, err, tol[u], len(band[u])))
        assert err <= tol[u], (name, u, sc, s64[u, 0], tol[u])
        assert any(np.array_equal(got, h64[u][n]) for n in band[u]), (name, u, got, h64[u][0])
        if lm is None:
            assert ac == sc
        else:
            ulps = 0.5 * (np.spacing(np.float32(abs(sc))) + np.spacing(np.float32(abs(ac))))
            assert abs((sc - ac) - lm.score(got)) <= tol[u] + ulps, (name, u, sc, ac, lm.score(got))
        assert ac <= ctc_log_prob(z[seg[u]:seg[u + 1]], got) + tol[u], (name, u, ac)  # a lower bound
        worst = max(worst, err)
    print("%s: largest |device - float64| %.3e, smallest tol %.3e" % (name, worst, tol.min()))
    return h64


# ---- 1. where label_topk prunes nothing the results are the existing kernel's, bit for bit ----
def _link_inputs(O):
    if O == 3:
        cases = enumeration_cases()
        return np.concatenate(cases).astype(np.float32), [6] * len(cases)
    rng = np.random.default_rng(300 + O)
    utt = [0, 1, 37, 0, 22, 1, 30, 0]  # zero- and one-frame utterances at the start, in the middle and at the end
    if O == 64:
        return (2.0 * rng.standard_normal((sum(utt), O))).astype(np.float32), utt
    return peaky_logits(rng, sum(utt), O, 12), utt


@pytest.mark.parametrize("O", [3, 9, 36, 64])
def test_unpruned_results_equal_the_existing_entries_bit_for_bit(gpu, O):
    z, utt = _link_inputs(O)
    rng = np.random.default_rng(O)
    lms = [None] + [_random_lm(rng, O, order, eos=eos) for order, eos in ((1, False), (2, True), (3, False), (3, True))]
    labels = 0
    for W in (1, 16, 128):  # (W = 128 with O = 64 fills the 8192-key table)
        P = min(3, W)
        for lm in lms:
            if lm is None:
                want_h, want_s = _device_beam_logits(z, utt, W, P)
                want_a = want_s
            else:
                want_h, want_s, want_a = _device_beam_lm_logits(z, utt, W, P, lm)
            for K in (O - 1, 63):
                hyps, scores, am = _device_topk_logits(z, utt, W, P, K, lm)
                what = (O, W, K, None if lm is None else (lm.order, lm.end_of_sequence))
                assert _same_hyps(hyps, want_h), what
                assert scores.tobytes() == want_s.tobytes() and am.tobytes() == want_a.tobytes(), what
            labels += sum(h[0].size for h in want_h)
    assert labels > 0
    # ld > O: the padding is never read
    hyps, scores, am = _device_topk_logits(z, utt, 16, 3, 63, lms[2], ld=O + 5)
    want_h, want_s, want_a = _device_beam_lm_logits(z, utt, 16, 3, lms[2])
    assert _same_hyps(hyps, want_h) and scores.tobytes() == want_s.tobytes() and am.tobytes() == want_a.tobytes()


# ---- 2. the enumeration cases, pruned to one label per frame ----
@pytest.mark.parametrize("with_lm", [False, True])
def test_enumeration_cases_at_one_label_per_frame(gpu, with_lm):
    lm = enumeration_lm(2, True) if with_lm else None
    cases = enumeration_cases()
    z = np.concatenate(cases).astype(np.float32)
    utt = [6] * len(cases)
    P = 8
    hyps, scores, am = _device_topk_logits(z, utt, 128, P, 1, lm)
    h64, s64, a64, tol = _restatement(("enumeration", with_lm), z, utt, 128, 1, lm, P)
    worst, compared = 0.0, 0
    for u in range(len(utt)):
        assert np.array_equal(hyps[u][0], h64[u][0]), (u, hyps[u][0], h64[u][0])
        live = [n for n in range(P) if np.isfinite(s64[u, n])]
        clear = [n for n in live if (n == 0 or s64[u, n - 1] - s64[u, n] > 2 * tol[u])
                 and (n == P - 1 or s64[u, n] - s64[u, n + 1] > 2 * tol[u])]
        assert 0 in clear
        for n in clear:
            assert np.array_equal(hyps[u][n], h64[u][n]), (u, n)
            assert abs(scores[u, n] - s64[u, n]) <= max(tol[u], 1e-6 * abs(s64[u, n])), (u, n, scores[u, n], s64[u, n])
            assert abs(am[u, n] - a64[u, n]) <= max(tol[u], 1e-6 * abs(a64[u, n])), (u, n, am[u, n], a64[u, n])
            worst = max(worst, abs(scores[u, n] - s64[u, n]))
        compared += len(clear)
        for n in range(P):  # what the pruning left no alignment for has probability zero (a prefix of the beam, or padding)
            if not np.isfinite(s64[u, n]):
                assert scores[u, n] == -np.inf and am[u, n] == -np.inf
    assert compared >= 3 * len(utt)
    print("enumeration cases K = 1 model %d: %d entries compared, largest |device - float64| %.3e, smallest tol %.3e"
          % (with_lm, compared, worst, tol.min()))


# ---- 3. restatement parity on wide alphabets ----
#        name: (O, K, W, model order or None)
PARITY = {
    "O65 K63 W16 order2": (65, 63, 16, 2),
    "O128 K16 W32": (128, 16, 32, None),
    "O129 K16 W32": (129, 16, 32, None),
    "O200 K16 W32 order2": (200, 16, 32, 2),
    "O200 K63 W128 order1": (200, 63, 128, 1),  # 128 * 64 candidates: the full key table
    "O1000 K8 W16": (1000, 8, 16, None),
    "O1000 K8 W16 order2": (1000, 8, 16, 2),
    "O4000 K4 W8": (4000, 4, 8, None),
    "O65 K8 W16 order3": (65, 8, 16, 3),
    "O65 K8 W16 order4": (65, 8, 16, 4),
}


def _parity_lm(O, order):
    if order is None:
        return None
    rng = np.random.default_rng(1000 * order + O)
    table = 1.5 * rng.standard_normal((O ** (order - 1), O), dtype=np.float32)
    table -= np.log(np.exp(table).sum(axis=1, keepdims=True))
    return NgramLM(table, order, weight=0.6, label_bonus=0.4, end_of_sequence=order == 2)


@pytest.mark.parametrize("name", sorted(PARITY))
def test_standalone_entry_equals_restatement(gpu, name):
    O, K, W, order = PARITY[name]
    z, utt = wide_logits(O, Tn=40 if W == 128 else 60)
    lm = _parity_lm(O, order)
    hyps, scores, am = _device_topk_logits(z, utt, W, 3, K, lm, ld=O + 3)
    h64 = _check_best(name, z, utt, W, K, lm, hyps, scores, am)
    assert np.all(scores[:, :-1] >= scores[:, 1:])  # best first
    assert sum(h[0].size for h in hyps) > 20
    if name == "O1000 K8 W16":  # K is honoured: the unpruned search decides otherwise for some utterance
        plain = prefix_beam_search(z, utt, W, 1)[0]
        assert any(not np.array_equal(plain[u][0], h64[u][0]) for u in range(len(utt)))


def test_the_widest_alphabet(gpu):
    """O = 65536, the limit: 30 frames in all"""
    O, K, W = 65536, 8, 8
    utt = [14, 0, 1, 15]
    z = peaky_logits(np.random.default_rng(65536), sum(utt), O, 8, scale=10.0)
    z[3, 65534] = z[3].max() + 4.0  # the last label, and a label beyond 2^15, must be reachable
    z[20, 40000] = z[20].max() + 4.0
    hyps, scores, am = _device_topk_logits(z, utt, W, 2, K, ld=O + 1)
    h64 = _check_best("O65536 K8 W8", z, utt, W, K, None, hyps, scores, am)
    assert 65534 in h64[0][0] and 40000 in h64[3][0]
    assert hyps[1][0].size == 0 and scores[1].tolist() == [0.0, -np.inf]


@pytest.mark.parametrize("O", [65, 128, 129, 200, 1000, 4000])
def test_edge_shapes(gpu, O):
    """zero- and one-frame utterances at the start, in the middle and at the end; W = 1; K = 1; more paths than survivors;
    on peaky logits and on dense ones (unit Gaussian: many labels are close, so at K = 1 and 2 most prefixes have children
    whose label is not kept at the next frame)"""
    rng = np.random.default_rng(O + 17)
    utt = [0, 1, 23, 0, 1, 31, 1, 0]
    z = peaky_logits(rng, sum(utt), O, 10)
    dense = rng.standard_normal((sum(utt), O)).astype(np.float32)
    lm = _parity_lm(O, 2) if O <= 1000 else None  # (the parity table has no model at O = 4000: 64 MB of table)
    for what, W, K, model in (("peaky", 1, 8, None), ("peaky", 8, 1, None), ("peaky", 1, 1, lm), ("peaky", 16, 8, lm),
                              ("dense", 8, 1, None), ("dense", 5, 2, lm), ("dense", 1, 1, None)):
        P = min(3, W)
        zz = z if what == "peaky" else dense
        hyps, scores, am = _device_topk_logits(zz, utt, W, P, K, model, ld=O + 7)
        _check_best("edges %s O=%d W=%d K=%d model %d" % (what, O, W, K, model is not None), zz, utt, W, K, model, hyps,
                    scores, am, crowded_ok=W > 1)
        for u in (0, 3, 7):  # zero frames: the empty hypothesis, acoustic 0, combined 0 or the end term of the start context
            end = float(np.float32(model.weight) * model.table[-1, -1]) if model is not None else 0.0
            assert all(h.size == 0 for h in hyps[u])
            assert am[u].tolist() == [0.0] + [-np.inf] * (P - 1) and scores[u].tolist() == [end] + [-np.inf] * (P - 1)
    # one frame, K = 1, W = 8, 4 paths: only () and (the kept label) exist -- the other paths are padding
    hyps, scores, am = _device_topk_logits(z[:1], [1], 8, 4, 1)
    assert np.isfinite(scores[0, :2]).all() and scores[0, 2:].tolist() == [-np.inf, -np.inf]
    assert sorted(h.size for h in hyps[0]) == [0, 0, 0, 1] and all(h.size == 0 for h in hyps[0][2:])
    empty = _device_topk_logits(np.zeros((0, O), np.float32), [0, 0], 4, 1, 5)
    assert all(h[0].size == 0 for h in empty[0]) and empty[1].tolist() == [[0.0], [0.0]]


# ---- 3b. dense logits, one or two labels per frame, beams of 3 to 11 ----
# Here the beam is cut while it is still filling: nb * (K + 1) is near W, and most children's labels are NOT kept at the next
# frame, so they kill no candidate of their parent's.  The cut must then be decided by the live candidates alone -- counting
# every child as a dead candidate would skip it and keep the first W candidates in index order instead of the W best.
DENSE_W = list(range(3, 12))
DENSE_O = (4, 7, 11)
_DENSE = {}


def _dense_inputs(W, O):
    """12 utterances of 4 to 11 frames of unit Gaussian logits (computed once per shape)"""
    if (W, O) not in _DENSE:
        rng = np.random.default_rng(9000 + 16 * W + O)
        utt = rng.integers(4, 12, size=12).tolist()
        _DENSE[(W, O)] = (rng.standard_normal((sum(utt), O)).astype(np.float32), utt)
    return _DENSE[(W, O)]


@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("K", [1, 2])
def test_dense_logits_small_beams_equal_restatement(gpu, K, with_lm):
    """the N-best list against the restatement, as the enumeration test compares it: every entry that is more than 2 tol
    away from its neighbours has the restatement's labels and score.  An utterance counts only if the restatement's float32
    run gives the float64 run's N-best labels (else rounding, not the search, decides there); that this holds for at least
    75 % of the utterances is asserted on the restatement alone"""
    restated = []
    for W in DENSE_W:
        for O in DENSE_O:
            z, utt = _dense_inputs(W, O)
            lm = _random_lm(np.random.default_rng(O), O, 2, eos=True) if with_lm else None
            P = min(W, 4)
            h64, s64, a64 = prefix_beam_search_topk(z, utt, W, P, K, lm)
            h32, s32, _ = prefix_beam_search_topk(z, utt, W, P, K, lm, dtype=np.float32)
            tol = np.maximum(4.0 * np.abs(s32[:, 0] - s64[:, 0]).max(), 1e-6 * np.abs(s64[:, 0]))
            steady = [u for u in range(len(utt)) if all(np.array_equal(a, b) for a, b in zip(h32[u], h64[u]))]
            restated.append((W, O, z, utt, lm, P, h64, s64, a64, tol, steady))
    counted, total = sum(len(r[-1]) for r in restated), sum(len(r[3]) for r in restated)
    assert 4 * counted >= 3 * total, (counted, total)
    compared, worst = 0, 0.0
    for W, O, z, utt, lm, P, h64, s64, a64, tol, steady in restated:
        hyps, scores, am = _device_topk_logits(z, utt, W, P, K, lm, ld=O + 1)
        for u in steady:
            live = [n for n in range(P) if np.isfinite(s64[u, n])]
            clear = [n for n in live if (n == 0 or s64[u, n - 1] - s64[u, n] > 2 * tol[u])
                     and (n == P - 1 or s64[u, n] - s64[u, n + 1] > 2 * tol[u])]
            for n in clear:
                what = (W, O, K, u, n, hyps[u][n], h64[u][n], scores[u, n], s64[u, n])
                assert np.array_equal(hyps[u][n], h64[u][n]), what
                assert abs(scores[u, n] - s64[u, n]) <= max(tol[u], 1e-6 * abs(s64[u, n])), what
                assert abs(am[u, n] - a64[u, n]) <= max(tol[u], 1e-6 * abs(a64[u, n])), what
                worst = max(worst, abs(scores[u, n] - s64[u, n]))
            compared += len(clear)
    print("dense logits K = %d model %d: %d of %d utterances counted, %d entries compared, largest |device - float64| %.3e"
          % (K, with_lm, counted, total, compared, worst))
    assert compared >= 2 * counted


def test_known_answers_on_integer_logits(gpu):
    rows = known_answer_rows()
    for z, K, best, nbest in rows:
        for O in (z.shape[1], 70):  # the same rows inside a wider alphabet: the added labels are far below
            zz = z if O == z.shape[1] else np.concatenate(
                [z[:, :-1], np.full((z.shape[0], O - z.shape[1]), -30.0, np.float32), z[:, -1:]], axis=1)
            hyps, scores, am = _device_topk_logits(zz, [z.shape[0]], 8, 3, K)
            want_h, want_s, _ = prefix_beam_search_topk(zz, [z.shape[0]], 8, 3, K)
            assert hyps[0][0].tolist() == best
            if nbest is not None:
                assert [h.tolist() for h in hyps[0][:len(nbest)]] == nbest
            fin = np.isfinite(want_s[0])
            assert np.array_equal(np.isfinite(scores[0]), fin)
            assert np.abs(scores[0][fin] - want_s[0][fin]).max() <= 1e-5
    # the tie that K = 2 does not cut: (1) and (3) have the same score, bit for bit
    z, K, _, _ = rows[1]
    hyps, scores, _ = _device_topk_logits(z, [1], 8, 3, K)
    assert [h.tolist() for h in hyps[0]] == [[1], [3], []] and scores[0, 0] == scores[0, 1]


# ---- 4. the engine's entries ----
@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
@pytest.mark.parametrize("O", [65, 200])
def test_engine_entry_equals_restatement_on_the_engines_logits(gpu, dtype, O):
    rng = np.random.default_rng(400 + O)
    eng, _ = make_pair(rng, max_frames=512, compute_dtype=dtype, **dict(KW, output_dim=O))
    _sharpen(eng, rng, 6.0, 3.0)
    utt = [30, 0, 1, 55, 70, 2, 0, 44]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    labels, lab = _refs(rng, len(utt), O)
    z = eng.posteriors(X, raw_logits=True)
    P = 3
    lm = _parity_lm(O, 2)
    for W, K, model in ((10, 8, None), (32, 16, lm)):
        name = "%s O=%d W=%d K=%d model %d" % (dtype, O, W, K, model is not None)
        if model is None:
            hyps, scores, edits = eng.ctc_beam(X, utt, beam_width=W, top_paths=P, labels=labels, label_lens=lab, label_topk=K)
            am = scores
        else:
            hyps, scores, am, edits = eng.ctc_beam_lm(X, utt, model, beam_width=W, top_paths=P, labels=labels,
                                                      label_lens=lab, label_topk=K)
        assert scores.shape == (len(utt), P) and scores.dtype == np.float32 and edits.dtype == np.int32
        _check_best(name, z, utt, W, K, model, hyps, scores, am)
        assert edits.tolist() == [levenshtein(h[0], r) for h, r in zip(hyps, _split(labels, lab))]
        end = float(np.float32(model.weight) * model.table[-1, -1]) if model is not None else 0.0
        for u in (1, 6):
            assert all(p.size == 0 for p in hyps[u]) and scores[u].tolist() == [end] + [-np.inf] * (P - 1)
        # the logits entry on the engine's logits gives the same bits, and so does a second call
        alone = _device_topk_logits(z, utt, W, P, K, model)
        assert _same_hyps(alone[0], hyps) and alone[1].tobytes() == scores.tobytes() and alone[2].tobytes() == am.tobytes()
        if model is None:
            again = eng.ctc_beam(X, utt, beam_width=W, top_paths=P, label_topk=K)
            assert again[2] is None and again[1].tobytes() == scores.tobytes() and _same_hyps(again[0], hyps)
    assert sum(h[0].size for h in hyps) > 10
    # only zero-frame utterances: the binding fills the outputs itself
    hyps, scores, edits = eng.ctc_beam(X[:0], [0, 0], beam_width=4, top_paths=2, labels=[1, 2, 3], label_lens=[1, 2],
                                       label_topk=4)
    assert scores.tolist() == [[0.0, -np.inf]] * 2 and edits.tolist() == [1, 2]
    eng.close()


def test_raw_entry_equals_host_spliced_bit_for_bit(gpu):
    import torch
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(8)
    D, C, O = 4, 2, 90
    eng, _ = make_pair(rng, max_frames=256, **dict(KW, input_dim=D * (2 * C + 1), output_dim=O))
    _sharpen(eng, rng, 4.0, 2.0)
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 5, 63, 17)]
    lens = [u.shape[0] for u in utts]
    labels, lab = _refs(rng, len(utts), O)
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)
    lm = _parity_lm(O, 2)
    kw = dict(beam_width=20, top_paths=4, labels=labels, label_lens=lab, label_topk=12)

    def same(a, b):
        return (_same_hyps(a[0], b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:-1], b[1:-1]))
                and np.array_equal(a[-1], b[-1]))

    spliced = np.concatenate([u.spliced() for u in utts])
    host = eng.ctc_beam(spliced, lens, **kw)
    assert same(host, eng.ctc_beam_raw(raw, lens, C, cmvn=cmvn_table(utts), **kw))
    assert same(host, eng.ctc_beam_raw(torch.from_numpy(raw).cuda(), lens, C, cmvn=cmvn_table(utts), **kw))
    host_lm = eng.ctc_beam_lm(spliced, lens, lm, **kw)
    assert same(host_lm, eng.ctc_beam_lm_raw(raw, lens, C, lm, cmvn=cmvn_table(utts), **kw))
    assert same(host_lm, eng.ctc_beam_lm_raw(torch.from_numpy(raw).cuda(), lens, C, lm, cmvn=cmvn_table(utts), **kw))
    assert not _same_hyps(host[0], host_lm[0])  # (the model is used)
    assert host[2].tolist() == [levenshtein(h[0], r) for h, r in zip(host[0], _split(labels, lab))]
    assert sum(h[0].size for h in host[0]) > 5
    eng.close()


def _engine_state(eng):
    """everything a decoding call must leave alone, as bytes: parameters, gradient accumulators, Adam moments, batch-norm
    statistics, the step counters and the accumulated loss and frame count"""
    from tfkaldi_amd import _lib
    state = {"p" + k: v.tobytes() for k, v in engine_params(eng).items()}
    state.update(("g" + k, v.tobytes()) for k, v in engine_grads(eng).items())
    for l in range(eng.L + 1):
        for slot in (_lib.SLOT_ADAM_M, _lib.SLOT_ADAM_V):
            state["adam%d W%d" % (slot, l)] = eng.get(_lib.WEIGHTS, l, slot).tobytes()
            state["adam%d b%d" % (slot, l)] = eng.get(_lib.BIASES, l, slot).tobytes()
    for l in range(eng.L):
        state["mean%d" % l] = eng.get(_lib.BN_MOVING_MEAN, l).tobytes()
        state["var%d" % l] = eng.get(_lib.BN_MOVING_VAR, l).tobytes()
    for which in (_lib.GLOBAL_STEP, _lib.ADAM_STEPS, _lib.BATCH_LOSS, _lib.NUM_FRAMES):
        state["scalar%d" % which] = eng.scalar(which)
    state["checksum"] = eng.param_checksum(0)
    return state


def test_old_entries_are_what_they_were_around_a_pruned_call(gpu):
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    rng = np.random.default_rng(31)
    utt = [50, 0, 33]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    # a wide engine: the old entries refuse it before and after, a pruned call leaves everything else untouched
    wide, _ = make_pair(rng, max_frames=256, **dict(KW, output_dim=65))
    _sharpen(wide, rng, 6.0, 3.0)
    lm = _parity_lm(65, 2)
    wide.ctc_set_lm(lm)  # (accepted now: a model over 65 outputs)
    # one whole step, then the first micro-batch of the next: the moments, the statistics and the accumulators all hold
    # something when the pruned calls come
    labels, lab = _refs(rng, 2, 65, 2, 6)
    wide.accumulate_ctc(X[:50], [50], labels[:lab[0]], [lab[0]], last=True)
    wide.apply()
    wide.accumulate_ctc(X[50:], [33], labels[lab[0]:], [lab[1]])
    state0 = _engine_state(wide)
    assert any(np.frombuffer(state0[k], np.float32).any() for k in state0 if k.startswith("gW"))
    w0 = wide.get(_lib.WEIGHTS, wide.L).copy()
    post0 = wide.posteriors(X)
    for _ in range(2):
        with pytest.raises(EngineError, match="output_dim"):
            wide.ctc_beam(X, utt, beam_width=4)
        with pytest.raises(EngineError, match="output_dim"):
            wide.ctc_beam_lm(X, utt, lm, beam_width=4)
        got = wide.ctc_beam_lm(X, utt, lm, beam_width=8, top_paths=2, label_topk=6)
        assert np.isfinite(got[1][0]).all() and wide._lm_table is lm.table
    assert got[1].tobytes() == wide.ctc_beam_lm(X, utt, lm, beam_width=8, top_paths=2, label_topk=6)[1].tobytes()
    wide.ctc_beam(X, utt, beam_width=8, top_paths=2, label_topk=6)
    assert np.array_equal(wide.get(_lib.WEIGHTS, wide.L), w0) and np.array_equal(wide.posteriors(X), post0)
    state1 = _engine_state(wide)
    assert sorted(state1) == sorted(state0)
    for k in state0:
        assert state1[k] == state0[k], k
    # the model on the device is the one that was set: the old model entry's twin at K = 63 would need O <= 64, so it is read
    # back through a pruned call whose model term is known -- score - am_score of every best path is the model's value
    got = wide.ctc_beam_lm(X, utt, lm, beam_width=8, top_paths=1, label_topk=6)
    assert wide._lm_table is lm.table
    for u in range(len(utt)):  # (float32: two roundings per label in the kernel's sum, one in each output)
        sc, ac, path = float(got[1][u, 0]), float(got[2][u, 0]), got[0][u][0]
        assert abs((sc - ac) - lm.score(path)) <= (2 * path.size + 2) * np.spacing(np.float32(abs(sc) + abs(ac) + 1.0))
    wide.close()
    # a narrow engine: the old entries give the same bits before and after a pruned call, and K >= O - 1 gives them too
    eng, _ = make_pair(rng, max_frames=256, **KW)
    _sharpen(eng, rng, 6.0, 3.0)
    lm9 = _random_lm(rng, KW["output_dim"], 3, eos=True)
    before = eng.ctc_beam(X, utt, beam_width=16, top_paths=3)
    before_lm = eng.ctc_beam_lm(X, utt, lm9, beam_width=16, top_paths=3)
    pruned = eng.ctc_beam(X, utt, beam_width=16, top_paths=3, label_topk=2)
    full = eng.ctc_beam(X, utt, beam_width=16, top_paths=3, label_topk=63)
    full_lm = eng.ctc_beam_lm(X, utt, lm9, beam_width=16, top_paths=3, label_topk=8)
    after = eng.ctc_beam(X, utt, beam_width=16, top_paths=3)
    after_lm = eng.ctc_beam_lm(X, utt, lm9, beam_width=16, top_paths=3)
    for a, b in ((before, after), (before, full), (before_lm, after_lm), (before_lm, full_lm)):
        assert _same_hyps(a[0], b[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:-1], b[1:-1]))
    assert pruned[1].tobytes() != before[1].tobytes()  # (K = 2 of 8 labels does prune)
    eng.close()


# ---- 5. limits ----
def test_limits_are_reported_and_leave_the_engine_usable(gpu):
    import torch
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    rng = np.random.default_rng(13)
    O = 80
    eng, _ = make_pair(rng, max_frames=256, **dict(KW, output_dim=O))
    utt = [20, 15]
    X = rng.standard_normal((35, KW["input_dim"])).astype(np.float32)
    good = eng.ctc_beam(X, utt, beam_width=16, top_paths=2, label_topk=8)
    h, n = np.empty((3, 35), np.int32), np.empty((3, 2), np.int32)
    s, a = np.empty((3, 2), np.float32), np.empty((3, 2), np.float32)
    lens = np.array(utt, np.int32)
    ptr = lambda x: x.ctypes.data_as(c_void_p)
    null = c_void_p(None)
    call = lambda W, P, K, flags=0: eng.lib.tfk_ctc_beam_topk(
        eng._h, ptr(X), X.shape[1], 35, ptr(lens), 2, W, P, K, c_float(0.6), c_float(0.4), null, null, ptr(h), ptr(n), ptr(s),
        ptr(a), null, flags)

    def usable():
        again = eng.ctc_beam(X, utt, beam_width=16, top_paths=2, label_topk=8)
        assert again[1].tobytes() == good[1].tobytes() and _same_hyps(again[0], good[0])

    for W, P, K, flags, word in ((4, 1, 0, 0, b"label_topk"), (4, 1, 64, 0, b"label_topk"), (129, 1, 8, 0, b"128"),
                                 (4, 5, 8, 0, b"top_paths"), (4, 1, 8, _lib.RAW_DEVICE, b"flags"),
                                 (4, 1, 8, _lib.CTC_LM, b"no language model"),
                                 (4, 1, 8, _lib.CTC_LM_EOS, b"TFK_CTC_LM")):
        assert call(W, P, K, flags) != 0
        assert word in eng.lib.tfk_last_error(), (W, P, K, flags, eng.lib.tfk_last_error())
        usable()
    for K in (0, 64):
        with pytest.raises(EngineError, match="label_topk"):
            eng.ctc_beam(X, utt, beam_width=4, label_topk=K)
    assert call(3, 3, 63) == 0 and np.array_equal(s, a)  # without the model am_score is score
    # a table above 2^26 entries is refused by its size alone: nothing of it is read (4 floats stand in for 10^9)
    lm = _parity_lm(O, 2)
    eng.ctc_set_lm(lm)
    with_lm = eng.ctc_beam_lm(X, utt, lm, beam_width=16, top_paths=2, label_topk=8)
    wide, _ = make_pair(rng, max_frames=256, **dict(KW, output_dim=1000))
    tiny = np.zeros(4, np.float32)
    assert wide.lib.tfk_ctc_lm_set(wide._h, ptr(tiny), 3) != 0
    assert b"67108864" in wide.lib.tfk_last_error() and b"entries" in wide.lib.tfk_last_error()
    assert len(wide.ctc_greedy(X, utt)[0]) == 2
    assert np.isfinite(wide.ctc_beam(X, utt, beam_width=4, label_topk=4)[1]).all()
    wide.close()
    again = eng.ctc_beam_lm(X, utt, lm, beam_width=16, top_paths=2, label_topk=8)  # the other engine kept its model
    assert again[1].tobytes() == with_lm[1].tobytes()
    assert call(3, 3, 8, _lib.CTC_LM) == 0 and call(3, 3, 8, _lib.CTC_LM | _lib.CTC_LM_EOS) == 0
    usable()
    eng.close()
    # the logits entry: O = 65537, a label_topk of 0 and 64, the end flag without a table
    z = np.zeros((4, 8), np.float32)
    for K, word in ((0, b"label_topk"), (64, b"label_topk")):
        rc, msg = _device_topk_logits(z, [4], 4, 1, K, check=False)
        assert rc != 0 and word in msg
    lib = _lib.load()
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = c_void_p(d.data_ptr())
    assert lib.tfk_ctc_beam_topk_logits(c_void_p(0), p, 65537, 65537, 0, p, 1, 4, 1, 8, null, 0, c_float(0), c_float(0), 0,
                                        p, p, p, p) != 0
    assert b"65536" in lib.tfk_last_error()
    assert lib.tfk_ctc_beam_topk_logits(c_void_p(0), p, 8, 8, 4, p, 1, 4, 1, 8, null, 0, c_float(0), c_float(0),
                                        _lib.CTC_LM_EOS, p, p, p, p) != 0
    assert b"TFK_CTC_LM_EOS" in lib.tfk_last_error()
    assert lib.tfk_ctc_beam_topk_logits(c_void_p(0), p, 1000, 1000, 0, p, 1, 4, 1, 8, p, 3, c_float(0), c_float(0), 0,
                                        p, p, p, p) != 0
    assert b"entries" in lib.tfk_last_error()


# ---- 6. end to end, with a model of more than 64 outputs ----
WIDE_O = 80


def test_decoder_and_trainer_end_to_end(gpu, tmp_path):
    from tfkaldi_amd._lib import EngineError
    from tfkaldi_amd.neuralNetworks.classifiers import activation as act
    from tfkaldi_amd.neuralNetworks.classifiers.dnn import DNN
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    _, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    assert coder.num_labels < WIDE_O - 1
    dnn = DNN(WIDE_O, 2, 48, act.TfActivation(act.Batchnorm(None), "relu"), False)  # the blank is class 79
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    for _ in range(60):
        tr.update(xs, ys)
    lm = NgramLM.from_label_sequences(ys, WIDE_O - 1, 2, weight=0.5, label_bonus=1.0)
    greedy = tr.label_errors(xs, ys)
    with pytest.raises(EngineError, match="output_dim"):
        tr.label_errors(xs, ys, beam_width=10)  # the unpruned search still refuses 80 outputs
    plain = tr.label_errors(xs, ys, beam_width=10, label_topk=8)
    with_lm = tr.label_errors(xs, ys, beam_width=10, lm=lm, label_topk=8)
    assert type(plain[0]) is int and plain[1] == with_lm[1] == greedy[1] == sum(len(y) for y in ys)
    with pytest.raises(ValueError, match="beam_width"):
        tr.label_errors(xs, ys, label_topk=8)
    flat, lens = np.concatenate(xs), [len(x) for x in xs]
    hyps, scores, _ = tr.engine.ctc_beam(flat, lens, beam_width=10, top_paths=2, label_topk=8)
    assert plain[0] == sum(levenshtein(h[0], np.asarray(y).astype(np.int64)) for h, y in zip(hyps, ys))
    hyps_lm, scores_lm, am_lm, _ = tr.engine.ctc_beam_lm(flat, lens, lm, beam_width=10, top_paths=2, label_topk=8)
    assert with_lm[0] == sum(levenshtein(h[0], np.asarray(y).astype(np.int64)) for h, y in zip(hyps_lm, ys))
    print("toy model with %d outputs after 60 updates: label errors greedy %d, pruned beam %d, + model %d of %d"
          % (WIDE_O, greedy[0], plain[0], with_lm[0], plain[1]))
    assert plain[0] <= 2 * greedy[0] + 2  # (the search is no stranger to the model it decodes)
    tr.save_model(str(tmp_path / "model"))
    tr.close()
    dec = Decoder(dnn, F, maxlen)
    dec.restore(str(tmp_path / "model"))
    got, got_scores = dec.ctc_beam_search(xs, beam_width=10, top_paths=2, label_topk=8)
    assert got_scores.tobytes() == scores.tobytes() and _same_hyps(got, hyps)
    got, got_scores, got_am = dec.ctc_beam_search_lm(xs, lm, beam_width=10, top_paths=2, label_topk=8)
    assert got_scores.tobytes() == scores_lm.tobytes() and got_am.tobytes() == am_lm.tobytes() and _same_hyps(got, hyps_lm)
    assert all(isinstance(coder.decode(h[0]), str) for h in got)
    assert dec.ctc_beam_search([], label_topk=8)[0] == []
    dec.close()


def _dp_lm():
    return _parity_lm(WIDE_O, 2)


def _dp_worker(rank, world, port, num_mb, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), TFK_SHARE_DEVICE="1", TFK_DIST_BACKEND="gloo")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from tfkaldi_amd.dataparallel import CtcMicroBatch, DataParallel, init_from_env
    from util import make_pair as pair
    init_from_env()
    dp = DataParallel()
    assert dp.enabled
    eng, _ = pair(np.random.default_rng(5), max_frames=256, torch_state=True, **dict(KW, output_dim=WIDE_O))
    mbs = [CtcMicroBatch(*mb) for mb in _dp_data(num_mb, 3)]
    got = dp.label_errors(eng, mbs, beam_width=10, lm=_dp_lm(), label_topk=6)
    got += dp.label_errors(eng, mbs, beam_width=10, label_topk=6)
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(got, dtype=np.int64))
    eng.close()
    dist.destroy_process_group()


def test_label_errors_two_ranks_equal_single_process(gpu, tmp_path):
    import torch.multiprocessing as mp
    from tfkaldi_amd.dataparallel import CtcMicroBatch, DataParallel
    world, num_mb = 2, 3
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_worker, args=(world, port, num_mb, str(tmp_path)), nprocs=world, join=True)
    eng, _ = make_pair(np.random.default_rng(5), max_frames=256, **dict(KW, output_dim=WIDE_O))
    mbs = [CtcMicroBatch(*mb) for mb in _dp_data(num_mb, 3)]
    want = DataParallel().label_errors(eng, mbs, beam_width=10, lm=_dp_lm(), label_topk=6)
    want += DataParallel().label_errors(eng, mbs, beam_width=10, label_topk=6)
    eng.close()
    assert want[0] > 0 and want[1] > 0 and want[2] > 0
    for rank in range(world):
        assert tuple(np.load(os.path.join(str(tmp_path), "rank%d.npy" % rank)).tolist()) == want
