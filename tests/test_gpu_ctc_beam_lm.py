"""CTC prefix beam search with a character n-gram language model on the device (tfk_ctc_lm_set / tfk_ctc_beam_lm /
tfk_ctc_beam_lm_raw / tfk_ctc_beam_lm_logits, csrc/ctc.hip) against the float64 numpy restatement of
tests/test_ctc_beam_lm_host.py applied to the SAME logits and the same table.

Tolerance and hypothesis band are those of tests/test_gpu_ctc_beam.py, applied to the COMBINED score: `tol` = 4 x the largest
|float32 run - float64 run| of the restatement's best score on the same inputs, floored at 1e-6 x |score|; the device's best
path must be one of the restatement's hypotheses within 2 tol of its best; that this band holds a single hypothesis for at
least 75 % of a test's utterances is asserted on the restatement alone, before the device is consulted."""
import os
import socket
import sys
from ctypes import c_float, c_void_p

import numpy as np
import pytest

from test_ctc_beam_host import ctc_log_prob, enumeration_cases, log_softmax, peaky_logits, prefix_beam_search
from test_ctc_beam_lm_host import enumeration_lm, prefix_beam_search_lm
from test_ctc_decode_host import levenshtein
from test_gpu_ctc_beam import KW, _device_beam_logits, _dp_data, _sharpen
from test_gpu_ctc_decode import _refs, _split, _toy_ctc
from util import make_pair

from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_lm(rng, O, order, weight=0.6, bonus=0.4, eos=False):
    return NgramLM(log_softmax(1.5 * rng.standard_normal((O ** (order - 1), O))), order, weight=weight, label_bonus=bonus,
                   end_of_sequence=eos)


def _device_beam_lm_logits(z, utt, W, P, lm):
    """tfk_ctc_beam_lm_logits on host logits: (hyps[u][n], scores [U, P], am_scores [U, P])"""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    T, O = z.shape
    assert O == lm.num_classes
    U = len(utt)
    seg = np.concatenate([[0], np.cumsum(utt)]).astype(np.int32)
    d_z, d_seg = torch.from_numpy(z).cuda(), torch.from_numpy(seg).cuda()
    d_lm = torch.from_numpy(lm.table).cuda()
    hyp = torch.full((P, max(T, 1)), -7, dtype=torch.int32, device="cuda")
    hyp_len = torch.full((P, U), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    am = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tfk_ctc_beam_lm_logits(
        c_void_p(stream), c_void_p(d_z.data_ptr()), O, O, T, c_void_p(d_seg.data_ptr()), U, W, P, c_void_p(d_lm.data_ptr()),
        lm.order, c_float(lm.weight), c_float(lm.label_bonus), _lib.CTC_LM_EOS if lm.end_of_sequence else 0,
        c_void_p(hyp.data_ptr()), c_void_p(hyp_len.data_ptr()), c_void_p(score.data_ptr()), c_void_p(am.data_ptr())))
    torch.cuda.synchronize()
    hyp, hyp_len, score, am = hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy(), am.cpu().numpy()
    for n in range(P):  # the rows past a hypothesis are -1
        for u in range(U):
            assert np.all(hyp[n, seg[u] + hyp_len[n, u]:seg[u + 1]] == -1)
    hyps = [[hyp[n, seg[u]:seg[u] + hyp_len[n, u]].copy() for n in range(P)] for u in range(U)]
    return hyps, score.T.copy(), am.T.copy()


def _restatement(z, utt, W, lm, P=8):
    """float64 N-best of the restatement and the per-utterance tol from its own float32 run"""
    P = min(P, W)
    h64, s64, a64 = prefix_beam_search_lm(z, utt, W, P, lm)
    _, s32, _ = prefix_beam_search_lm(z, utt, W, 1, lm, dtype=np.float32)
    tol = np.maximum(4.0 * np.abs(s32[:, 0] - s64[:, 0]).max(), 1e-6 * np.abs(s64[:, 0]))
    return h64, s64, a64, tol


def _check_best(name, z, utt, W, lm, hyps, scores, am, must_change=None):
    """every utterance's best path: combined score within tol of the restatement's, the hypothesis inside its 2-tol band,
    score - am_score = the model's value of the labels, am_score no more than the labels' exact log-probability.
    must_change: the utterances whose best path the model has to change (asserted on the restatements alone)."""
    h64, s64, a64, tol = _restatement(z, utt, W, lm)
    U = len(utt)
    band = [[n for n in range(s64.shape[1]) if s64[u, n] >= s64[u, 0] - 2 * tol[u]] for u in range(U)]
    crowded = sum(len(b) > 1 for b in band)
    assert 4 * crowded <= U, "%s: %d of %d utterances have rivals within 2 tol of the best" % (name, crowded, U)
    if must_change is not None:
        plain = prefix_beam_search(z, utt, W, 1)[0]
        same = [u for u in must_change if np.array_equal(plain[u][0], h64[u][0])]
        assert not same, "%s: the model leaves the best path of utterances %s alone" % (name, same)
    seg = np.concatenate([[0], np.cumsum(utt)])
    worst = 0.0
    for u in range(U):
        got, sc, ac = hyps[u][0], float(scores[u, 0]), float(am[u, 0])
        err = abs(sc - s64[u, 0])
        print("%s utt %d: T %d labels %d device %.6f float64 %.6f am %.6f |diff| %.2e tol %.2e band %d"
              % (name, u, utt[u], got.size, sc, s64[u, 0], ac, err, tol[u], len(band[u])))
        assert err <= tol[u], (name, u, sc, s64[u, 0], tol[u])
        assert any(np.array_equal(got, h64[u][n]) for n in band[u]), (name, u, got, h64[u][0])
        # (both values come back as float32: on top of tol, half a unit in the last place of each, which a score of
        # several hundred makes comparable to tol itself)
        ulps = 0.5 * (np.spacing(np.float32(abs(sc))) + np.spacing(np.float32(abs(ac))))
        assert abs((sc - ac) - lm.score(got)) <= tol[u] + ulps, (name, u, sc, ac, lm.score(got))
        assert ac <= ctc_log_prob(z[seg[u]:seg[u + 1]], got) + tol[u], (name, u, ac)
        worst = max(worst, err)
    print("%s: largest |device - float64| %.3e, smallest tol %.3e" % (name, worst, tol.min()))


# ---- 1. weight 0 is the acoustic search, bit for bit ----
def _zero_weight_cases():
    cases = enumeration_cases()
    yield "enumeration", np.concatenate(cases).astype(np.float32), [6] * len(cases), 128, 2
    z = peaky_logits(np.random.default_rng(61), 8 * 200, 36, 8 * 25)
    for W in (1, 10, 100):
        yield "peaky W=%d" % W, z, [200] * 8, W, 2 if W == 10 else 3
    yield "full key table", (2.0 * np.random.default_rng(64).standard_normal((4 * 30, 64))).astype(np.float32), [30] * 4, 128, 3


def test_zero_weight_equals_the_acoustic_search_bit_for_bit(gpu):
    rng = np.random.default_rng(1)
    for name, z, utt, W, order in _zero_weight_cases():
        O = z.shape[1]
        lm = NgramLM(3.0 * rng.standard_normal((O ** (order - 1), O)), order, weight=0.0, label_bonus=0.0)
        P = min(3, W)
        want_h, want_s = _device_beam_logits(z, utt, W, P)
        hyps, scores, am = _device_beam_lm_logits(z, utt, W, P, lm)
        assert all(np.array_equal(a, b) for x, y in zip(hyps, want_h) for a, b in zip(x, y)), name
        assert scores.tobytes() == want_s.tobytes() and am.tobytes() == scores.tobytes(), name
        assert sum(h[0].size for h in hyps) > 0


# ---- 2. the enumeration cases with the model ----
@pytest.mark.parametrize("eos", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_enumeration_cases_with_the_model(gpu, order, eos):
    lm = enumeration_lm(order, eos)
    cases = enumeration_cases()
    z = np.concatenate(cases).astype(np.float32)
    utt = [6] * len(cases)
    P = 8
    hyps, scores, am = _device_beam_lm_logits(z, utt, 128, P, lm)
    h64, s64, a64, tol = _restatement(z, utt, 128, lm, P)
    worst = 0.0
    for u in range(len(utt)):
        assert np.array_equal(hyps[u][0], h64[u][0]), (u, hyps[u][0], h64[u][0])
        clear = [n for n in range(P) if (n == 0 or s64[u, n - 1] - s64[u, n] > 2 * tol[u])
                 and (n == P - 1 or s64[u, n] - s64[u, n + 1] > 2 * tol[u])]
        assert 0 in clear and len(clear) >= 4
        for n in clear:
            assert np.array_equal(hyps[u][n], h64[u][n]), (u, n)
            tol_n = max(tol[u], 1e-6 * abs(s64[u, n]))
            assert abs(scores[u, n] - s64[u, n]) <= tol_n, (u, n, scores[u, n], s64[u, n], tol_n)
            assert abs(am[u, n] - a64[u, n]) <= max(tol[u], 1e-6 * abs(a64[u, n])), (u, n, am[u, n], a64[u, n])
            worst = max(worst, abs(scores[u, n] - s64[u, n]))
    print("enumeration cases order %d eos %d: largest |device - float64| %.3e, smallest tol %.3e"
          % (order, eos, worst, tol.min()))


# ---- 3. + 4. restatement parity, and the acoustic part ----
def _parity_case(name):
    if name == "O9 W10 order2" or name == "O9 W100 order3":
        rng = np.random.default_rng(90)
        z = (2.0 * rng.standard_normal((16 * 40, 9))).astype(np.float32)
        W, order = (10, 2) if name == "O9 W10 order2" else (100, 3)
        return z, [40] * 16, W, _random_lm(np.random.default_rng(91), 9, order)
    if name == "O36 peaky W10 order2":
        rng = np.random.default_rng(61)
        return peaky_logits(rng, 8 * 200, 36, 8 * 25), [200] * 8, 10, _random_lm(rng, 36, 2)
    if name == "O64 W100 order3":
        rng = np.random.default_rng(64)
        return (2.0 * rng.standard_normal((8 * 30, 64))).astype(np.float32), [30] * 8, 100, _random_lm(rng, 64, 3)
    assert name == "O16 W10 order4"
    rng = np.random.default_rng(16)
    return (2.0 * rng.standard_normal((8 * 40, 16))).astype(np.float32), [40] * 8, 10, _random_lm(rng, 16, 4)


@pytest.mark.parametrize("name", ["O9 W10 order2", "O9 W100 order3", "O36 peaky W10 order2", "O64 W100 order3",
                                  "O16 W10 order4"])
def test_standalone_entry_equals_restatement(gpu, name):
    z, utt, W, lm = _parity_case(name)
    hyps, scores, am = _device_beam_lm_logits(z, utt, W, 3, lm)
    _check_best(name, z, utt, W, lm, hyps, scores, am, must_change=range(len(utt)))
    assert np.all(scores[:, :-1] >= scores[:, 1:])  # best first, by the combined score


@pytest.mark.parametrize("eos", [False, True])
def test_edge_shapes(gpu, eos):
    """a one-frame and a zero-frame utterance among longer ones; W = 1; one label + blank.  The model changes the best path
    of every utterance it can (not of zero-frame ones, nor of the one-frame utterance 1, where the best label stays best)."""
    rng = np.random.default_rng(17)
    utt = [23, 1, 0, 40, 0, 1, 16]
    z = (2.0 * rng.standard_normal((sum(utt), 9))).astype(np.float32)
    lm = _random_lm(rng, 9, 3, eos=eos)
    for W in (1, 10):
        P = min(2, W)
        hyps, scores, am = _device_beam_lm_logits(z, utt, W, P, lm)
        _check_best("edges eos %d W=%d" % (eos, W), z, utt, W, lm, hyps, scores, am, must_change=[0, 3, 5, 6])
        for u in (2, 4):  # zero frames: the empty hypothesis, acoustic 0, combined 0 or the end term of the start context
            end = np.float32(lm.weight) * lm.table[-1, -1] if eos else np.float32(0.0)
            assert all(h.size == 0 for h in hyps[u])
            assert am[u].tolist() == [0.0] + [-np.inf] * (P - 1) and scores[u].tolist() == [float(end)] + [-np.inf] * (P - 1)
    # one label: a model that makes the label improbable (p = 0.0025 after itself, 0.0025 at the start) shortens every path
    z2 = (2.0 * np.random.default_rng(171).standard_normal((20, 2))).astype(np.float32)
    lm2 = NgramLM(log_softmax(np.array([[-4.0, 2.0], [-5.0, 1.0]])), 2, weight=0.6, label_bonus=0.4, end_of_sequence=eos)
    utt2 = [12, 7, 1, 0]
    hyps, scores, am = _device_beam_lm_logits(z2, utt2, 4, 2, lm2)
    _check_best("one label eos %d" % eos, z2, utt2, 4, lm2, hyps, scores, am, must_change=[0, 1, 2])
    all_empty = _device_beam_lm_logits(np.zeros((0, 9), np.float32), [0, 0], 4, 1, lm)
    assert all(h[0].size == 0 for h in all_empty[0]) and all_empty[2].tolist() == [[0.0], [0.0]]


# ---- 5. the engine's entries ----
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("O", [9, 36])
def test_engine_entry_equals_restatement_on_the_engines_logits(gpu, dtype, O):
    rng = np.random.default_rng(200 + O)
    eng, _ = make_pair(rng, max_frames=512, compute_dtype=dtype, **dict(KW, output_dim=O))
    _sharpen(eng, rng, 6.0, 3.0)
    utt = [30, 0, 1, 77, 140, 2, 0, 65]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    labels, lab = _refs(rng, len(utt), O)
    z = eng.posteriors(X, raw_logits=True)
    for W, eos in ((10, False), (100, True)):
        lm = _random_lm(rng, O, 2, eos=eos)
        P = 3
        hyps, scores, am, edits = eng.ctc_beam_lm(X, utt, lm, beam_width=W, top_paths=P, labels=labels, label_lens=lab)
        assert scores.shape == am.shape == (len(utt), P) and scores.dtype == am.dtype == np.float32
        assert edits.dtype == np.int32
        _check_best("%s O=%d W=%d" % (dtype, O, W), z, utt, W, lm, hyps, scores, am)
        assert edits.tolist() == [levenshtein(h[0], r) for h, r in zip(hyps, _split(labels, lab))]
        end = float(np.float32(lm.weight) * lm.table[-1, -1]) if eos else 0.0
        for u in (1, 6):
            assert all(p.size == 0 for p in hyps[u]) and scores[u].tolist() == [end] + [-np.inf] * (P - 1)
            assert am[u].tolist() == [0.0] + [-np.inf] * (P - 1)
        alone = eng.ctc_beam_lm(X, utt, lm, beam_width=W, top_paths=P)  # (7. two calls agree bit for bit)
        assert alone[3] is None and alone[1].tobytes() == scores.tobytes() and alone[2].tobytes() == am.tobytes()
        assert all(np.array_equal(a, b) for x, y in zip(alone[0], hyps) for a, b in zip(x, y))
    assert sum(h[0].size for h in hyps) > 20
    # only zero-frame utterances: the binding fills the outputs itself, by the same rule
    hyps, scores, am, edits = eng.ctc_beam_lm(X[:0], [0, 0], lm, beam_width=4, top_paths=2, labels=[1, 2, 3], label_lens=[1, 2])
    assert scores.tolist() == [[end, -np.inf]] * 2 and am.tolist() == [[0.0, -np.inf]] * 2 and edits.tolist() == [1, 2]
    eng.close()


def test_raw_entry_equals_host_spliced_bit_for_bit(gpu):
    import torch
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(8)
    D, C = 4, 2
    eng, _ = make_pair(rng, max_frames=256, **dict(KW, input_dim=D * (2 * C + 1), output_dim=12))
    _sharpen(eng, rng, 4.0, 2.0)
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 5, 63, 17)]
    lens = [u.shape[0] for u in utts]
    labels, lab = _refs(rng, len(utts), 12)
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)
    lm = _random_lm(rng, 12, 3, eos=True)
    kw = dict(beam_width=20, top_paths=4, labels=labels, label_lens=lab)

    def same(a, b):
        return (all(np.array_equal(p, q) for x, y in zip(a[0], b[0]) for p, q in zip(x, y))
                and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and np.array_equal(a[3], b[3]))

    spliced = np.concatenate([u.spliced() for u in utts])
    host = eng.ctc_beam_lm(spliced, lens, lm, **kw)
    dev = eng.ctc_beam_lm_raw(raw, lens, C, lm, cmvn=cmvn_table(utts), **kw)
    cuda = eng.ctc_beam_lm_raw(torch.from_numpy(raw).cuda(), lens, C, lm, cmvn=cmvn_table(utts), **kw)
    assert same(host, dev) and same(host, cuda)
    assert same(host, eng.ctc_beam_lm(spliced, lens, lm, **kw))  # two identical calls are bit-identical
    assert host[3].tolist() == [levenshtein(h[0], r) for h, r in zip(host[0], _split(labels, lab))]
    assert sum(h[0].size for h in host[0]) > 5
    eng.close()


# ---- 6. tfk_ctc_beam ignores the model ----
def test_the_acoustic_entry_ignores_the_model(gpu):
    rng = np.random.default_rng(23)
    eng, _ = make_pair(rng, max_frames=256, **KW)
    _sharpen(eng, rng, 6.0, 3.0)
    utt = [50, 0, 33]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    lm = _random_lm(rng, KW["output_dim"], 3, weight=2.0, bonus=1.0)

    def same(a, b):
        return all(np.array_equal(p, q) for x, y in zip(a[0], b[0]) for p, q in zip(x, y)) and a[1].tobytes() == b[1].tobytes()

    before = eng.ctc_beam(X, utt, beam_width=16, top_paths=3)
    eng.ctc_set_lm(lm)
    assert same(before, eng.ctc_beam(X, utt, beam_width=16, top_paths=3))
    with_lm = eng.ctc_beam_lm(X, utt, lm, beam_width=16, top_paths=3)
    assert not same(before, with_lm[:2])  # (the model entry does use it)
    eng.ctc_set_lm(None)
    assert same(before, eng.ctc_beam(X, utt, beam_width=16, top_paths=3))
    # the binding skips the upload for the table it has set, and uploads another one
    eng.ctc_set_lm(lm)
    held = eng._lm_table
    eng.ctc_set_lm(lm)
    assert eng._lm_table is held and held is lm.table
    other = _random_lm(rng, KW["output_dim"], 1, weight=2.0, bonus=1.0)
    assert not same(with_lm[:2], eng.ctc_beam_lm(X, utt, other, beam_width=16, top_paths=3)[:2]) and eng._lm_table is other.table
    assert same(with_lm[:2], eng.ctc_beam_lm(X, utt, lm, beam_width=16, top_paths=3)[:2])
    eng.close()


# ---- 8. limits ----
def test_limits_are_reported_and_leave_the_engine_usable(gpu):
    from tfkaldi_amd._lib import EngineError, check
    rng = np.random.default_rng(13)
    eng, _ = make_pair(rng, max_frames=256, **KW)
    O = KW["output_dim"]
    utt = [20, 15]
    X = rng.standard_normal((35, KW["input_dim"])).astype(np.float32)
    lm = _random_lm(rng, O, 2)
    h, n = np.empty((3, 35), np.int32), np.empty((3, 2), np.int32)
    s, a = np.empty((3, 2), np.float32), np.empty((3, 2), np.float32)
    lens = np.array(utt, np.int32)
    ptr = lambda x: x.ctypes.data_as(c_void_p)
    null = c_void_p(None)
    call = lambda W, P, flags=0: eng.lib.tfk_ctc_beam_lm(eng._h, ptr(X), X.shape[1], 35, ptr(lens), 2, W, P, c_float(0.6),
                                                         c_float(0.4), null, null, ptr(h), ptr(n), ptr(s), ptr(a), null, flags)
    assert call(4, 1) != 0 and b"no language model" in eng.lib.tfk_last_error()  # nothing set yet
    good = eng.ctc_beam_lm(X, utt, lm, beam_width=16, top_paths=2)
    table = np.ascontiguousarray(lm.table)
    for order in (0, 5):
        assert eng.lib.tfk_ctc_lm_set(eng._h, ptr(table), order) != 0 and b"order" in eng.lib.tfk_last_error()
    for bad in (np.nan, np.inf):
        t = table.copy()
        t[3, 4] = bad
        assert eng.lib.tfk_ctc_lm_set(eng._h, ptr(t), 2) != 0 and b"entry %d " % (3 * O + 4) in eng.lib.tfk_last_error()
    for W, P, flags, word in ((4, 5, 0, b"top_paths"), (129, 1, 0, b"128"), (4, 1, 1, b"flags")):
        assert call(W, P, flags) != 0
        assert word in eng.lib.tfk_last_error(), (W, P, eng.lib.tfk_last_error())
    with pytest.raises(ValueError, match="top_paths"):
        eng.ctc_beam_lm(X, utt, lm, beam_width=2, top_paths=3)
    with pytest.raises(ValueError, match="labels"):
        eng.ctc_beam_lm(X, utt, _random_lm(rng, O + 1, 2), beam_width=4)
    # every rejected call left the model and the engine as they were
    again = eng.ctc_beam_lm(X, utt, lm, beam_width=16, top_paths=2)
    assert again[1].tobytes() == good[1].tobytes() and again[2].tobytes() == good[2].tobytes()
    assert call(3, 3) == 0 and call(3, 3, 32) == 0
    eng.ctc_set_lm(None)
    assert call(4, 1) != 0 and b"no language model" in eng.lib.tfk_last_error()  # dropped
    with pytest.raises(EngineError, match="order"):
        check(eng.lib.tfk_ctc_lm_set(eng._h, ptr(table), 7))
    assert len(eng.ctc_greedy(X, utt)[0]) == 2
    eng.close()


# ---- 9. end to end ----
def _toy_lm(ys, num_labels):
    return NgramLM.from_label_sequences(ys, num_labels, 2, weight=0.5, label_bonus=1.0)


def test_decoder_and_trainer_end_to_end(gpu, tmp_path):
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    for _ in range(60):
        tr.update(xs, ys)
    lm = _toy_lm(ys, coder.num_labels)
    plain = tr.label_errors(xs, ys, beam_width=10)
    with_lm = tr.label_errors(xs, ys, beam_width=10, lm=lm)
    assert type(with_lm[0]) is int and with_lm[1] == plain[1] == sum(len(y) for y in ys)
    with pytest.raises(ValueError, match="beam_width"):
        tr.label_errors(xs, ys, lm=lm)
    assert tr.label_errors(xs, ys, beam_width=10) == plain  # the acoustic count is what it was
    hyps, scores, am, _ = tr.engine.ctc_beam_lm(np.concatenate(xs), [len(x) for x in xs], lm, beam_width=10, top_paths=2)
    assert with_lm[0] == sum(levenshtein(h[0], np.asarray(y).astype(np.int64)) for h, y in zip(hyps, ys))
    print("toy model after 60 updates: label errors beam %d, beam + model %d of %d" % (plain[0], with_lm[0], with_lm[1]))
    tr.save_model(str(tmp_path / "model"))
    tr.close()
    dec = Decoder(dnn, F, maxlen)
    dec.restore(str(tmp_path / "model"))
    got, got_scores, got_am = dec.ctc_beam_search_lm(xs, lm, beam_width=10, top_paths=2)
    assert got_scores.tobytes() == scores.tobytes() and got_am.tobytes() == am.tobytes()
    assert all(np.array_equal(a, b) for x, y in zip(got, hyps) for a, b in zip(x, y))
    assert all(isinstance(coder.decode(h[0]), str) for h in got)
    assert dec.ctc_beam_search_lm([], lm)[0] == []
    dec.close()


def _dp_lm():
    return _random_lm(np.random.default_rng(77), KW["output_dim"], 3)


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
    eng, _ = pair(np.random.default_rng(5), max_frames=256, torch_state=True, **KW)
    got = dp.label_errors(eng, [CtcMicroBatch(*mb) for mb in _dp_data(num_mb, 3)], beam_width=10, lm=_dp_lm())
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(got, dtype=np.int64))
    eng.close()
    dist.destroy_process_group()


def test_lm_label_errors_two_ranks_equal_single_process(gpu, tmp_path):
    import torch.multiprocessing as mp
    from tfkaldi_amd.dataparallel import CtcMicroBatch, DataParallel
    world, num_mb = 2, 3
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_worker, args=(world, port, num_mb, str(tmp_path)), nprocs=world, join=True)
    eng, _ = make_pair(np.random.default_rng(5), max_frames=256, **KW)
    mbs = [CtcMicroBatch(*mb) for mb in _dp_data(num_mb, 3)]
    want = DataParallel().label_errors(eng, mbs, beam_width=10, lm=_dp_lm())
    plain = DataParallel().label_errors(eng, mbs, beam_width=10)
    eng.close()
    assert want[0] > 0 and want[1] > 0 and want != plain
    for rank in range(world):
        assert tuple(np.load(os.path.join(str(tmp_path), "rank%d.npy" % rank)).tolist()) == want
