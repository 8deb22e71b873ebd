"""CTC N-best rescoring without a GPU: the numpy restatement of tfk_ctc_score (the forward recursion of the CTC loss as the
kernel runs it: fp32 emissions z - logsumexp(z), the state vector re-centred on its maximum every 8 frames with the sum of
the shifts in double), pinned against ctc_log_prob and against exhaustive enumeration; decoder.ctc_rerank; and
label_errors(rescore_paths=N) against a numpy stand-in engine."""
import os
import sys

import numpy as np
import pytest

from test_ctc_beam_host import (NumpyBeamEngine, _microbatches, ctc_log_prob, enumerate_labellings, enumeration_cases,
                                log_softmax, prefix_beam_search)
from test_ctc_beam_lm_host import NumpyBeamLmEngine, _stand_in_lm
from test_ctc_decode_host import levenshtein

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM  # noqa: E402
from tfkaldi_amd.neuralNetworks.decoder import ctc_rerank  # noqa: E402


def ctc_score_restated(logits, labels, dtype=np.float64, recentre=8):
    """numpy restatement of tfk_ctc_score for ONE pair: log p(labels | logits [T, O]) by the forward recursion in `dtype`.
    Emissions lp = z - logsumexp(z) in dtype; after every `recentre`-th step the state vector's maximum moves into an
    offset kept in float64, as the kernel does.  -inf for a pair too short for its labels; T == 0: 0 if S == 0 else -inf."""
    z = np.asarray(logits).astype(dtype)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    T, O = z.shape
    if T == 0:
        return 0.0 if labels.size == 0 else -np.inf
    mx = z.max(axis=1)
    lse = (mx + np.log(np.exp(z - mx[:, None]).sum(axis=1, dtype=dtype))).astype(dtype)
    ext = np.full(2 * labels.size + 1, O - 1, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(ext.size, dtype=bool)
    skip[2:] = (ext[2:] != O - 1) & (ext[2:] != ext[:-2])
    ninf = dtype(-np.inf)
    a = np.full(ext.size, ninf, dtype=dtype)
    a[:2] = z[0, ext[:2]] - lse[0]
    off = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            s1 = np.concatenate([[ninf], a[:-1]]).astype(dtype)
            s2 = np.where(skip, np.concatenate([[ninf, ninf], a[:-2]])[:a.size], ninf).astype(dtype)
            a = (np.logaddexp(np.logaddexp(a, s1), s2) + (z[t, ext] - lse[t])).astype(dtype)
            if t % recentre == 0 and a.max() > -np.inf:
                m = a.max()
                off += float(m)
                a = (a - m).astype(dtype)
    end = np.logaddexp(a[-1], a[-2]) if ext.size > 1 else a[-1]
    return off + float(end) if end > -np.inf else -np.inf


def rescore_tol(zs, hyps):
    """(float64 scores, tol) for pairs (logits, labels): tol = 4 x the largest |float32 run - float64 run| of the
    restatement over the finite pairs, floored at 1e-6 x |score| -- computed from the restatement alone"""
    s64 = np.array([ctc_score_restated(z, h) for z, h in zip(zs, hyps)], dtype=np.float64).reshape(-1)
    s32 = np.array([ctc_score_restated(z, h, np.float32) for z, h in zip(zs, hyps)], dtype=np.float64).reshape(-1)
    finite = np.isfinite(s64)
    assert np.array_equal(finite, np.isfinite(s32))
    diff = np.abs(s32[finite] - s64[finite]).max() if finite.any() else 0.0
    return s64, np.maximum(4.0 * diff, 1e-6 * np.abs(np.where(finite, s64, 0.0)))


def _random_pairs(rng, count=40):
    out = []
    for _ in range(count):
        T, O = int(rng.integers(0, 40)), int(rng.integers(2, 8))
        S = int(rng.integers(0, 12))
        lab = rng.integers(0, O - 1, size=S)
        if S >= 4:
            lab[2] = lab[3]
        out.append((2.0 * rng.standard_normal((T, O)), lab))
    return out


def test_float64_restatement_equals_ctc_log_prob():
    rng = np.random.default_rng(1400)
    finite = 0
    for z, lab in _random_pairs(rng):
        want, got = ctc_log_prob(z, lab), ctc_score_restated(z, lab)
        if want == -np.inf:
            assert got == -np.inf
            continue
        finite += 1
        assert abs(got - want) <= 1e-11 * max(1.0, abs(want)), (z.shape, lab, got, want)
    assert finite >= 15
    z = 2.0 * rng.standard_normal((300, 9))  # a long utterance: many re-centrings
    lab = rng.integers(0, 8, size=60)
    assert abs(ctc_score_restated(z, lab) - ctc_log_prob(z, lab)) <= 1e-9
    assert ctc_score_restated(np.zeros((2, 3)), [0, 0]) == -np.inf  # too short: a a needs three frames
    assert ctc_score_restated(np.zeros((3, 3)), [0, 0]) > -np.inf   # exactly feasible
    assert ctc_score_restated(np.zeros((0, 3)), []) == 0.0 and ctc_score_restated(np.zeros((0, 3)), [1]) == -np.inf


@pytest.mark.parametrize("dtype,bound", [(np.float64, 1e-12), (np.float32, 4e-5)])
def test_restatement_equals_exhaustive_enumeration(dtype, bound):
    """T = 6, 2 labels + blank: every labelling's probability by summing all 3^6 alignments; the labellings sum to one.
    (float32 bound: values below 64 in magnitude round by at most half an ulp = 1.9e-6 per operation, three rounded
    operations per frame, six frames and the end: 4e-5)"""
    for z in enumeration_cases(count=12):
        want = enumerate_labellings(z)
        got = {lab: ctc_score_restated(z.astype(np.float32) if dtype is np.float32 else z, lab, dtype) for lab in want}
        ref = want if dtype is np.float64 else enumerate_labellings(z.astype(np.float32))
        assert max(abs(got[lab] - ref[lab]) for lab in want) <= bound
        if dtype is np.float64:
            assert abs(np.logaddexp.reduce(np.array(list(got.values())))) <= 1e-12
    # (0, 0, 1, 1) needs 4 labels + 2 separating blanks = 6 frames: in the enumeration; (0, 0, 0, 0) needs 7: not
    z = enumeration_cases(count=1)[0]
    assert (0, 0, 1, 1) in enumerate_labellings(z) and ctc_score_restated(z, (0, 0, 0, 0)) == -np.inf


def test_float32_restatement_is_close():
    rng = np.random.default_rng(1401)
    pairs = [p for p in _random_pairs(rng, 30) if ctc_log_prob(*p) > -np.inf]
    s64, tol = rescore_tol([z.astype(np.float32) for z, _ in pairs], [lab for _, lab in pairs])
    assert np.all(tol < 1e-3) and np.all(tol > 0)


# ---- ctc_rerank ----
def _lm(eos=False, weight=0.7, bonus=0.3):
    rng = np.random.default_rng(77)
    table = np.log(rng.dirichlet(np.ones(4), size=4)).astype(np.float32)  # order 2 over 3 labels + blank
    return NgramLM(table, 2, weight=weight, label_bonus=bonus, end_of_sequence=eos)


def test_rerank_known_answers():
    hyps = [np.array([0, 1]), np.array([2]), np.zeros(0, np.int32), np.array([1, 1, 1])]
    order, scores, post = ctc_rerank(hyps, [-3.0, -1.0, -2.0, -8.0])
    assert order.tolist() == [1, 2, 0, 3] and scores.tolist() == [-1.0, -2.0, -3.0, -8.0] and scores.dtype == np.float64
    want = np.exp(np.array([-1.0, -2.0, -3.0, -8.0]))
    assert np.allclose(post, want / want.sum(), rtol=1e-14) and abs(post.sum() - 1.0) <= 1e-15
    # float32 input is widened before anything is added
    order, scores, _ = ctc_rerank(hyps, np.array([-3.0, -1.0, -2.0, -8.0], np.float32))
    assert scores.dtype == np.float64 and order.tolist() == [1, 2, 0, 3]
    order, scores, post = ctc_rerank([], [])
    assert order.size == 0 and scores.size == 0 and post.size == 0
    with pytest.raises(ValueError):
        ctc_rerank(hyps, [-1.0, -2.0])
    with pytest.raises(ValueError):
        ctc_rerank(hyps[:1], [np.nan])


def test_rerank_is_stable_on_ties():
    hyps = [np.array([k]) for k in range(5)]
    order, scores, post = ctc_rerank(hyps, [-2.0, -1.0, -2.0, -1.0, -2.0])
    assert order.tolist() == [1, 3, 0, 2, 4]  # ties keep the beam's order
    assert abs(post.sum() - 1.0) <= 1e-15 and post[0] == post[1] and post[2] == post[3] == post[4]
    assert ctc_rerank(hyps, [-1.0] * 5)[0].tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("eos", [False, True])
def test_rerank_adds_the_models_score(eos):
    lm = _lm(eos)
    rng = np.random.default_rng(5)
    hyps = [rng.integers(0, 3, size=n).astype(np.int32) for n in (0, 1, 4, 2, 7, 3)]
    am = -10.0 * rng.random(len(hyps))
    order, scores, post = ctc_rerank(hyps, am, lm)
    combined = np.array([a + lm.score(h) for a, h in zip(am, hyps)])
    assert sorted(order.tolist()) == list(range(len(hyps)))
    assert np.array_equal(scores, combined[order]) and np.all(np.diff(scores) <= 0)
    assert abs(post.sum() - 1.0) <= 1e-14
    assert np.allclose(post, np.exp(scores - np.logaddexp.reduce(scores)), rtol=1e-13)
    if eos:  # the end term is in: it differs from the ranking without it
        plain = NgramLM(lm.table, 2, weight=lm.weight, label_bonus=lm.label_bonus)
        assert not np.array_equal(ctc_rerank(hyps, am, plain)[1], scores)
        ctx = lm.context(hyps[2])
        assert abs(lm.score(hyps[2]) - plain.score(hyps[2]) - lm.weight * float(lm.table[ctx, 3])) <= 1e-15
    # the model can change the winner
    two = [np.array([0, 0, 0, 0, 0, 0]), np.array([1])]
    heavy = NgramLM(lm.table, 2, weight=5.0)
    assert ctc_rerank(two, [-1.0, -1.5])[0][0] == 0 and ctc_rerank(two, [-1.0, -1.5], heavy)[0][0] == 1


def test_rerank_minus_infinity_sorts_last_with_posterior_zero():
    hyps = [np.array([0]), np.array([1]), np.array([2])]
    order, scores, post = ctc_rerank(hyps, [-np.inf, -4.0, -3.0], _lm())
    assert order[-1] == 0 and scores[-1] == -np.inf and post[-1] == 0.0 and abs(post.sum() - 1.0) <= 1e-15
    order, scores, post = ctc_rerank(hyps, [-np.inf] * 3)
    assert order.tolist() == [0, 1, 2] and np.all(post == 0.0) and not np.any(np.isnan(post))


# ---- label_errors(rescore_paths=N) against a numpy stand-in engine ----
class NumpyScoreEngine(NumpyBeamLmEngine):
    """NumpyBeamEngine + ctc_score: the float64 restatement on logits = X @ W, edits by levenshtein"""

    def ctc_beam(self, X, utt_lens, beam_width=100, top_paths=1, labels=None, label_lens=None):
        if labels is not None:
            return NumpyBeamLmEngine.ctc_beam(self, X, utt_lens, beam_width, top_paths, labels, label_lens)
        self.calls.append("beam%d/%d" % (beam_width, top_paths))
        hyps, scores = prefix_beam_search(np.asarray(X, dtype=np.float32) @ self.W, utt_lens, beam_width, top_paths)
        return hyps, scores.astype(np.float32), None

    def ctc_beam_lm(self, X, utt_lens, lm, beam_width=100, top_paths=1, labels=None, label_lens=None):
        if labels is None:  # (the parent computes edits: give it empty references and drop them)
            labels, label_lens = np.zeros(0, np.int32), np.zeros(len(utt_lens), np.int32)
            return NumpyBeamLmEngine.ctc_beam_lm(self, X, utt_lens, lm, beam_width, top_paths, labels, label_lens)[:3] + (None,)
        return NumpyBeamLmEngine.ctc_beam_lm(self, X, utt_lens, lm, beam_width, top_paths, labels, label_lens)

    def ctc_score(self, X, utt_lens, hyp_counts, labels, label_lens, ref_labels=None, ref_lens=None):
        self.calls.append("score%d" % int(np.sum(hyp_counts)))
        zs = np.split(np.asarray(X, dtype=np.float32) @ self.W, np.cumsum(utt_lens)[:-1])
        hyps = np.split(np.asarray(labels), np.cumsum(label_lens)[:-1]) if len(label_lens) else []
        refs = np.split(np.asarray(ref_labels), np.cumsum(ref_lens)[:-1])
        utt = np.repeat(np.arange(len(utt_lens)), hyp_counts)
        score = np.array([ctc_score_restated(zs[u], h) for h, u in zip(hyps, utt)], dtype=np.float32)
        edits = np.array([levenshtein(h, refs[u]) for h, u in zip(hyps, utt)], dtype=np.int32)
        cuts = np.cumsum(hyp_counts)[:-1]
        return np.split(score, cuts), np.split(edits, cuts)

    def ctc_score_raw(self, raw, utt_lens, context_width, hyp_counts, labels, label_lens, ref_labels=None, ref_lens=None,
                      cmvn=None):
        assert context_width == 0 and cmvn is None
        return self.ctc_score(raw, utt_lens, hyp_counts, labels, label_lens, ref_labels, ref_lens)


def _want_rescored(eng, mbs, W, N, lm=None):
    """the restatement's count: N-best by the numpy search, exact float64 scores (as float32, what the entry returns),
    ctc_rerank, the edits of the new best"""
    edits = total = moved = 0
    for mb in mbs:
        z = np.asarray(mb.X, dtype=np.float32) @ eng.W
        if lm is None:
            hyps, scores = prefix_beam_search(z, mb.utt_lens, W, N)
        else:
            from test_ctc_beam_lm_host import prefix_beam_search_lm
            hyps, scores = prefix_beam_search_lm(z, mb.utt_lens, W, N, lm)[:2]
        zs = np.split(z, np.cumsum(mb.utt_lens)[:-1])
        refs = np.split(mb.labels, np.cumsum(mb.label_lens)[:-1])
        for u in range(len(mb.utt_lens)):
            kept = [h for h, s in zip(hyps[u], scores[u]) if s > -np.inf]
            exact = np.array([ctc_score_restated(zs[u], h) for h in kept], dtype=np.float32)
            best = ctc_rerank(kept, exact, lm)[0][0]
            moved += int(best != 0)
            edits += levenshtein(kept[best], refs[u])
            total += len(refs[u])
    return (edits, total), moved


def test_label_errors_rescored_are_the_restatements_edits_of_the_reranked_best():
    from tfkaldi_amd.dataparallel import DataParallel
    mbs = _microbatches(4, seed=7)
    eng = NumpyScoreEngine()
    got = DataParallel().label_errors(eng, mbs, beam_width=2, rescore_paths=2)
    want, moved = _want_rescored(eng, mbs, 2, 2)
    assert got == want and all(type(v) is int for v in got) and got[0] > 0
    assert moved >= 1  # the re-ranking does change a winner on these inputs
    assert [c for c in eng.calls if c.startswith("beam")] == ["beam2/2"] * 4 and sum(c.startswith("score") for c in eng.calls) == 4
    # rescore_paths = 1 re-ranks a list of one: the beam's own best path
    assert DataParallel().label_errors(NumpyScoreEngine(), mbs, beam_width=3, rescore_paths=1) == \
        DataParallel().label_errors(NumpyBeamEngine(), mbs, beam_width=3)


def test_label_errors_rescored_honour_the_model():
    from tfkaldi_amd.dataparallel import DataParallel
    lm = _stand_in_lm()
    mbs = _microbatches(3, seed=4)
    eng = NumpyScoreEngine()
    got = DataParallel().label_errors(eng, mbs, beam_width=4, lm=lm, rescore_paths=4)
    assert got == _want_rescored(eng, mbs, 4, 4, lm)[0]


def test_rescore_paths_none_is_todays_result_and_needs_a_beam():
    from tfkaldi_amd.dataparallel import DataParallel, _label_errors
    mbs = _microbatches(3)
    for kw in ({}, {"beam_width": 8}):
        eng = NumpyScoreEngine()
        assert DataParallel().label_errors(eng, mbs, rescore_paths=None, **kw) == \
            DataParallel().label_errors(NumpyBeamEngine(), mbs, **kw)
        assert not any(c.startswith("score") for c in eng.calls)
    with pytest.raises(ValueError, match="beam_width"):
        DataParallel().label_errors(NumpyScoreEngine(), mbs, rescore_paths=3)
    with pytest.raises(ValueError, match="beam_width"):
        _label_errors(NumpyScoreEngine(), mbs[0], rescore_paths=3)


def test_engine_side_levenshtein_and_argument_checks():
    """the private numpy Levenshtein of engine.py (what ctc_score reports when there is no frame at all)"""
    from tfkaldi_amd.engine import _levenshtein
    rng = np.random.default_rng(9)
    for _ in range(30):
        a, b = rng.integers(0, 4, size=rng.integers(0, 9)), rng.integers(0, 4, size=rng.integers(0, 9))
        assert _levenshtein(a, b) == levenshtein(a, b)
    assert _levenshtein([], [1, 2]) == 2 and _levenshtein([1, 2, 3], []) == 3 and _levenshtein([], []) == 0
