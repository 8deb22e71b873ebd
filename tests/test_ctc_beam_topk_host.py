"""CTC prefix beam search with per-frame label pruning, CPU tier: the numpy restatement the GPU tests check the engine
against (the search stated in include/tfkaldi_hip.h at tfk_ctc_beam_topk), with and without a language model; pinned by its
identity with the unpruned restatements, by a CONSTRAINED exhaustive enumeration (only the alignments the pruned search may
sum), and by known answers on integer logits; NgramLM's size check; and label_errors(label_topk=) over a numpy stand-in
engine."""
import itertools
import os
import sys

import numpy as np
import pytest

from test_ctc_beam_host import (NumpyBeamEngine, _microbatches, _Trie, enumerate_labellings, enumeration_cases, log_softmax,
                                peaky_logits, prefix_beam_search)
from test_ctc_beam_lm_host import NumpyBeamLmEngine, _stand_in_lm, enumeration_lm, prefix_beam_search_lm
from test_ctc_decode_host import levenshtein

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM  # noqa: E402


def kept_labels(z, K):
    """keep [T, O - 1] bool: the K labels (never the blank) with the largest logits of every row, the lower class among equals"""
    z = np.asarray(z)
    T, O = z.shape
    keep = np.zeros((T, O - 1), dtype=bool)
    for t in range(T):
        keep[t, np.argsort(-z[t, :O - 1], kind="stable")[:K]] = True
    return keep


def _beam_one_topk(lp, keep, W, lm, dtype):
    """one utterance: test_ctc_beam_lm_host._beam_one_lm (lm None: g = 0 throughout, which is test_ctc_beam_host._beam_one)
    with the extensions by a label outside keep[t] taken out: their value is -inf and they are no candidates.  Returns
    [(labels, combined, acoustic)] of the final beam, best combined first (then shorter, then lexicographically smaller)."""
    T, O = lp.shape
    blank = O - 1
    ninf = dtype(-np.inf)
    C = lm.num_contexts if lm else 1
    if lm:
        w, bonus = dtype(lm.weight), dtype(lm.label_bonus)
        table = lm.table.astype(dtype)
    trie = _Trie()
    ids = [0]
    pb, pnb = np.zeros(1, dtype), np.full(1, ninf, dtype)
    g, ctx = np.zeros(1, dtype), np.array([C - 1], dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            row = lp[t]
            nb = len(ids)
            tot = np.logaddexp(pb, pnb)
            last = np.array([trie.label[q] for q in ids])
            has = last >= 0
            base = np.repeat(tot[:, None], O - 1, axis=1)
            base[has, last[has]] = pb[has]
            ext = base + row[None, :blank]
            ext[:, ~keep[t]] = ninf  # a label that is not kept starts nothing at this frame
            stay_pb = tot + row[blank]
            stay_pnb = np.where(has, pnb + row[np.where(has, last, 0)], ninf).astype(dtype)  # the TRUE lp[last]
            alive = np.ones((nb, O), dtype=bool)
            alive[:, :blank] = keep[t][None, :]
            slot = {q: i for i, q in enumerate(ids)}
            for j, q in enumerate(ids):
                i = slot.get(trie.parent[q]) if q else None
                if i is not None:
                    stay_pnb[j] = np.logaddexp(stay_pnb[j], ext[i, last[j]])
                    alive[i, last[j]] = False
            cand = np.concatenate([ext, np.logaddexp(stay_pb, stay_pnb)[:, None]], axis=1)
            if lm:
                g_ext = ((g[:, None] + w * table[ctx, :blank]).astype(dtype) + bonus).astype(dtype)
                g_cand = np.concatenate([g_ext, g[:, None]], axis=1)
                key = (cand + g_cand).astype(dtype)
            else:
                key = cand
            ii, cc = np.nonzero(alive)
            sc = key[ii, cc]
            if sc.size > W:
                thr = np.partition(sc, sc.size - W)[sc.size - W]
                sure = np.nonzero(sc > thr)[0]
                tied = np.nonzero(sc == thr)[0]
                if sure.size + tied.size > W:
                    seq = lambda k: trie.labels(ids[ii[k]]) + (() if cc[k] == blank else (int(cc[k]),))
                    tied = np.array(sorted(tied, key=lambda k: (len(seq(k)), seq(k)))[:W - sure.size], dtype=np.int64)
                sel = np.sort(np.concatenate([sure, tied]))
                if sel.size < W:
                    rest = np.setdiff1d(np.arange(sc.size), sel)[:W - sel.size]
                    sel = np.sort(np.concatenate([sel, rest]))
                ii, cc = ii[sel], cc[sel]
            stay = cc == blank
            new_ids = [ids[i] if s else trie.extend(ids[i], int(c)) for i, c, s in zip(ii, cc, stay)]
            new_pb = np.where(stay, stay_pb[ii], ninf).astype(dtype)
            new_pnb = np.where(stay, stay_pnb[ii], ext[ii, np.where(stay, 0, cc)]).astype(dtype)
            if lm:
                g = g_cand[ii, cc].astype(dtype)
                ctx = np.where(stay, ctx[ii], (ctx[ii] * O + cc) % C)
            else:
                g, ctx = np.zeros(len(new_ids), dtype), np.zeros(len(new_ids), dtype=np.int64)
            ids, pb, pnb = new_ids, new_pb, new_pnb
        tot = np.logaddexp(pb, pnb)
        comb = tot
        if lm:
            comb = (tot + g).astype(dtype)
            if lm.end_of_sequence:
                comb = (comb + w * table[ctx, blank]).astype(dtype)
    final = [(trie.labels(q), float(s), float(a)) for q, s, a in zip(ids, comb, tot)]
    final.sort(key=lambda e: (-e[1], len(e[0]), e[0]))
    return final


def prefix_beam_search_topk(logits, utt_lens, W, top_paths, label_topk, lm=None, dtype=np.float64):
    """numpy restatement of tfk_ctc_beam_topk on logits [sum(utt_lens), O]: (hyps, scores, am_scores) as
    prefix_beam_search_lm; without lm the two score arrays are equal.  The kept labels come from the logits as given."""
    logits = np.asarray(logits)
    U, O = len(utt_lens), logits.shape[1]
    K = min(int(label_topk), O - 1)
    hyps, scores, am, t0 = [], np.full((U, top_paths), -np.inf), np.full((U, top_paths), -np.inf), 0
    for u, n in enumerate(utt_lens):
        z = logits[t0:t0 + n]
        final = _beam_one_topk(log_softmax(z.astype(dtype)), kept_labels(z, K), W, lm, dtype)[:top_paths]
        t0 += n
        hyps.append([np.array(h, dtype=np.int32) for h, _, _ in final] + [np.zeros(0, np.int32)] * (top_paths - len(final)))
        scores[u, :len(final)] = [s for _, s, _ in final]
        am[u, :len(final)] = [a for _, _, a in final]
    return hyps, scores, am


def enumerate_labellings_topk(logits, K):
    """{labelling: log-probability} over the alignments the pruned search may sum: every frame that BEGINS a label
    occurrence (its class is a label and differs from the previous frame's class) has that label among its kept ones"""
    logits = np.asarray(logits, dtype=np.float64)
    lp = log_softmax(logits)
    keep = kept_labels(logits, K)
    T, O = lp.shape
    acc = {}
    for path in itertools.product(range(O), repeat=T):
        begins = [(t, k) for t, (k, prev) in enumerate(zip(path, (-1,) + path[:-1])) if k != O - 1 and k != prev]
        if all(keep[t, k] for t, k in begins):
            acc.setdefault(tuple(k for _, k in begins), []).append(sum(lp[t, k] for t, k in enumerate(path)))
    return {lab: float(np.logaddexp.reduce(np.array(v))) for lab, v in acc.items()}


def _lists(hyps):
    return [[h.tolist() for h in u] for u in hyps]


# the known-answer rows on integer logits (shared with the GPU tier): (logits [T, O], label_topk, best path, why)
def known_answer_rows():
    O = 6  # labels 0..4, blank 5
    rows = []
    # a tie that K cuts through: labels 1 and 3 tie at the top of the only frame, K = 1 keeps the lower class.  (1) and (3)
    # would tie; with label 3 pruned, (3) is not even a candidate
    z = np.zeros((1, O), np.float32)
    z[0, [1, 3]] = 8.0
    rows.append((z, 1, [1], [[1], []]))
    # the same with K = 2: both are kept
    rows.append((z.copy(), 2, [1], None))
    # a prefix whose last label is pruned at the next frame still collects pnb + lp[last]: frame 0 emits 2; at frame 1 the
    # labels 0 and 2 tie at the top and K = 1 keeps 0, the lower class.  (2) = 2 2 + 2 blank must still beat (2, 0) = 2 0,
    # by the blank's share; without the true lp[2] at frame 1 it would fall far behind
    z = np.zeros((2, O), np.float32)
    z[0, 2] = 12.0
    z[1, [0, 2]] = 6.0
    z[1, 5] = 2.0
    rows.append((z, 1, [2], [[2], [2, 0]]))
    return rows


@pytest.mark.parametrize("O", [9, 36, 64])
def test_unpruned_topk_is_the_existing_restatements(O):
    rng = np.random.default_rng(O)
    lens = [23, 0, 1, 12]
    z = peaky_logits(rng, sum(lens), O, 9)
    lm = NgramLM(log_softmax(1.5 * rng.standard_normal((O, O))), 2, weight=0.7, label_bonus=0.3, end_of_sequence=True)
    for dtype in (np.float64, np.float32):
        for W, P in ((1, 1), (8, 4)):
            for K in (O - 1, 63):
                h0, s0 = prefix_beam_search(z, lens, W, P, dtype=dtype)
                h1, s1, a1 = prefix_beam_search_topk(z, lens, W, P, K, dtype=dtype)
                assert _lists(h0) == _lists(h1) and np.array_equal(s0, s1) and np.array_equal(a1, s1)
                h0, s0, a0 = prefix_beam_search_lm(z, lens, W, P, lm, dtype=dtype)
                h1, s1, a1 = prefix_beam_search_topk(z, lens, W, P, K, lm, dtype=dtype)
                assert _lists(h0) == _lists(h1) and np.array_equal(s0, s1) and np.array_equal(a0, a1)


@pytest.mark.parametrize("with_lm", [False, True])
def test_pruned_beam_equals_the_constrained_enumeration(with_lm):
    """2 labels + blank, T = 6, K = 1, W = 128 (nothing is cut by the beam): the N-best list is the constrained enumeration's"""
    lm = enumeration_lm(2, True) if with_lm else None
    differ, worst, gap = 0, 0.0, np.inf
    for z in enumeration_cases():
        exact = enumerate_labellings_topk(z, 1)
        g = (lambda lab: lm.score(lab)) if lm else (lambda lab: 0.0)
        want = sorted(((lab, s + g(lab)) for lab, s in exact.items()), key=lambda e: (-e[1], len(e[0]), e[0]))
        hyps, scores, am = prefix_beam_search_topk(z, [6], 128, 127, 1, lm)
        n = len(want)
        assert [tuple(h.tolist()) for h in hyps[0][:n]] == [lab for lab, _ in want]
        worst = max(worst, np.abs(scores[0, :n] - np.array([s for _, s in want])).max())
        assert np.abs(am[0, :n] - np.array([exact[lab] for lab, _ in want])).max() <= 1e-12
        assert np.all(scores[0, n:] == -np.inf)
        gap = min(gap, want[0][1] - want[1][1])
        full = enumerate_labellings(z)
        assert all(exact[lab] <= full[lab] + 1e-12 for lab in exact)  # a lower bound of the full probability
        differ += abs(exact[want[0][0]] - full[want[0][0]]) > 1e-9 or want[0][0] != max(
            ((lab, s + g(lab)) for lab, s in full.items()), key=lambda e: e[1])[0]
    print("model %d: worst |restatement - constrained enumeration| %.1e, %d of 40 cases differ from the unpruned answer, "
          "smallest gap best to second %.1e" % (with_lm, worst, differ, gap))
    assert worst <= 1e-12
    assert differ >= 20  # the pin is not vacuous
    assert gap > 1e-3    # (so the GPU version of this test needs no exclusions)


def test_known_answers_on_integer_logits():
    rows = known_answer_rows()
    z, K, best, nbest = rows[0]
    assert kept_labels(z, K)[0].tolist() == [False, True, False, False, False]  # the lower class of the tie
    hyps, scores, _ = prefix_beam_search_topk(z, [1], 8, 3, K)
    assert _lists(hyps)[0][:2] == nbest and scores[0, 2] == -np.inf  # (1), (): label 3 started nothing
    z, K, best, _ = rows[1]
    hyps, scores, _ = prefix_beam_search_topk(z, [1], 8, 3, K)
    assert _lists(hyps)[0] == [[1], [3], []] and scores[0, 0] == scores[0, 1]
    z, K, _, _ = rows[2]
    assert kept_labels(z, K)[1].tolist() == [True, False, False, False, False]
    hyps, scores, _ = prefix_beam_search_topk(z, [2], 8, 2, K)
    lp = log_softmax(z.astype(np.float64))
    assert _lists(hyps)[0][0] == [2]
    # (2) = 2 2 + 2 blank: the first term needs the true lp[2] of frame 1, though 2 is not kept there
    assert abs(scores[0, 0] - (lp[0, 2] + np.logaddexp(lp[1, 2], lp[1, 5]))) <= 1e-12
    assert _lists(hyps)[0][1] == [2, 0] and abs(scores[0, 1] - (lp[0, 2] + lp[1, 0])) <= 1e-12
    assert scores[0, 0] - scores[0, 1] > 1e-2
    # the unpruned search agrees on the best; its score also holds blank 2, which begins a 2 where 2 is not kept
    full = prefix_beam_search(z, [2], 8, 1)[1][0, 0]
    assert abs(full - np.logaddexp(scores[0, 0], lp[0, 5] + lp[1, 2])) <= 1e-12 and full > scores[0, 0]


def wide_logits(O, U=8, Tn=60):
    """the peaky logits of the wide parity shapes (shared with the GPU tier): U utterances of Tn frames, 8 labels each"""
    return peaky_logits(np.random.default_rng(O), U * Tn, O, U * 8), [Tn] * U


def test_pruning_changes_the_best_path_on_wide_alphabets():
    """the shapes at which the GPU tier asserts that K is honoured"""
    for O, K, W in ((200, 16, 32), (1000, 8, 16)):
        z, lens = wide_logits(O)
        hp = prefix_beam_search_topk(z, lens, W, 1, K)[0]
        hf = prefix_beam_search(z, lens, W, 1)[0]
        assert _lists(hp) != _lists(hf)


def test_ngram_lm_refuses_a_table_the_device_does_not_take():
    class Huge(NgramLM):
        def __init__(self, O, order):  # (only the shape: nobody allocates 4 GB here)
            self.num_classes, self.order = O, order
    with pytest.raises(ValueError, match="entries"):
        Huge(1000, 3).check(1000)
    with pytest.raises(ValueError, match="entries"):
        Huge(65536, 2).check(65536)
    Huge(8192, 2).check(8192)
    Huge(400, 3).check(400)
    Huge(64, 4).check(64)


# ---- label_errors(beam_width=, label_topk=) over a numpy stand-in engine ----
class NumpyBeamTopkEngine(NumpyBeamLmEngine):
    def ctc_beam(self, X, utt_lens, beam_width=100, top_paths=1, labels=None, label_lens=None, label_topk=None):
        if label_topk is None:
            return NumpyBeamLmEngine.ctc_beam(self, X, utt_lens, beam_width, top_paths, labels, label_lens)
        self.calls.append("topk%d/%d" % (beam_width, label_topk))
        hyps, scores, _ = prefix_beam_search_topk(np.asarray(X, dtype=np.float32) @ self.W, utt_lens, beam_width, top_paths,
                                                  label_topk)
        return hyps, scores.astype(np.float32), self._edits([h[0] for h in hyps], labels, label_lens)

    def ctc_beam_raw(self, raw, utt_lens, context_width, cmvn=None, beam_width=100, top_paths=1, labels=None,
                     label_lens=None, label_topk=None):
        assert context_width == 0 and cmvn is None
        return self.ctc_beam(raw, utt_lens, beam_width, top_paths, labels, label_lens, label_topk)

    def ctc_beam_lm(self, X, utt_lens, lm, beam_width=100, top_paths=1, labels=None, label_lens=None, label_topk=None):
        if label_topk is None:
            return NumpyBeamLmEngine.ctc_beam_lm(self, X, utt_lens, lm, beam_width, top_paths, labels, label_lens)
        self.calls.append("lmtopk%d/%d" % (beam_width, label_topk))
        hyps, scores, am = prefix_beam_search_topk(np.asarray(X, dtype=np.float32) @ self.W, utt_lens, beam_width, top_paths,
                                                   label_topk, lm)
        return hyps, scores.astype(np.float32), am.astype(np.float32), self._edits([h[0] for h in hyps], labels, label_lens)

    def ctc_beam_lm_raw(self, raw, utt_lens, context_width, lm, cmvn=None, beam_width=100, top_paths=1, labels=None,
                        label_lens=None, label_topk=None):
        assert context_width == 0 and cmvn is None
        return self.ctc_beam_lm(raw, utt_lens, lm, beam_width, top_paths, labels, label_lens, label_topk)


def test_label_errors_carry_label_topk_through():
    from tfkaldi_amd.dataparallel import DataParallel
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    lm = _stand_in_lm()
    mbs = _microbatches(4)
    eng = NumpyBeamTopkEngine()

    def want(K, model):
        edits = labels = 0
        for mb in mbs:
            z = np.asarray(mb.X, dtype=np.float32) @ eng.W
            hyps = prefix_beam_search_topk(z, mb.utt_lens, 8, 1, K, model)[0]
            refs = np.split(np.asarray(mb.labels), np.cumsum(mb.label_lens)[:-1])
            edits += sum(levenshtein(h[0], r) for h, r in zip(hyps, refs))
            labels += int(mb.label_lens.sum())
        return edits, labels

    got = DataParallel().label_errors(eng, mbs, beam_width=8, label_topk=1)
    assert eng.calls == ["topk8/1"] * 4 and got == want(1, None)
    got_lm = DataParallel().label_errors(eng, mbs, beam_width=8, lm=lm, label_topk=1)
    assert eng.calls[-4:] == ["lmtopk8/1"] * 4 and got_lm == want(1, lm)
    full = DataParallel().label_errors(eng, mbs, beam_width=8)
    assert eng.calls[-4:] == ["beam8"] * 4
    assert got != full  # K = 1 of 4 labels is not a bystander here
    assert DataParallel().label_errors(eng, mbs, beam_width=8, label_topk=4) == full  # K = O - 1: the unpruned search

    class _T(object):
        dp, engine = DataParallel(), NumpyBeamTopkEngine()
        _microbatches = staticmethod(lambda inputs, targets: mbs)
    assert CTCTrainer.label_errors(_T(), object(), object(), beam_width=8, label_topk=1) == got
    assert CTCTrainer.label_errors(_T(), object(), object(), beam_width=8, lm=lm, label_topk=1) == got_lm
    with pytest.raises(ValueError, match="beam_width"):
        CTCTrainer.label_errors(_T(), object(), object(), label_topk=4)
    with pytest.raises(ValueError, match="beam_width"):
        DataParallel().label_errors(eng, mbs, label_topk=4)
    # an engine that does not know the keyword keeps serving every call that does not give it
    old = NumpyBeamEngine()
    assert DataParallel().label_errors(old, mbs, beam_width=8) == full


def test_decoder_forwards_label_topk_only_when_given():
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    seen = []

    class _E(object):
        def ctc_beam(self, frames, lens, **kw):
            seen.append(("beam", kw))
            return [], np.zeros((0, 1), np.float32), None

        def ctc_beam_lm(self, frames, lens, lm, **kw):
            seen.append(("lm", kw))
            return [], None, None, None
    d = Decoder.__new__(Decoder)
    d.engine, d.max_length = _E(), 100
    utts = [np.zeros((3, 4), np.float32)]
    d.ctc_beam_search(utts, beam_width=4)
    d.ctc_beam_search(utts, beam_width=4, label_topk=7)
    d.ctc_beam_search_lm(utts, object(), beam_width=4)
    d.ctc_beam_search_lm(utts, object(), beam_width=4, label_topk=7)
    assert [("label_topk" in kw, kw.get("label_topk")) for _, kw in seen] == [(False, None), (True, 7), (False, None), (True, 7)]


def test_peaky_wide_logits_have_clear_winners():
    """the condition the GPU parity tests assert before they consult the device, at two of their shapes"""
    for O, K, W in ((200, 16, 32), (1000, 8, 16)):
        z, lens = wide_logits(O)
        _, s64, _ = prefix_beam_search_topk(z, lens, W, 4, K)
        _, s32, _ = prefix_beam_search_topk(z, lens, W, 1, K, dtype=np.float32)
        tol = np.maximum(4 * np.abs(s32[:, 0] - s64[:, 0]).max(), 1e-6 * np.abs(s64[:, 0]))
        crowded = sum(int((s64[u] >= s64[u, 0] - 2 * tol[u]).sum() > 1) for u in range(8))
        assert 4 * crowded <= 8, (tol, s64)
