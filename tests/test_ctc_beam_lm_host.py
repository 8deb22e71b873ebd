"""CTC prefix beam search with a character n-gram language model, CPU tier: the numpy restatement the GPU tests check the
engine against (the search stated in include/tfkaldi_hip.h at tfk_ctc_beam_lm), pinned by exhaustive enumeration, by the
identity with the acoustic-only restatement and by a known answer; the NgramLM class; and Trainer.label_errors(beam_width=,
lm=) over a numpy stand-in engine."""
import os
import sys

import numpy as np
import pytest

from test_ctc_beam_host import (NumpyBeamEngine, _microbatches, _Trie, enumerate_labellings, enumeration_cases, log_softmax,
                                peaky_logits, prefix_beam_search)
from test_ctc_decode_host import levenshtein

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM  # noqa: E402


def _beam_one_lm(lp, W, lm, dtype):
    """one utterance: test_ctc_beam_host._beam_one with every prefix carrying g (in `dtype`, three roundings per label:
    (g + weight * table[ctx][c]) + bonus) and a context id; candidates are cut by total + g.  Returns [(labels, combined,
    acoustic)] of the final beam, best combined first (then shorter, then lexicographically smaller)."""
    T, O = lp.shape
    blank = O - 1
    C = lm.num_contexts
    ninf = dtype(-np.inf)
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
            stay_pb = tot + row[blank]
            stay_pnb = np.where(has, pnb + row[np.where(has, last, 0)], ninf).astype(dtype)
            alive = np.ones((nb, O), dtype=bool)
            slot = {q: i for i, q in enumerate(ids)}
            for j, q in enumerate(ids):
                i = slot.get(trie.parent[q]) if q else None
                if i is not None:
                    stay_pnb[j] = np.logaddexp(stay_pnb[j], ext[i, last[j]])
                    alive[i, last[j]] = False
            cand = np.concatenate([ext, np.logaddexp(stay_pb, stay_pnb)[:, None]], axis=1)
            g_ext = ((g[:, None] + w * table[ctx, :blank]).astype(dtype) + bonus).astype(dtype)
            g_cand = np.concatenate([g_ext, g[:, None]], axis=1)
            key = (cand + g_cand).astype(dtype)
            ii, cc = np.nonzero(alive)
            sc = key[ii, cc]
            if sc.size > W:
                thr = np.partition(sc, sc.size - W)[sc.size - W]
                sure = np.nonzero(sc > thr)[0]
                tied = np.nonzero(sc == thr)[0]
                if sure.size + tied.size > W:
                    seq = lambda k: trie.labels(ids[ii[k]]) + (() if cc[k] == blank else (int(cc[k]),))
                    tied = np.array(sorted(tied, key=lambda k: (len(seq(k)), seq(k)))[:W - sure.size], dtype=np.int64)
                keep = np.sort(np.concatenate([sure, tied]))
                if keep.size < W:
                    rest = np.setdiff1d(np.arange(sc.size), keep)[:W - keep.size]
                    keep = np.sort(np.concatenate([keep, rest]))
                ii, cc = ii[keep], cc[keep]
            stay = cc == blank
            new_ids = [ids[i] if s else trie.extend(ids[i], int(c)) for i, c, s in zip(ii, cc, stay)]
            new_pb = np.where(stay, stay_pb[ii], ninf).astype(dtype)
            new_pnb = np.where(stay, stay_pnb[ii], ext[ii, np.where(stay, 0, cc)]).astype(dtype)
            new_g = g_cand[ii, cc].astype(dtype)
            new_ctx = np.where(stay, ctx[ii], (ctx[ii] * O + cc) % C)
            ids, pb, pnb, g, ctx = new_ids, new_pb, new_pnb, new_g, new_ctx
        tot = np.logaddexp(pb, pnb)
        comb = (tot + g).astype(dtype)
        if lm.end_of_sequence:
            comb = (comb + w * table[ctx, blank]).astype(dtype)
    final = [(trie.labels(q), float(s), float(a)) for q, s, a in zip(ids, comb, tot)]
    final.sort(key=lambda e: (-e[1], len(e[0]), e[0]))
    return final


def prefix_beam_search_lm(logits, utt_lens, W, top_paths, lm, dtype=np.float64):
    """numpy restatement of tfk_ctc_beam_lm on logits [sum(utt_lens), O]: (hyps, scores, am_scores) with hyps[u][n] int32
    arrays, best combined score first, both score arrays float64 [U, top_paths]; missing paths are empty with -inf."""
    logits = np.asarray(logits)
    U = len(utt_lens)
    hyps, scores, am, t0 = [], np.full((U, top_paths), -np.inf), np.full((U, top_paths), -np.inf), 0
    for u, n in enumerate(utt_lens):
        final = _beam_one_lm(log_softmax(logits[t0:t0 + n].astype(dtype)), W, lm, dtype)[:top_paths]
        t0 += n
        hyps.append([np.array(h, dtype=np.int32) for h, _, _ in final] + [np.zeros(0, np.int32)] * (top_paths - len(final)))
        scores[u, :len(final)] = [s for _, s, _ in final]
        am[u, :len(final)] = [a for _, _, a in final]
    return hyps, scores, am


def enumeration_lm(order, eos, O=3):
    """the table of the exhaustive pin (and of its GPU twin): a random row-normalised one per order"""
    table = log_softmax(1.5 * np.random.default_rng(50 + order).standard_normal((O ** (order - 1), O)))
    return NgramLM(table, order, weight=0.8, label_bonus=0.5, end_of_sequence=eos)


@pytest.mark.parametrize("eos", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_unpruned_beam_equals_exhaustive_enumeration_with_the_model(order, eos):
    """2 labels + blank, T = 6, W = 128 prunes nothing: the N-best list is the enumeration sorted by log p_ctc + model"""
    lm = enumeration_lm(order, eos)
    changed, worst = 0, 0.0
    for z in enumeration_cases():
        exact = enumerate_labellings(z)
        want = sorted(((lab, s + lm.score(lab)) for lab, s in exact.items()), key=lambda e: (-e[1], len(e[0]), e[0]))
        hyps, scores, am = prefix_beam_search_lm(z, [6], 128, 127, lm)
        n = len(want)
        assert [tuple(h.tolist()) for h in hyps[0][:n]] == [lab for lab, _ in want]
        worst = max(worst, np.abs(scores[0, :n] - np.array([s for _, s in want])).max())
        assert np.abs(am[0, :n] - np.array([exact[lab] for lab, _ in want])).max() <= 1e-12
        assert want[0][1] - want[1][1] > 1e-3  # (so the GPU version of this test needs no exclusions)
        changed += want[0][0] != max(exact.items(), key=lambda e: e[1])[0]
    print("order %d eos %d: worst |restatement - enumeration| %.1e, the model changes the best labelling in %d of 40"
          % (order, eos, worst, changed))
    assert worst <= 1e-12
    assert changed >= 5  # the model matters on these inputs


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_weight_is_the_acoustic_search(dtype):
    rng = np.random.default_rng(7)
    lens = [25, 0, 1, 14]
    z = (2.0 * rng.standard_normal((sum(lens), 6))).astype(np.float32)
    for order in (1, 3):
        lm = NgramLM(rng.standard_normal((6 ** (order - 1), 6)), order, weight=0.0, label_bonus=0.0)
        for W, P in ((1, 1), (4, 3), (16, 8)):
            h0, s0 = prefix_beam_search(z, lens, W, P, dtype=dtype)
            h1, s1, a1 = prefix_beam_search_lm(z, lens, W, P, lm, dtype=dtype)
            assert [[h.tolist() for h in u] for u in h0] == [[h.tolist() for h in u] for u in h1]
            assert np.array_equal(s0, s1) and np.array_equal(a1, s1)


def test_known_answer():
    """two frames, p(a) = 0.4, p(blank) = 0.6 each: [a] 0.64 over [] 0.36 by acoustic score; a model that gives a the
    probability 0.5 turns that into 0.32 against 0.36; a bonus of log 2 per label turns it back"""
    z = np.log(np.array([[0.4, 0.6], [0.4, 0.6]]))
    table = np.log(np.array([[0.5, 0.5]]))
    hyps, scores, am = prefix_beam_search_lm(z, [2], 4, 2, NgramLM(table, 1, weight=1.0))
    assert [h.tolist() for h in hyps[0]] == [[], [0]]
    assert np.allclose(np.exp(scores[0]), [0.36, 0.32], rtol=1e-12) and np.allclose(np.exp(am[0]), [0.36, 0.64], rtol=1e-12)
    hyps, scores, am = prefix_beam_search_lm(z, [2], 4, 2, NgramLM(table, 1, weight=1.0, label_bonus=np.log(2.0)))
    assert [h.tolist() for h in hyps[0]] == [[0], []]
    assert np.allclose(np.exp(scores[0]), [0.64, 0.36], rtol=1e-12)
    # the end term: [] ends after the start context, [a] after a (order 2: rows a, start)
    t2 = np.log(np.array([[0.5, 0.5], [0.9, 0.1]]))
    hyps, scores, _ = prefix_beam_search_lm(z, [2, 0], 4, 2, NgramLM(t2, 2, weight=1.0, end_of_sequence=True))
    assert [h.tolist() for h in hyps[0]] == [[0], []]
    assert np.allclose(np.exp(scores[0]), [0.64 * 0.9 * 0.5, 0.36 * 0.1], rtol=1e-12)
    assert hyps[1][0].size == 0 and np.allclose(np.exp(scores[1]), [0.1, 0.0], rtol=1e-12)  # a zero-frame utterance


def test_ngram_lm_contexts_and_scores():
    O = 4  # labels 0..2, blank / start digit 3
    rng = np.random.default_rng(3)
    lm1 = NgramLM(rng.standard_normal((1, O)), 1)
    assert lm1.context([]) == 0 and lm1.context([2, 1, 0]) == 0
    lm2 = NgramLM(rng.standard_normal((O, O)), 2)
    assert lm2.context([]) == 3 and lm2.context([1]) == 1 and lm2.context([1, 2, 0]) == 0
    lm3 = NgramLM(rng.standard_normal((O * O, O)), 3)
    assert lm3.context([]) == 15 and lm3.context([2]) == 3 * O + 2 and lm3.context([2, 1]) == 2 * O + 1
    assert lm3.context([0, 2, 1, 1]) == 1 * O + 1  # older labels fall out
    lm4 = NgramLM(rng.standard_normal((O ** 3, O)), 4, weight=0.5, label_bonus=0.25, end_of_sequence=True)
    assert lm4.context([]) == 63 and lm4.context([1]) == (3 * O + 3) * O + 1 and lm4.context([0, 1, 2, 0, 1]) == (2 * O + 0) * O + 1
    t = lm4.table.astype(np.float64)
    want = 0.5 * (t[63, 1] + t[(3 * O + 3) * O + 1, 2] + t[(3 * O + 1) * O + 2, 2] + t[(1 * O + 2) * O + 2, 0]) + 4 * 0.25
    want += 0.5 * t[(2 * O + 2) * O + 0, 3]
    assert abs(lm4.score([1, 2, 2, 0]) - want) <= 1e-12
    assert abs(lm4.score([]) - 0.5 * t[63, 3]) <= 1e-15
    assert NgramLM(lm4.table, 4).score([]) == 0.0
    with pytest.raises(ValueError):
        lm4.context([3])  # the blank is not a label


def test_ngram_lm_from_label_sequences():
    seqs = [[0, 1, 0], [1], []]
    lm = NgramLM.from_label_sequences(seqs, 2, 2, add_k=1.0)
    O = 3
    assert lm.table.shape == (3, 3) and lm.order == 2
    # rows: after 0, after 1, at the start
    counts = np.array([[0, 1, 1], [1, 0, 1], [1, 1, 1]], dtype=np.float64)
    want = np.log((counts + 1.0) / (counts.sum(1, keepdims=True) + O))
    assert np.allclose(lm.table, want, rtol=1e-6)
    for order in (1, 2, 3, 4):
        lm = NgramLM.from_label_sequences([[0, 1, 1, 2, 0], [2, 2]], 3, order, add_k=0.5, weight=0.3)
        assert lm.table.shape == (4 ** (order - 1), 4) and lm.weight == 0.3
        assert np.allclose(np.exp(lm.table.astype(np.float64)).sum(axis=1), 1.0, atol=1e-6)
    uni = NgramLM.from_label_sequences([[0, 0, 1]], 2, 1, add_k=1.0)
    assert np.allclose(np.exp(uni.table[0]), np.array([3, 2, 2]) / 7.0, rtol=1e-6)
    with pytest.raises(ValueError):
        NgramLM.from_label_sequences([[2]], 2, 2)


def test_ngram_lm_rejects_bad_tables():
    good = np.zeros((9, 3))
    NgramLM(good, 3)
    for table, order in ((good, 2), (np.zeros((3, 3, 3)), 3), (np.zeros((1, 1)), 1), (good, 0), (good, 5)):
        with pytest.raises(ValueError):
            NgramLM(table, order)
    for bad in (np.nan, np.inf, -np.inf):
        t = good.copy()
        t[2, 1] = bad
        with pytest.raises(ValueError, match="entry 7"):
            NgramLM(t, 3)
    with pytest.raises(ValueError):
        NgramLM(good, 3).check(5)


# ---- Trainer.label_errors(beam_width=, lm=) over a numpy stand-in engine ----
class NumpyBeamLmEngine(NumpyBeamEngine):
    def ctc_beam_lm(self, X, utt_lens, lm, beam_width=100, top_paths=1, labels=None, label_lens=None):
        self.calls.append("lm%d" % beam_width)
        hyps, scores, am = prefix_beam_search_lm(np.asarray(X, dtype=np.float32) @ self.W, utt_lens, beam_width, top_paths, lm)
        return hyps, scores.astype(np.float32), am.astype(np.float32), self._edits([h[0] for h in hyps], labels, label_lens)

    def ctc_beam_lm_raw(self, raw, utt_lens, context_width, lm, cmvn=None, beam_width=100, top_paths=1, labels=None,
                        label_lens=None):
        assert context_width == 0 and cmvn is None
        return self.ctc_beam_lm(raw, utt_lens, lm, beam_width, top_paths, labels, label_lens)


def _stand_in_lm():
    rng = np.random.default_rng(21)
    return NgramLM(log_softmax(2.0 * rng.standard_normal((5, 5))), 2, weight=1.5, label_bonus=-0.5, end_of_sequence=True)


def test_label_errors_with_a_model_are_the_restatements_edit_distances():
    from tfkaldi_amd.dataparallel import DataParallel
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    lm = _stand_in_lm()
    mbs = _microbatches(4)
    eng = NumpyBeamLmEngine()
    got = DataParallel().label_errors(eng, mbs, beam_width=8, lm=lm)
    assert eng.calls == ["lm8"] * 4
    want_edits = want_labels = plain_edits = 0
    for mb in mbs:
        z = np.asarray(mb.X, dtype=np.float32) @ eng.W
        hyps = prefix_beam_search_lm(z, mb.utt_lens, 8, 1, lm)[0]
        refs = np.split(np.asarray(mb.labels), np.cumsum(mb.label_lens)[:-1])
        want_edits += sum(levenshtein(h[0], r) for h, r in zip(hyps, refs))
        plain_edits += sum(levenshtein(h[0], r) for h, r in zip(prefix_beam_search(z, mb.utt_lens, 8, 1)[0], refs))
        want_labels += int(mb.label_lens.sum())
    assert got == (want_edits, want_labels) and want_edits > 0
    assert want_edits != plain_edits  # the model is not a bystander here
    # without lm nothing changes: the acoustic entry is called
    assert DataParallel().label_errors(eng, mbs, beam_width=8) == (plain_edits, want_labels)
    assert eng.calls[-4:] == ["beam8"] * 4

    # Trainer.label_errors carries lm through; lm without a beam_width is an error before anything runs
    class _T(object):
        dp, engine = DataParallel(), NumpyBeamLmEngine()
        _microbatches = staticmethod(lambda inputs, targets: mbs)
    assert CTCTrainer.label_errors(_T(), object(), object(), beam_width=8, lm=lm) == got
    assert CTCTrainer.label_errors(_T(), object(), object(), beam_width=8) == (plain_edits, want_labels)
    with pytest.raises(ValueError, match="beam_width"):
        CTCTrainer.label_errors(_T(), object(), object(), lm=lm)
    with pytest.raises(ValueError, match="beam_width"):
        DataParallel().label_errors(eng, mbs, lm=lm)


def test_peaky_logits_with_a_model_have_clear_winners():
    """the condition the GPU parity test at O = 36 asserts before it consults the device (same inputs, same tol)"""
    rng = np.random.default_rng(61)
    lens = [200] * 8
    z = peaky_logits(rng, sum(lens), 36, 8 * 25)
    lm = NgramLM(log_softmax(1.5 * rng.standard_normal((36, 36))), 2, weight=0.6, label_bonus=0.4)
    _, s64, _ = prefix_beam_search_lm(z, lens, 10, 4, lm)
    _, s32, _ = prefix_beam_search_lm(z, lens, 10, 1, lm, dtype=np.float32)
    tol = np.maximum(4 * np.abs(s32[:, 0] - s64[:, 0]).max(), 1e-6 * np.abs(s64[:, 0]))
    crowded = sum(int((s64[u] >= s64[u, 0] - 2 * tol[u]).sum() > 1) for u in range(8))
    assert 4 * crowded <= 8, (tol, s64)
