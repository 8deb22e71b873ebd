"""CTC prefix beam search constrained by a finite-state grammar, CPU tier: the numpy restatement the GPU tests check the
engine against (the search stated in include/tfkaldi_hip.h at tfk_ctc_graph_set), pinned by the identity with the n-gram
restatement, by exhaustive enumeration under a constraint and by a grammar that leaves fewer live candidates than the beam;
and the GraphLM class with its builders."""
import itertools
import os
import sys

import numpy as np
import pytest

from test_ctc_beam_host import _Trie, enumerate_labellings, enumeration_cases, log_softmax
from test_ctc_beam_lm_host import prefix_beam_search_lm
from test_ctc_beam_topk_host import kept_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tfkaldi_amd.neuralNetworks import ctc_lm  # noqa: E402
from tfkaldi_amd.neuralNetworks.ctc_lm import GraphLM, NgramLM  # noqa: E402


def _beam_one_graph(lp, W, lm, dtype, keep=None, live=None):
    """one utterance: test_ctc_beam_lm_host._beam_one_lm over a graph -- an extension exists only where the state has an arc
    (and, with keep [T, O - 1], where the label is kept at the frame: test_ctc_beam_topk_host._beam_one_topk), g is formed
    only there, the new state is read from next, a non-final state ends at -inf under the end flag, and the kept set is
    never padded.  live: a list that receives every frame's number of live candidates.  Returns [(labels, combined,
    acoustic)] of the final beam, best combined first (then shorter, then lexicographically smaller)."""
    T, O = lp.shape
    blank = O - 1
    ninf = dtype(-np.inf)
    w, bonus = dtype(lm.weight), dtype(lm.label_bonus)
    table = lm.table.astype(dtype)
    nxt = lm.next.astype(np.int64)
    trie = _Trie()
    ids = [0]
    pb, pnb = np.zeros(1, dtype), np.full(1, ninf, dtype)
    g, state = np.zeros(1, dtype), np.array([lm.start], dtype=np.int64)
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
            if keep is not None:
                ext[:, ~keep[t]] = ninf  # a label that is not kept starts nothing at this frame
            stay_pb = tot + row[blank]
            stay_pnb = np.where(has, pnb + row[np.where(has, last, 0)], ninf).astype(dtype)
            arc = table[state, :blank] > ninf
            alive = np.ones((nb, O), dtype=bool)
            if keep is not None:
                alive[:, :blank] = keep[t][None, :]
            alive[:, :blank] &= arc
            slot = {q: i for i, q in enumerate(ids)}
            for j, q in enumerate(ids):
                i = slot.get(trie.parent[q]) if q else None
                if i is not None and (keep is None or keep[t][last[j]]):
                    assert arc[i, last[j]]  # (a prefix in the beam got there over an arc)
                    stay_pnb[j] = np.logaddexp(stay_pnb[j], ext[i, last[j]])
                    alive[i, last[j]] = False
            cand = np.concatenate([ext, np.logaddexp(stay_pb, stay_pnb)[:, None]], axis=1)
            arc_w = np.where(arc, table[state, :blank], dtype(0))  # (0 * -inf is NaN: existence comes first)
            g_ext = ((g[:, None] + w * arc_w).astype(dtype) + bonus).astype(dtype)
            g_cand = np.concatenate([g_ext, g[:, None]], axis=1)
            key = (cand + g_cand).astype(dtype)
            ii, cc = np.nonzero(alive)
            if live is not None:
                live.append(int(ii.size))
            sc = key[ii, cc]
            if sc.size > W:
                thr = np.partition(sc, sc.size - W)[sc.size - W]
                sure = np.nonzero(sc > thr)[0]
                tied = np.nonzero(sc == thr)[0]
                if sure.size + tied.size > W:
                    seq = lambda k: trie.labels(ids[ii[k]]) + (() if cc[k] == blank else (int(cc[k]),))
                    tied = np.array(sorted(tied, key=lambda k: (len(seq(k)), seq(k)))[:W - sure.size], dtype=np.int64)
                sel = np.sort(np.concatenate([sure, tied]))
                ii, cc = ii[sel], cc[sel]
            stay = cc == blank
            new_ids = [ids[i] if s else trie.extend(ids[i], int(c)) for i, c, s in zip(ii, cc, stay)]
            new_pb = np.where(stay, stay_pb[ii], ninf).astype(dtype)
            new_pnb = np.where(stay, stay_pnb[ii], ext[ii, np.where(stay, 0, cc)]).astype(dtype)
            new_g = g_cand[ii, cc].astype(dtype)
            new_state = np.where(stay, state[ii], nxt[state[ii], np.where(stay, 0, cc)])
            ids, pb, pnb, g, state = new_ids, new_pb, new_pnb, new_g, new_state
        tot = np.logaddexp(pb, pnb)
        comb = (tot + g).astype(dtype)
        if lm.end_of_sequence:
            end = table[state, blank]
            comb = np.where(end > ninf, (comb + w * np.where(end > ninf, end, dtype(0))).astype(dtype), ninf)
    final = [(trie.labels(q), float(s), float(a)) for q, s, a in zip(ids, comb, tot)]
    final.sort(key=lambda e: (-e[1], len(e[0]), e[0]))
    return final


def prefix_beam_search_graph(logits, utt_lens, W, top_paths, lm, dtype=np.float64, label_topk=None, live=None):
    """numpy restatement of the search with a GraphLM on logits [sum(utt_lens), O]: (hyps, scores, am_scores) as
    prefix_beam_search_lm; a listed path whose state is not final has score -inf and a finite am_score; missing paths are
    empty with -inf in both.  label_topk: the pruned search (tfk_ctc_beam_topk), the kept labels from the logits as given.
    live: a list that receives one list per utterance, every frame's number of live candidates."""
    logits = np.asarray(logits)
    U, O = len(utt_lens), logits.shape[1]
    hyps, scores, am, t0 = [], np.full((U, top_paths), -np.inf), np.full((U, top_paths), -np.inf), 0
    for u, n in enumerate(utt_lens):
        z = logits[t0:t0 + n]
        keep = None if label_topk is None else kept_labels(z, min(int(label_topk), O - 1))
        counts = [] if live is not None else None
        final = _beam_one_graph(log_softmax(z.astype(dtype)), W, lm, dtype, keep, counts)[:top_paths]
        if live is not None:
            live.append(counts)
        t0 += n
        hyps.append([np.array(h, dtype=np.int32) for h, _, _ in final] + [np.zeros(0, np.int32)] * (top_paths - len(final)))
        scores[u, :len(final)] = [s for _, s, _ in final]
        am[u, :len(final)] = [a for _, _, a in final]
    return hyps, scores, am


# ---- 1. a graph made from an n-gram is the n-gram search, exactly ----
@pytest.mark.parametrize("eos", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_from_ngram_equals_the_ngram_restatement_exactly(order, eos):
    z = 2.0 * np.random.default_rng(90).standard_normal((4 * 40, 9))
    table = log_softmax(1.5 * np.random.default_rng(91).standard_normal((9 ** (order - 1), 9)))
    lm = NgramLM(table, order, weight=0.6, label_bonus=0.4, end_of_sequence=eos)
    graph = GraphLM.from_ngram(lm)
    assert graph.num_states == 9 ** (order - 1) and graph.start == lm.start and graph.table is not lm.table
    for dtype in (np.float64, np.float32):
        want = prefix_beam_search_lm(z, [40] * 4, 10, 4, lm, dtype=dtype)
        got = prefix_beam_search_graph(z, [40] * 4, 10, 4, graph, dtype=dtype)
        assert [[h.tolist() for h in u] for u in got[0]] == [[h.tolist() for h in u] for u in want[0]]
        assert got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
    assert sum(h[0].size for h in got[0]) > 10
    for seq in ([], [3], [1, 7, 7, 0, 2]):
        assert graph.score(seq) == lm.score(seq) and graph.state(seq) == lm.context(seq) and graph.accepts(seq)


# ---- 2. exhaustive enumeration under a constraint ----
def enumeration_graph(eos):
    """the graph of the exhaustive pin (and of its GPU twin): 4 states over 2 labels + blank; from the start only label 0
    leaves, then both labels loop on state 1; states 2 and 3 are never reached.  Every state is final (a finite end weight)."""
    weight = log_softmax(1.5 * np.random.default_rng(11).standard_normal((4, 3))).astype(np.float32)
    nxt = np.array([[1, -1, 0], [1, 1, 0], [2, -1, 0], [-1, 1, 0]])
    return GraphLM(weight, nxt, start=0, weight=0.8, label_bonus=0.5, end_of_sequence=eos)


@pytest.mark.parametrize("eos", [False, True])
def test_unpruned_beam_equals_the_enumeration_of_the_accepted_labellings(eos):
    lm = enumeration_graph(eos)
    worst, margin = 0.0, np.inf
    for z in enumeration_cases():
        exact = enumerate_labellings(z)
        accepted = {lab: s for lab, s in exact.items() if lm.accepts(lab)}
        assert 2 <= len(accepted) <= 40 and len(accepted) < len(exact)  # the constraint bites and is not empty
        want = sorted(((lab, s + lm.score(lab)) for lab, s in accepted.items()), key=lambda e: (-e[1], len(e[0]), e[0]))
        hyps, scores, am = prefix_beam_search_graph(z, [6], 128, 127, lm)
        n = len(want)
        assert [tuple(h.tolist()) for h in hyps[0][:n]] == [lab for lab, _ in want]
        assert np.all(scores[0, n:] == -np.inf) and np.all(am[0, n:] == -np.inf)  # nothing else is in the beam
        worst = max(worst, np.abs(scores[0, :n] - np.array([s for _, s in want])).max())
        assert np.abs(am[0, :n] - np.array([exact[lab] for lab, _ in want])).max() <= 1e-12
        margin = min(margin, want[0][1] - want[1][1])
    print("eos %d: %d accepted labellings, worst |restatement - enumeration| %.1e, smallest margin %.2e"
          % (eos, n, worst, margin))
    assert worst <= 1e-12
    assert margin > 1e-3  # (so the GPU version of this test needs no exclusions)


# ---- 3. GraphLM ----
def test_graph_lm_rejects_bad_graphs(monkeypatch):
    w = np.zeros((3, 4))
    nxt = np.array([[1, 2, -1, 0], [0, -1, -1, 0], [2, 2, 2, 0]])
    g = GraphLM(w, nxt, start=1)
    assert g.num_states == 3 and g.num_classes == 4 and g.num_labels == 3 and g.start == 1
    assert g.table.dtype == np.float32 and g.next.dtype == np.int32
    assert np.array_equal(np.isneginf(g.table), np.array([[0, 0, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]], dtype=bool))
    assert g.weight == 1.0 and g.label_bonus == 0.0 and g.end_of_sequence is False
    for bad_next in (3, -2):
        n2 = nxt.copy()
        n2[1, 0] = bad_next
        with pytest.raises(ValueError, match="entry 4 of next"):
            GraphLM(w, n2)
    n2 = nxt.copy()
    n2[2, 3] = 99  # (the final column of next is not read)
    GraphLM(w, n2)
    for bad in (-np.inf, np.inf, np.nan):
        w2 = w.copy()
        w2[0, 1] = bad  # on an arc
        with pytest.raises(ValueError, match="entry 1 "):
            GraphLM(w2, nxt)
    for bad in (np.nan, np.inf):
        w2 = w.copy()
        w2[0, 2] = bad  # NaN and +inf are rejected anywhere, arc or not
        with pytest.raises(ValueError, match="entry 2 "):
            GraphLM(w2, nxt)
        w2 = w.copy()
        w2[1, 3] = bad  # and as a final weight
        with pytest.raises(ValueError, match="entry 7 "):
            GraphLM(w2, nxt)
    w2 = w.copy()
    w2[0, 2] = w2[1, 3] = -np.inf  # -inf where there is no arc, and a state that is not final
    assert not np.isfinite(GraphLM(w2, nxt).table[1, 3])
    for start in (-1, 3):
        with pytest.raises(ValueError, match="start"):
            GraphLM(w, nxt, start=start)
    for shape_w, shape_n in (((3, 4), (3, 3)), ((3, 1), (3, 1)), ((2, 3, 4), (2, 3, 4))):
        with pytest.raises(ValueError):
            GraphLM(np.zeros(shape_w), np.zeros(shape_n, dtype=np.int64))
    with pytest.raises(ValueError):
        GraphLM(w, nxt.astype(np.float64))
    with pytest.raises(ValueError, match="labels"):
        g.check(5)
    g.check(4)
    monkeypatch.setattr(ctc_lm, "MAX_GRAPH_ENTRIES", 11)  # the size limit, without allocating 2^25 entries
    with pytest.raises(ValueError, match="more than the device takes"):
        GraphLM(w, nxt)
    assert ctc_lm.MAX_GRAPH_ENTRIES == 11


def test_graph_lm_size_limit_is_the_devices():
    assert ctc_lm.MAX_GRAPH_ENTRIES == 1 << 25


def test_graph_lm_scores_states_and_acceptance():
    # labels a = 0, b = 1, blank 2.  state 0 -a-> 1, state 1 -b-> 0 and -a-> 1; only state 0 is final
    w = np.array([[-0.5, 0.0, -0.25], [-1.0, -2.0, -np.inf]])
    nxt = np.array([[1, -1, 0], [1, 0, 0]])
    g = GraphLM(w, nxt, weight=0.5, label_bonus=0.125)
    assert g.state([]) == 0 and g.state([0]) == 1 and g.state([0, 0, 1]) == 0 and g.state([1]) is None and g.state([0, 1, 1]) is None
    assert g.accepts([]) and g.accepts([0, 0]) and not g.accepts([1]) and not g.accepts([0, 1, 1, 0])
    assert g.score([0, 0, 1]) == 0.5 * (-0.5 - 1.0 - 2.0) + 3 * 0.125
    assert g.score([]) == 0.0 and g.score([1]) == -np.inf and g.score([0, 1, 1]) == -np.inf
    e = GraphLM(w, nxt, weight=0.5, label_bonus=0.125, end_of_sequence=True)
    assert e.score([0, 1]) == 0.5 * (-0.5 - 2.0) + 2 * 0.125 + 0.5 * -0.25 and e.score([]) == 0.5 * -0.25
    assert e.score([0]) == -np.inf and not e.accepts([0]) and e.accepts([0, 1]) and e.state([0]) == 1
    z = GraphLM(w, nxt, weight=0.0, end_of_sequence=True)  # the constraint does not depend on the weight
    assert z.score([0, 1]) == 0.0 and z.score([0]) == -np.inf and z.score([1]) == -np.inf
    with pytest.raises(ValueError):
        g.state([2])  # the blank is not a label


LEXICON = [[0, 1], [0, 1, 2], [2], [1, 0, 0], [2, 2, 1]]  # (word 0 is a prefix of word 1)


def _word_sequences(sep, max_len):
    """every label string up to max_len that is w1 sep w2 ... sep wn, n >= 1 (sep None: n == 1)"""
    words = [tuple(w) for w in LEXICON]
    out, frontier = set(), set(words)
    while frontier:
        out |= {s for s in frontier if len(s) <= max_len}
        frontier = set() if sep is None else {s + (sep,) + w for s in frontier for w in words if len(s) + 1 + len(w) <= max_len}
    return out


def test_from_lexicon_accepts_exactly_the_word_sequences():
    logp = np.log(np.array([0.1, 0.2, 0.3, 0.25, 0.15]))
    lm = GraphLM.from_lexicon(LEXICON, 4, separator=3, word_logprob=logp, end_of_sequence=True)
    assert lm.num_classes == 5 and lm.start == 0 and lm.table[0, -1] == -np.inf  # the root is not final
    want = _word_sequences(3, 6)
    got = {s for n in range(7) for s in itertools.product(range(4), repeat=n) if lm.accepts(s)}
    assert got == want and len(want) > 20
    assert abs(lm.score([0, 1, 3, 2]) - (logp[0] + logp[2])) <= 1e-6  # the separator and the end carry the word's weight
    assert abs(lm.score([0, 1, 2]) - logp[1]) <= 1e-6
    open_end = GraphLM.from_lexicon(LEXICON, 4, separator=3)  # without the end flag every prefix of a sequence is a path
    assert open_end.accepts([0]) and open_end.accepts([0, 1, 3]) and not open_end.accepts([3]) and not open_end.accepts([0, 0])
    assert open_end.score([0, 1, 3, 2, 2]) == 0.0
    alone = GraphLM.from_lexicon(LEXICON, 4, separator=None, word_logprob=logp, end_of_sequence=True)
    got = {s for n in range(7) for s in itertools.product(range(4), repeat=n) if alone.accepts(s)}
    assert got == {tuple(w) for w in LEXICON} == _word_sequences(None, 6)
    assert abs(alone.score([2, 2, 1]) - logp[4]) <= 1e-6
    with pytest.raises(ValueError, match="repeats word 0"):
        GraphLM.from_lexicon(LEXICON + [[0, 1]], 4, separator=3)
    for words in ([[0, 3]], [[]], [[4]], []):
        with pytest.raises(ValueError):
            GraphLM.from_lexicon(words, 4, separator=3)
    with pytest.raises(ValueError):
        GraphLM.from_lexicon(LEXICON, 4, separator=4)
    with pytest.raises(ValueError):
        GraphLM.from_lexicon(LEXICON, 4, separator=3, word_logprob=logp[:4])


# ---- 4. fewer live candidates than the beam ----
def single_word_inputs():
    """one word of 12 labels over 5 letters + separator 5 + blank 6, two utterances of 30 frames of noise.  Draw order: the
    logits, then the word."""
    rng = np.random.default_rng(3)
    z = (2.0 * rng.standard_normal((2 * 30, 7))).astype(np.float32)
    word = rng.integers(0, 5, size=12)
    return z, [30, 30], word


def test_fewer_live_candidates_than_the_beam():
    z, utt, word = single_word_inputs()
    lm = GraphLM.from_lexicon([word], 6, separator=5, weight=0.5, label_bonus=0.3)
    live = []
    hyps, scores, am = prefix_beam_search_graph(z, utt, 8, 8, lm, live=live)
    fewest = min(min(c) for c in live)
    print("live candidates per frame: fewest %d, most %d (beam 8)" % (fewest, max(max(c) for c in live)))
    assert fewest <= 2
    assert all(min(c) < 8 for c in live)
    for u in range(2):
        listed = [h for h, s in zip(hyps[u], scores[u]) if s > -np.inf]
        assert listed and all(lm.accepts(h) for h in listed)
        assert len({tuple(h.tolist()) for h in listed}) == len(listed)
    assert np.all(np.isfinite(scores[:, 0])) and not np.any(np.isnan(scores)) and not np.any(np.isnan(am))
    h32, s32, _ = prefix_beam_search_graph(z, utt, 8, 1, lm, dtype=np.float32)
    assert np.abs(s32[:, 0] - scores[:, 0]).max() < 1e-3


# ---- the lexicon inputs of the GPU tier ----
def lexicon_inputs(U=8, Tn=120, words_per_utt=3):
    """the lexicon inputs of the GPU tests (and of tools/ctc_bench.py --graph): 26 letters, separator 26, blank 27; 50 distinct
    words of 2 to 6 letters with the log of a Dirichlet draw as their weights; U utterances of Tn frames that spell
    words_per_utt lexicon words each -- noise of deviation 1.5, the blank + 6, one peak + U(3, 15) per label on distinct
    frames out of every third frame, 15 % of the peaks moved to a random letter.  Everything from default_rng(7), drawn in
    this order: the 50 words' lengths, then letters until 50 distinct words stand, the Dirichlet draw, per utterance its
    words; then per utterance the noise, the peak frames, the peak heights, which peaks are moved and where to.  Returns
    (logits float32, utterance lengths, reference label arrays, the GraphLM: weight 0.5, bonus 0.3, end flag on)."""
    rng = np.random.default_rng(7)
    O, sep = 28, 26
    lengths = rng.integers(2, 7, size=50)
    words, seen = [], set()
    for n in lengths:
        while True:
            w = tuple(rng.integers(0, 26, size=n).tolist())
            if w not in seen:
                break
        seen.add(w)
        words.append(np.array(w))
    logp = np.log(rng.dirichlet(np.ones(50)))
    refs = []
    for u in range(U):
        pick = rng.integers(0, 50, size=words_per_utt)
        refs.append(np.concatenate([np.concatenate([[sep], words[i]]) for i in pick])[1:].astype(np.int32))
    z = np.empty((U * Tn, O))
    for u, ref in enumerate(refs):
        zu = rng.standard_normal((Tn, O)) * 1.5
        zu[:, O - 1] += 6.0
        frames = np.sort(rng.choice(np.arange(0, Tn, 3), size=ref.size, replace=False))
        height = rng.uniform(3.0, 15.0, size=ref.size)
        moved = rng.random(ref.size) < 0.15
        other = rng.integers(0, 26, size=ref.size)
        zu[frames, np.where(moved, other, ref)] += height
        z[u * Tn:(u + 1) * Tn] = zu
    lm = GraphLM.from_lexicon(words, 27, sep, word_logprob=logp, weight=0.5, label_bonus=0.3, end_of_sequence=True)
    return z.astype(np.float32), [Tn] * U, refs, lm
