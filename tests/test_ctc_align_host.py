"""CTC forced alignment, CPU tier: the numpy restatement the GPU tests check the engine against (the contract stated in
include/tfkaldi_hip.h at tfk_ctc_align: the Viterbi path through the CTC lattice of a KNOWN label sequence, the max-plus
recursion on the raw logits, ties to the higher-numbered predecessor), pinned by exhaustive enumeration of all frame
labellings and by known answers; ctc_segments; and Decoder.ctc_align over a numpy stand-in engine."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def row_lse(z):
    """log-sum-exp of every row, in z's dtype"""
    m = z.max(axis=1)
    return m + np.log(np.exp(z - m[:, None]).sum(axis=1, dtype=z.dtype))


def lattice(labels, O):
    """(class of every state, skip-transition mask) of the 2S + 1 states blank, l_0, blank, ..., blank"""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    ext = np.full(2 * labels.size + 1, O - 1, dtype=np.int64)
    ext[1::2] = labels
    skip = np.zeros(ext.size, dtype=bool)
    skip[3::2] = labels[1:] != labels[:-1]  # into a label state whose label differs from the label two states back
    return ext, skip


def viterbi_align(z, labels, dtype=np.float64):
    """numpy restatement of tfk_ctc_align for ONE utterance with logits z [T, O]: (ali, score).  ali int32 [T]: per frame
    the position of the label it emits, -1 for a blank frame; None when no valid path exists.  score: the natural-log
    probability of the path, -inf without one.  dtype: the arithmetic of the row log-sum-exps and of the recursion, which
    runs on the raw logits: candidates in the order stay, +1, +2, a later one wins only if strictly larger."""
    z = np.asarray(z).astype(dtype)
    T, O = z.shape
    ext, skip = lattice(labels, O)
    n = ext.size
    if T == 0:
        return (np.zeros(0, np.int32), 0.0) if n == 1 else (None, -np.inf)
    ninf = dtype(-np.inf)
    v = np.full(n, ninf, dtype=dtype)
    v[:2] = z[0, ext[:2]]
    back = np.zeros((T, n), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            best, d = v.copy(), back[t]
            p1 = np.concatenate([[ninf], v[:-1]])
            take = p1 > best
            best[take], d[take] = p1[take], 1
            p2 = np.concatenate([[ninf, ninf], v[:-2]])[:n]
            take = skip & (p2 > best)
            best[take], d[take] = p2[take], 2
            v = (best + z[t, ext]).astype(dtype)
    s = n - 2 if n >= 2 and v[n - 2] > v[n - 1] else n - 1  # n - 1 wins unless n - 2 is strictly larger
    if not v[s] > ninf:
        return None, -np.inf
    score = float(v[s] - row_lse(z).sum(dtype=dtype))
    states = np.empty(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(back[t, s])
    return np.where(states & 1, states >> 1, -1).astype(np.int32), score


def path_score(z, labels, ali):
    """float64 log-probability of the alignment `ali` of `labels` under logits z [T, O]"""
    z = np.asarray(z, dtype=np.float64)
    ali = np.asarray(ali)
    cls = np.where(ali >= 0, np.asarray(labels, dtype=np.int64)[np.maximum(ali, 0)] if len(labels) else 0, z.shape[1] - 1)
    return float((z[np.arange(z.shape[0]), cls] - row_lse(z)).sum())


def collapse(classes, blank):
    """merge repeats, then drop blanks"""
    return tuple(int(k) for k, prev in zip(classes, (-1,) + tuple(classes[:-1])) if k != blank and k != prev)


def check_valid(ali, labels, O):
    """`ali` is an allowed path of `labels`: positions non-decreasing in steps of at most one label, first label first, last
    label last, a blank between equal neighbours -- equivalently its frame classes collapse to the labels"""
    labels = np.asarray(labels, dtype=np.int64)
    ali = np.asarray(ali)
    assert ali.dtype == np.int32 and np.all(ali >= -1) and np.all(ali < labels.size)
    pos = ali[ali >= 0]
    assert np.all(np.diff(pos) >= 0) and np.all(np.diff(pos) <= 1)
    assert pos.size == 0 or (pos[0] == 0 and pos[-1] == labels.size - 1)
    assert labels.size == 0 or pos.size > 0
    # two frames of DIFFERENT positions with the same label need a blank frame between them
    t = np.nonzero(ali >= 0)[0]
    for a, b in zip(t[:-1], t[1:]):
        if ali[a] != ali[b] and labels[ali[a]] == labels[ali[b]]:
            assert b > a + 1
    classes = np.where(ali >= 0, labels[np.maximum(ali, 0)] if labels.size else 0, O - 1)
    assert collapse(tuple(classes.tolist()), O - 1) == tuple(labels.tolist())


def integer_logits(rng, T, O):
    return rng.integers(-3, 4, size=(T, O)).astype(np.float32)


def test_restatement_equals_exhaustive_enumeration():
    """2 labels + blank, T = 6: every one of the 3^6 frame labellings that collapses to the target is scored"""
    rng = np.random.default_rng(200)
    T, O = 6, 3
    paths = list(itertools.product(range(O), repeat=T))
    collapsed = [collapse(p, O - 1) for p in paths]
    targets = [(), (0,), (1,), (0, 1), (1, 0), (0, 0), (1, 1), (0, 1, 0), (1, 1, 0), (0, 0, 1), (0, 1, 0, 1), (1, 1, 1)]
    for case in range(60):
        z = 2.0 * rng.standard_normal((T, O))
        lp = z - row_lse(z)[:, None]
        target = targets[case % len(targets)]
        scores = [sum(lp[t, k] for t, k in enumerate(p)) for p, c in zip(paths, collapsed) if c == target]
        assert scores, target
        ali, score = viterbi_align(z, target)
        assert abs(score - max(scores)) <= 1e-12, (case, target)
        check_valid(ali, target, O)
        assert abs(path_score(z, target, ali) - score) <= 1e-12
    # (1, 1, 1, 1) needs 7 frames
    assert viterbi_align(z, (1, 1, 1, 1)) == (None, -np.inf)


def test_known_answers():
    O = 3
    z = np.array([[1.0, 0.0, 2.0], [0.5, 3.0, -1.0], [0.0, 0.0, 0.0], [2.0, 1.0, 0.5]])
    lp = z - row_lse(z)[:, None]
    ali, score = viterbi_align(z, [])  # S = 0: all blank
    assert ali.tolist() == [-1] * 4 and abs(score - lp[:, O - 1].sum()) <= 1e-12
    ali, score = viterbi_align(z[:3], [0, 0])  # exactly feasible: a blank a is the only path
    assert ali.tolist() == [0, -1, 1] and abs(score - (lp[0, 0] + lp[1, 2] + lp[2, 0])) <= 1e-12
    assert viterbi_align(z[:2], [0, 0]) == (None, -np.inf)  # one frame short
    ali, score = viterbi_align(z[:2], [0, 1])  # a b in two frames: the skip transition
    assert ali.tolist() == [0, 1] and abs(score - (lp[0, 0] + lp[1, 1])) <= 1e-12
    assert viterbi_align(np.zeros((0, O)), [])[1] == 0.0 and viterbi_align(np.zeros((0, O)), [])[0].size == 0
    assert viterbi_align(np.zeros((0, O)), [1]) == (None, -np.inf)
    ali, _ = viterbi_align(z[:1], [1])
    assert ali.tolist() == [0]
    # a clear answer: one-hot-like logits
    big = 20.0 * np.eye(O)[[2, 0, 0, 2, 1, 2]]
    assert viterbi_align(big, [0, 1])[0].tolist() == [-1, 0, 0, -1, 1, -1]


def test_ties_fall_as_the_rule_says():
    """of equal predecessors the higher-numbered wins (stay before +1 before +2); at the end n - 1 unless n - 2 is larger"""
    zero = np.zeros((2, 2))
    # states blank a blank, all paths tie: state 2 wins the end, its only predecessor at t = 0 is state 1
    assert viterbi_align(zero, [0])[0].tolist() == [0, -1]
    # frame 1 prefers a: the end state n - 2 is strictly larger; at state 1 stay ties with +1 and stays
    assert viterbi_align(np.array([[0.0, 0.0], [1.0, 0.0]]), [0])[0].tolist() == [0, 0]
    # frame 0 prefers the blank: at state 1, +1 is strictly larger than stay
    assert viterbi_align(np.array([[-1.0, 0.0], [0.0, 0.0]]), [0])[0].tolist() == [-1, 0]
    # a b over three all-zero frames: state 4 ends, from 3 (stay ties with +1 and +2 and keeps 3), which came by the skip
    assert viterbi_align(np.zeros((3, 3)), [0, 1])[0].tolist() == [0, 1, -1]
    # a a over four all-zero frames: no skip between equal labels
    assert viterbi_align(np.zeros((4, 3)), [0, 0])[0].tolist() == [0, -1, 1, -1]
    # the float32 run takes every tie the same way
    for z, lab in ((zero, [0]), (np.zeros((3, 3)), [0, 1]), (np.zeros((4, 3)), [0, 0])):
        assert viterbi_align(z, lab, np.float32)[0].tolist() == viterbi_align(z, lab)[0].tolist()


def test_integer_logits_are_exact_in_float32_and_exercise_the_tie_rule():
    """integer logits in [-3, 3]: the float32 and the float64 recursion give the same path (every intermediate is an exact
    integer), and such inputs are full of ties: breaking them the other way changes most paths"""
    rng = np.random.default_rng(201)
    changed = 0
    for case in range(40):
        T = int(rng.integers(20, 200))
        z = integer_logits(rng, T, 9)
        lab = rng.integers(0, 8, size=int(rng.integers(0, T // 3 + 1)))
        a64, s64 = viterbi_align(z, lab)
        a32, s32 = viterbi_align(z, lab, np.float32)
        assert np.array_equal(a64, a32)
        check_valid(a64, lab, 9)
        assert abs(s32 - s64) <= 1e-3 and abs(path_score(z, lab, a64) - s64) <= 1e-9
        # the same optimum reached through the mirrored problem: reversed frames and labels, path mirrored back
        back, sb = viterbi_align(z[::-1], lab[::-1])
        mirrored = np.where(back[::-1] >= 0, lab.size - 1 - back[::-1], -1)
        assert abs(sb - s64) <= 1e-9
        changed += not np.array_equal(mirrored, a64)
    assert changed >= 20, changed


def test_long_references():
    """the longest label sequence the engine takes, just enough frames and slack"""
    rng = np.random.default_rng(204)
    lab = rng.integers(0, 8, size=511)
    need = lab.size + int(np.sum(lab[1:] == lab[:-1]))
    for T in (need - 1, need, need + 200):
        z = integer_logits(rng, T, 9)
        ali, score = viterbi_align(z, lab)
        if T < need:
            assert ali is None and score == -np.inf
            continue
        check_valid(ali, lab, 9)
        assert np.array_equal(ali, viterbi_align(z, lab, np.float32)[0])
        assert abs(path_score(z, lab, ali) - score) <= 1e-9
        if T == need:  # a single path: every label one frame, a blank between equal neighbours
            assert np.array_equal(ali[ali >= 0], np.arange(lab.size))


# ---- ctc_segments ----
def test_ctc_segments():
    from tfkaldi_amd.neuralNetworks.decoder import ctc_segments
    ali = np.array([-1, 0, 0, -1, 1, 2, 2, 2, -1, -1], np.int32)
    assert ctc_segments(ali, [5, 7, 7]) == [(5, 1, 3), (7, 4, 5), (7, 5, 8)]  # a repeated label: two segments
    assert ctc_segments(np.array([0, -1, 1], np.int32), [3, 3]) == [(3, 0, 1), (3, 2, 3)]
    assert ctc_segments(np.full(4, -1, np.int32), []) == []  # all blank
    assert ctc_segments(np.zeros(0, np.int32), []) == []
    assert ctc_segments(None, [1, 2]) is None  # no valid alignment
    segs = ctc_segments(np.array([0, 1, 2], np.int32), np.array([4, 5, 4]))
    assert segs == [(4, 0, 1), (5, 1, 2), (4, 2, 3)] and all(type(v) is int for s in segs for v in s)
    for bad, lab in (([0, 2], [1, 1, 1]), ([1, 0], [1, 2]), ([0, 3], [1, 2]), ([-1, -1], [1]), ([0, -1, 0, 1], [1, 2])):
        with pytest.raises(ValueError):
            ctc_segments(np.array(bad, np.int32), lab)
    rng = np.random.default_rng(202)
    for _ in range(20):  # segments of the restatement's alignments: ordered, disjoint, one per label, the frames of ali
        T = int(rng.integers(10, 80))
        z = 2.0 * rng.standard_normal((T, 6))
        lab = rng.integers(0, 5, size=int(rng.integers(0, T // 3 + 1)))
        ali, _ = viterbi_align(z, lab)
        segs = ctc_segments(ali, lab)
        assert [s[0] for s in segs] == lab.tolist()
        assert all(0 <= a < b <= T for _, a, b in segs) and all(x[2] <= y[1] for x, y in zip(segs[:-1], segs[1:]))
        rebuilt = np.full(T, -1, np.int32)
        for j, (_, a, b) in enumerate(segs):
            rebuilt[a:b] = j
        assert np.array_equal(rebuilt, ali)


# ---- Decoder.ctc_align over a numpy stand-in engine ----
F, O = 6, 5


class NumpyAlignEngine(object):
    """stand-in for Engine's alignment entries: logits = X @ W of a fixed seeded matrix, aligned by the restatement"""

    def __init__(self):
        self.W = 3.0 * np.random.default_rng(12).standard_normal((F, O)).astype(np.float32)
        self.calls = []

    def ctc_align(self, X, utt_lens, labels, label_lens):
        self.calls.append(("align", len(utt_lens)))
        return self._run(X, utt_lens, labels, label_lens)

    def _run(self, X, utt_lens, labels, label_lens):
        z = np.asarray(X, dtype=np.float32) @ self.W
        assert z.shape[0] == sum(utt_lens) and len(labels) == sum(label_lens)
        zs = np.split(z, np.cumsum(utt_lens)[:-1])
        refs = np.split(np.asarray(labels), np.cumsum(label_lens)[:-1])
        out = [viterbi_align(a, b) for a, b in zip(zs, refs)]
        return [a for a, _ in out], np.array([s for _, s in out], dtype=np.float32)

    def ctc_align_raw(self, raw, utt_lens, context_width, labels, label_lens, cmvn=None):
        assert context_width == 0 and cmvn is None
        self.calls.append(("raw", len(utt_lens)))
        return self._run(raw, utt_lens, labels, label_lens)


def _decoder(engine, max_length=64):
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    dec = Decoder.__new__(Decoder)  # (the constructor creates a device engine)
    dec.engine, dec.max_length = engine, max_length
    return dec


def test_decoder_ctc_align_over_a_stand_in_engine():
    from tfkaldi_amd.neuralNetworks.decoder import ctc_segments
    from tfkaldi_amd.processing.feature_reader import Unspliced
    rng = np.random.default_rng(203)
    lens = [30, 2, 17, 0, 9]
    xs = [rng.standard_normal((n, F)).astype(np.float32) for n in lens]
    ys = [rng.integers(0, O - 1, size=k) for k in (6, 3, 0, 0, 2)]  # the second utterance is too short for its labels
    eng = NumpyAlignEngine()
    dec = _decoder(eng)
    alis, scores = dec.ctc_align(xs, ys)
    assert eng.calls == [("align", 5)]  # every utterance in ONE pass
    assert scores.dtype == np.float32 and scores.shape == (5,)
    assert alis[1] is None and scores[1] == -np.inf
    assert alis[3].size == 0 and scores[3] == 0.0
    for u in (0, 2, 4):
        want, s = viterbi_align(xs[u] @ eng.W, ys[u])
        assert np.array_equal(alis[u], want) and alis[u].dtype == np.int32 and abs(scores[u] - s) <= 1e-4
        assert [k for k, _, _ in ctc_segments(alis[u], ys[u])] == ys[u].tolist()
    assert ctc_segments(alis[1], ys[1]) is None
    # all Unspliced: the device-splice entry, one pass
    raw = dec.ctc_align([Unspliced(x, 0) for x in xs], ys)
    assert eng.calls == [("align", 5), ("raw", 5)]
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(raw[0], alis))
    assert raw[1].tobytes() == scores.tobytes()
    # mixed: spliced on the host, stacked
    mixed = dec.ctc_align([Unspliced(xs[0], 0)] + xs[1:], ys)
    assert eng.calls[-1] == ("align", 5) and mixed[1].tobytes() == scores.tobytes()
    got = dec.ctc_align([], [])
    assert got[0] == [] and got[1].shape == (0,) and got[1].dtype == np.float32
    with pytest.raises(ValueError):
        dec.ctc_align(xs, ys[:-1])
    with pytest.raises(ValueError):  # longer than the decoder's max_length, as every Decoder entry
        _decoder(eng, max_length=20).ctc_align(xs, ys)
