"""CTC alignment with wildcard gaps and keyword spotting, CPU tier: the numpy restatement the GPU tests check the engine
against (the contract stated in include/tfkaldi_hip.h at tfk_ctc_align_wild / tfk_ctc_spot: the lattice, transitions and
tie rule of tfk_ctc_align, a flagged gap state emitting the frame's largest logit), pinned by exhaustive enumeration of all
state paths, by known answers and by a planted keyword; and Decoder.ctc_align_wild / Decoder.ctc_spot over a numpy stand-in
engine."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from test_ctc_align_host import integer_logits, lattice, row_lse, viterbi_align  # noqa: E402


def gap_flags(labels, wild):
    """the S + 1 flags of one label sequence as a bool array; wild: None, "ends", "all" or the flags themselves"""
    S = len(labels)
    if wild is None:
        return np.zeros(S + 1, dtype=bool)
    if isinstance(wild, str):
        f = np.ones(S + 1, dtype=bool)
        if wild == "ends":
            f[1:-1] = False
        return f
    f = np.asarray(wild).astype(bool).reshape(-1)
    assert f.size == S + 1
    return f


def emissions(z, labels, wild):
    """[T, n] what every state emits per frame (raw logits; a wildcard gap: the row maximum), and the skip mask"""
    ext, skip = lattice(labels, z.shape[1])
    e = z[:, ext]
    w = np.zeros(ext.size, dtype=bool)
    w[0::2] = gap_flags(labels, wild)
    if z.shape[0]:
        e[:, w] = z.max(axis=1)[:, None]
    return e, skip


def _sweep(z, labels, wild, dtype):
    """the recursion of the contract in `dtype`: candidates in the order stay, +1, +2, a later one wins only if strictly
    larger; beside every state value the start frame of its path (set on entering state 1 from state 0 or starting there,
    else inherited from the chosen predecessor) and, per state, the frame at which it was last entered by a step of 1.
    Returns (back-pointers [T, n], end state or None, score, free, start, end)."""
    z = np.asarray(z).astype(dtype)
    T = z.shape[0]
    e, skip = emissions(z, labels, wild)
    n = e.shape[1]
    if T == 0:
        return None, (0 if n == 1 else None), (0.0 if n == 1 else -np.inf), 0.0, (0 if n == 1 else -1), (0 if n == 1 else -1)
    lse = row_lse(z)
    free = float((z.max(axis=1) - lse).sum(dtype=dtype))
    ninf = dtype(-np.inf)
    v = np.full(n, ninf, dtype=dtype)
    v[:2] = e[0, :2]
    st = np.zeros(n, dtype=np.int64)
    en = np.zeros(n, dtype=np.int64)
    back = np.zeros((T, n), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            best, d = v.copy(), back[t]
            p1 = np.concatenate([[ninf], v[:-1]])
            q1 = np.concatenate([[0], st[:-1]])
            if n > 1:
                q1[1] = t  # into state 1 from state 0: the path starts here
            take = p1 > best
            best[take], d[take] = p1[take], 1
            p2 = np.concatenate([[ninf, ninf], v[:-2]])[:n]
            q2 = np.concatenate([[0, 0], st[:-2]])[:n]
            take = skip & (p2 > best)
            best[take], d[take] = p2[take], 2
            st = np.where(d == 1, q1, np.where(d == 2, q2, st))
            en = np.where(d == 1, t, en)
            v = (best + e[t]).astype(dtype)
    s = n - 2 if n >= 2 and v[n - 2] > v[n - 1] else n - 1  # n - 1 wins unless n - 2 is strictly larger
    if not v[s] > ninf:
        return None, None, -np.inf, free, -1, -1
    score = float(v[s] - lse.sum(dtype=dtype))
    if n == 1:
        return back, s, score, free, 0, 0
    return back, s, score, free, int(st[s]), (T if s == n - 2 else int(en[n - 1]))


def wild_align(z, labels, wild=None, dtype=np.float64):
    """numpy restatement of tfk_ctc_align_wild for ONE utterance with logits z [T, O]: (ali, score, free).  ali int32 [T]: per
    frame the position of the label it emits, -1 for a frame in any gap; None without a valid path (score -inf)."""
    back, s, score, free, _, _ = _sweep(z, labels, wild, dtype)
    T = np.asarray(z).shape[0]
    if s is None:
        return None, score, free
    states = np.empty(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(back[t, s])
    return np.where(states & 1, states >> 1, -1).astype(np.int32), score, free


def wild_spot(z, labels, wild=None, dtype=np.float64):
    """numpy restatement of tfk_ctc_spot for ONE pair: (score, start, end) from the forward sweep alone, no back-trace"""
    _, _, score, _, start, end = _sweep(z, labels, wild, dtype)
    return score, start, end


def span(ali):
    """(start, end) read off an alignment: the first frame that emits a label and one past the last; (0, 0) without label
    frames, (-1, -1) without a path"""
    if ali is None:
        return -1, -1
    t = np.nonzero(np.asarray(ali) >= 0)[0]
    return (int(t[0]), int(t[-1]) + 1) if t.size else (0, 0)


def wild_path_score(z, labels, wild, ali):
    """float64 log-probability of the frame labelling an alignment stands for: a label frame emits its label, a frame in a
    wildcard gap the frame's best class, a frame in a plain gap the blank.  The gap of a frame follows from its neighbours:
    gap g lies behind label g - 1."""
    z = np.asarray(z, dtype=np.float64)
    ali = np.asarray(ali)
    flags = gap_flags(labels, wild)
    lse = row_lse(z)
    total, g = 0.0, 0
    for t in range(z.shape[0]):
        if ali[t] >= 0:
            total += z[t, int(labels[ali[t]])] - lse[t]
            g = int(ali[t]) + 1
        else:
            total += (z[t].max() if flags[g] else z[t, -1]) - lse[t]
    return float(total)


def enumerate_paths(T, n, skip):
    """every valid state path of T frames through n states"""
    paths = [[0]] + ([[1]] if n > 1 else [])
    for _ in range(T - 1):
        grown = []
        for p in paths:
            s = p[-1]
            grown.append(p + [s])
            if s + 1 < n:
                grown.append(p + [s + 1])
            if s + 2 < n and skip[s + 2]:
                grown.append(p + [s + 2])
        paths = grown
    return [p for p in paths if p[-1] >= n - 2]


TARGETS = [(), (0,), (1,), (0, 1), (1, 0), (0, 0), (1, 1), (0, 1, 0), (1, 1, 0), (0, 1, 0, 1)]


def test_restatement_equals_exhaustive_enumeration():
    """O = 3, T = 6, 10 targets of up to 4 labels (repeats included), random flags, 300 cases: every valid state path is
    scored; score <= free, score >= the plain alignment's; all flags zero is viterbi_align"""
    rng = np.random.default_rng(700)
    T, O = 6, 3
    for case in range(300):
        z = 2.0 * rng.standard_normal((T, O))
        target = TARGETS[case % len(TARGETS)]
        flags = rng.integers(0, 2, size=len(target) + 1).astype(bool)
        e, skip = emissions(z, target, flags)
        lse = row_lse(z)
        scores = [sum(e[t, s] - lse[t] for t, s in enumerate(p)) for p in enumerate_paths(T, e.shape[1], skip)]
        assert scores, target
        ali, score, free = wild_align(z, target, flags)
        assert abs(score - max(scores)) <= 1e-12, (case, target, flags)
        assert abs(wild_path_score(z, target, flags, ali) - score) <= 1e-12
        plain = viterbi_align(z, target)
        assert score <= free + 1e-12 and score >= plain[1] - 1e-12
        assert abs(free - float((z.max(axis=1) - lse).sum())) <= 1e-12
        none = wild_align(z, target, None)
        assert np.array_equal(none[0], plain[0]) and none[1] == plain[1]
        assert wild_spot(z, target, flags) == (score,) + span(ali)
    assert wild_align(z, (1, 1, 1, 1), "all")[:2] == (None, -np.inf)  # 7 frames are needed, wildcards or not
    assert wild_spot(z, (1, 1, 1, 1), "all") == (-np.inf, -1, -1)


def _random_case(rng, T, O=9):
    z = integer_logits(rng, T, O)
    lab = rng.integers(0, O - 1, size=int(rng.integers(0, T // 3 + 1)))
    return z, lab, rng.integers(0, 2, size=lab.size + 1).astype(bool)


def test_integer_logits_are_exact_in_float32_and_exercise_the_tie_rule():
    """integer logits in [-3, 3]: the float32 and the float64 recursion give the same path, start and end; the mirrored
    problem (frames, labels and flags reversed) has the same score and, ties broken the other way, mostly another path"""
    rng = np.random.default_rng(701)
    changed = 0
    for case in range(60):
        z, lab, flags = _random_case(rng, int(rng.integers(20, 201)))
        a64, s64, f64 = wild_align(z, lab, flags)
        a32, s32, f32 = wild_align(z, lab, flags, np.float32)
        assert np.array_equal(a64, a32)
        assert wild_spot(z, lab, flags)[1:] == span(a64) == wild_spot(z, lab, flags, np.float32)[1:]
        assert abs(s32 - s64) <= 1e-3 and abs(f32 - f64) <= 1e-3
        assert abs(wild_path_score(z, lab, flags, a64) - s64) <= 1e-9 and s64 <= f64 + 1e-9
        back, sb, fb = wild_align(z[::-1], lab[::-1], flags[::-1])
        mirrored = np.where(back[::-1] >= 0, lab.size - 1 - back[::-1], -1)
        assert abs(sb - s64) <= 1e-9 and abs(fb - f64) <= 1e-9
        changed += not np.array_equal(mirrored, a64)
    assert changed >= 30, changed


def test_known_answers():
    O = 3
    z = np.array([[1.0, 0.0, 2.0], [0.5, 3.0, -1.0], [0.0, 0.5, 0.0], [2.0, 1.0, 0.5]])
    lp = z - row_lse(z)[:, None]
    ali, score, free = wild_align(z, [], [1])  # S = 0, its one gap wild: the unconstrained best path
    assert ali.tolist() == [-1] * 4 and abs(score - free) <= 1e-12 and abs(free - lp.max(axis=1).sum()) <= 1e-12
    assert wild_spot(z, [], [1]) == (score, 0, 0)
    assert wild_align(z[:2], [0, 0], [0, 1, 0])[:2] == (None, -np.inf)  # a * a in two frames: the gap still takes a frame
    assert wild_spot(z[:2], [0, 0], [0, 1, 0]) == (-np.inf, -1, -1)
    ali, score, _ = wild_align(z[:3], [0, 0], [0, 1, 0])  # in three frames: exactly one path, a (best class) a
    assert ali.tolist() == [0, -1, 1] and abs(score - (lp[0, 0] + lp[1, 1] + lp[2, 0])) <= 1e-12
    assert wild_spot(z[:3], [0, 0], [0, 1, 0])[1:] == (0, 3)
    # one label, both ends wild, one-hot-like logits: the label is found where it lies and everything else is free.  On the
    # label's second frame the wildcard emits the same logit as the label: a tie, and staying in the gap wins it
    big = 20.0 * np.eye(O)[[1, 1, 0, 0, 1, 2]]
    ali, score, free = wild_align(big, [0], "ends")
    assert ali.tolist() == [-1, -1, 0, -1, -1, -1] and abs(score - free) <= 1e-12
    assert wild_spot(big, [0], "ends")[1:] == (2, 3)
    ali, score, free = wild_align(big, [0], None)  # without wildcards the two frames of class 1 cost 20 each
    assert score < free - 39.0
    # the zero-frame cases
    none = np.zeros((0, O))
    ali, score, free = wild_align(none, [], [1])
    assert ali.size == 0 and score == 0.0 and free == 0.0 and wild_spot(none, [], [1]) == (0.0, 0, 0)
    assert wild_align(none, [1], "all") == (None, -np.inf, 0.0) and wild_spot(none, [1], "all") == (-np.inf, -1, -1)


def planted_case(rng, T=120, O=9, per_label=3, labels=5):
    """logits with a planted keyword: N(0, 1) everywhere, the frame's chosen class gets +6.  Noise frames choose among the
    labels 4 .. 7 and the blank; the keyword's labels come from 0 .. 3 (repeats allowed, a blank frame between equal
    neighbours), per_label frames each, at a random offset.  Returns (z, keyword, first planted frame, end)."""
    kw = rng.integers(0, 4, size=labels)
    classes = []
    for j, k in enumerate(kw):
        if j and kw[j - 1] == k:
            classes.append(O - 1)
        classes += [int(k)] * per_label
    at = int(rng.integers(0, T - len(classes) + 1))
    best = rng.choice([4, 5, 6, 7, O - 1], size=T)
    best[at:at + len(classes)] = classes
    z = rng.standard_normal((T, O))
    z[np.arange(T), best] += 6.0
    return z, kw, at, at + len(classes)


def test_planted_pattern_is_found_where_it_lies():
    rng = np.random.default_rng(702)
    for case in range(300):
        z, kw, first, last = planted_case(rng)
        ali, score, free = wild_align(z, kw, "ends")
        assert abs(score - free) <= 1e-3, (case, score, free)
        start, end = span(ali)
        assert first <= start < end <= last, (case, start, end, first, last)
        assert wild_spot(z, kw, "ends")[1:] == (start, end)
        for shift in (1, 2, 3):
            other = (kw + shift) % 4
            if np.array_equal(other, kw):
                continue
            assert wild_align(z, other, "ends")[1] < free - 1.0, (case, shift)


# ---- Decoder.ctc_align_wild / Decoder.ctc_spot over a numpy stand-in engine ----
F, O = 6, 5


class NumpyWildEngine(object):
    """stand-in for Engine's wildcard entries: logits = X @ W of a fixed seeded matrix, aligned by the restatement"""

    def __init__(self):
        self.W = 3.0 * np.random.default_rng(12).standard_normal((F, O)).astype(np.float32)
        self.calls = []

    def _split(self, X, utt_lens, labels, label_lens, wild):
        z = np.asarray(X, dtype=np.float32) @ self.W
        label_lens = np.asarray(label_lens, dtype=np.int64)
        assert z.shape[0] == sum(utt_lens) and len(labels) == label_lens.sum()
        seqs = np.split(np.asarray(labels), np.cumsum(label_lens)[:-1]) if label_lens.size else []
        if wild is None:
            flags = [None] * len(seqs)
        else:
            assert wild.dtype == np.uint8 and wild.size == label_lens.sum() + label_lens.size and wild.max(initial=0) <= 1
            flags = np.split(wild, np.cumsum(label_lens + 1)[:-1]) if label_lens.size else []
        return np.split(z, np.cumsum(utt_lens)[:-1]), seqs, flags

    def _align(self, X, utt_lens, labels, label_lens, wild):
        zs, seqs, flags = self._split(X, utt_lens, labels, label_lens, wild)
        out = [wild_align(z, s, f) for z, s, f in zip(zs, seqs, flags)]
        return ([a for a, _, _ in out], np.array([s for _, s, _ in out], dtype=np.float32),
                np.array([f for _, _, f in out], dtype=np.float32))

    def ctc_align_wild(self, X, utt_lens, labels, label_lens, wild=None):
        self.calls.append(("align", len(utt_lens)))
        return self._align(X, utt_lens, labels, label_lens, wild)

    def ctc_align_wild_raw(self, raw, utt_lens, context_width, labels, label_lens, wild=None, cmvn=None):
        assert context_width == 0 and cmvn is None
        self.calls.append(("align_raw", len(utt_lens)))
        return self._align(raw, utt_lens, labels, label_lens, wild)

    def _spot(self, X, utt_lens, pat_counts, labels, label_lens, wild):
        zs, seqs, flags = self._split(X, utt_lens, labels, label_lens, wild)
        utt = np.repeat(np.arange(len(utt_lens)), pat_counts)
        assert utt.size == len(seqs)
        out = [wild_spot(zs[u], s, f) for u, s, f in zip(utt, seqs, flags)]
        cuts = np.cumsum(pat_counts)[:-1]
        free = np.array([wild_align(z, [], None)[2] for z in zs], dtype=np.float32)
        return (np.split(np.array([o[0] for o in out], dtype=np.float32), cuts),
                np.split(np.array([o[1] for o in out], dtype=np.int32), cuts),
                np.split(np.array([o[2] for o in out], dtype=np.int32), cuts), free)

    def ctc_spot(self, X, utt_lens, pat_counts, labels, label_lens, wild=None):
        self.calls.append(("spot", len(utt_lens), int(np.sum(pat_counts))))
        return self._spot(X, utt_lens, pat_counts, labels, label_lens, wild)

    def ctc_spot_raw(self, raw, utt_lens, context_width, pat_counts, labels, label_lens, wild=None, cmvn=None):
        assert context_width == 0 and cmvn is None
        self.calls.append(("spot_raw", len(utt_lens), int(np.sum(pat_counts))))
        return self._spot(raw, utt_lens, pat_counts, labels, label_lens, wild)


def _decoder(engine, max_length=64):
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    dec = Decoder.__new__(Decoder)  # (the constructor creates a device engine)
    dec.engine, dec.max_length = engine, max_length
    return dec


def _same_alis(a, b):
    return all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a, b))


def test_decoder_ctc_align_wild_over_a_stand_in_engine():
    from tfkaldi_amd.neuralNetworks.decoder import ctc_segments
    from tfkaldi_amd.processing.feature_reader import Unspliced
    rng = np.random.default_rng(703)
    lens = [30, 2, 17, 0, 9]
    xs = [rng.standard_normal((n, F)).astype(np.float32) for n in lens]
    ys = [rng.integers(0, O - 1, size=k) for k in (6, 3, 0, 0, 2)]  # the second utterance is too short for its labels
    eng = NumpyWildEngine()
    dec = _decoder(eng)
    alis, scores, free = dec.ctc_align_wild(xs, ys)  # the default: both ends wild
    assert eng.calls == [("align", 5)]  # every utterance in ONE pass
    assert scores.dtype == np.float32 and scores.shape == (5,) and free.dtype == np.float32 and free.shape == (5,)
    assert alis[1] is None and scores[1] == -np.inf and alis[3].size == 0 and scores[3] == 0.0 and free[3] == 0.0
    forms = {"ends": "ends", "all": "all", "none": None,
             "arrays": [rng.integers(0, 2, size=y.size + 1).astype(bool) for y in ys]}
    for name, wild in forms.items():
        got = dec.ctc_align_wild(xs, ys, wild=wild)
        for u in range(5):
            want = wild_align(xs[u] @ eng.W, ys[u], wild[u] if name == "arrays" else wild)
            assert (got[0][u] is None and want[0] is None) or np.array_equal(got[0][u], want[0]), (name, u)
            assert got[1][u] == np.float32(want[1]) and got[2][u] == np.float32(want[2]), (name, u)
            assert got[1][u] <= got[2][u]
            if got[0][u] is not None:
                assert [k for k, _, _ in ctc_segments(got[0][u], ys[u])] == ys[u].tolist()  # ctc_segments works unchanged
    assert _same_alis(dec.ctc_align_wild(xs, ys, wild="ends")[0], alis)
    plain = [viterbi_align(x @ eng.W, y) for x, y in zip(xs, ys)]
    none = dec.ctc_align_wild(xs, ys, wild=None)
    assert _same_alis(none[0], [a for a, _ in plain]) and np.all(none[1] <= scores)
    # all Unspliced: the device-splice entry, one pass
    eng.calls = []
    raw = dec.ctc_align_wild([Unspliced(x, 0) for x in xs], ys)
    assert eng.calls == [("align_raw", 5)]
    assert _same_alis(raw[0], alis) and raw[1].tobytes() == scores.tobytes() and raw[2].tobytes() == free.tobytes()
    mixed = dec.ctc_align_wild([Unspliced(xs[0], 0)] + xs[1:], ys)  # mixed: spliced on the host, stacked
    assert eng.calls[-1] == ("align", 5) and mixed[1].tobytes() == scores.tobytes()
    got = dec.ctc_align_wild([], [])
    assert got[0] == [] and all(g.shape == (0,) and g.dtype == np.float32 for g in got[1:])
    for bad in (dict(targets=ys[:-1]), dict(wild="middle"), dict(wild=forms["arrays"][:-1]),
                dict(wild=[np.zeros(y.size + 2, bool) for y in ys])):
        with pytest.raises(ValueError):
            dec.ctc_align_wild(xs, bad.get("targets", ys), wild=bad.get("wild", "ends"))
    with pytest.raises(ValueError):  # longer than the decoder's max_length, as every Decoder entry
        _decoder(eng, max_length=20).ctc_align_wild(xs, ys)


def test_decoder_ctc_spot_over_a_stand_in_engine():
    from tfkaldi_amd.processing.feature_reader import Unspliced
    rng = np.random.default_rng(704)
    lens = [30, 2, 17, 0, 9]
    xs = [rng.standard_normal((n, F)).astype(np.float32) for n in lens]
    pats = [rng.integers(0, O - 1, size=k) for k in (2, 0, 5, 1)]
    eng = NumpyWildEngine()
    dec = _decoder(eng)
    forms = {"ends": "ends", "all": "all", "none": None,
             "arrays": [rng.integers(0, 2, size=p.size + 1).astype(bool) for p in pats]}
    for name, wild in forms.items():
        eng.calls = []
        scores, starts, ends, free = dec.ctc_spot(xs, pats, wild=wild)
        assert eng.calls == [("spot", 5, 20)]  # U x K pairs in ONE pass
        assert scores.shape == starts.shape == ends.shape == (5, 4) and free.shape == (5,)
        assert scores.dtype == free.dtype == np.float32 and starts.dtype == ends.dtype == np.int32
        for k in range(4):  # every (u, k) is ctc_align_wild of that utterance and pattern
            alis, sc, fr = dec.ctc_align_wild(xs, [pats[k]] * 5, wild=[wild[k]] * 5 if name == "arrays" else wild)
            assert sc.tobytes() == scores[:, k].tobytes() and fr.tobytes() == free.tobytes(), (name, k)
            assert [span(a) for a in alis] == list(zip(starts[:, k].tolist(), ends[:, k].tolist())), (name, k)
        assert np.all(scores <= free[:, None])
    assert np.all(scores[3] == [-np.inf, 0.0, -np.inf, -np.inf]) and starts[3].tolist() == [-1, 0, -1, -1]  # no frames
    assert scores[1, 2] == -np.inf and (starts[1, 2], ends[1, 2]) == (-1, -1)  # 5 labels in 2 frames
    eng.calls = []
    raw = dec.ctc_spot([Unspliced(x, 0) for x in xs], pats, wild=forms["arrays"])
    assert eng.calls == [("spot_raw", 5, 20)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(raw, (scores, starts, ends, free)))
    got = dec.ctc_spot([], pats)
    assert [g.shape for g in got] == [(0, 4), (0, 4), (0, 4), (0,)]
    got = dec.ctc_spot(xs, [])  # no pattern: the pass still gives free
    assert [g.shape for g in got] == [(5, 0), (5, 0), (5, 0), (5,)] and got[3].tobytes() == free.tobytes()
    for bad in ("middle", forms["arrays"][:-1], [np.zeros(p.size + 2, bool) for p in pats]):
        with pytest.raises(ValueError):
            dec.ctc_spot(xs, pats, wild=bad)
    with pytest.raises(ValueError):
        _decoder(eng, max_length=20).ctc_spot(xs, pats)
