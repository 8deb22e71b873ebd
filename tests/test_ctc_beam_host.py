"""CTC prefix beam search, CPU tier: the numpy restatement the GPU tests check the engine against (the algorithm stated in
include/tfkaldi_hip.h at tfk_ctc_beam: Graves 2012 / Hannun et al. 2014 without a language model, the conventions of
tf.nn.ctc_beam_search_decoder(merge_repeated=False)), pinned by exhaustive enumeration of all alignments, by known answers
and by re-scoring with the CTC oracle; and the product's label_errors(beam_width=) over two gloo ranks driving a numpy
stand-in engine."""
import itertools
import os
import sys

import numpy as np
import pytest

from test_ctc_decode_host import _free_port, _one_hot, best_path, levenshtein

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def log_softmax(z):
    z = z - z.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


class _Trie(object):
    """label sequences as integer ids: (parent id, label) -> id; id 0 is the empty prefix"""

    def __init__(self):
        self.child, self.parent, self.label, self.length = {}, [-1], [-1], [0]

    def extend(self, p, c):
        key = (p, c)
        q = self.child.get(key)
        if q is None:
            q = self.child[key] = len(self.parent)
            self.parent.append(p)
            self.label.append(c)
            self.length.append(self.length[p] + 1)
        return q

    def labels(self, q):
        out = []
        while q:
            out.append(self.label[q])
            q = self.parent[q]
        return tuple(out[::-1])


def _beam_one(lp, W, dtype):
    """one utterance: log-probabilities lp [T, O] in `dtype` -> [(labels tuple, total score)] of the final beam, best first
    (order: higher score, then shorter, then lexicographically smaller).  Every step is one [beam, O] candidate array."""
    T, O = lp.shape
    blank = O - 1
    ninf = dtype(-np.inf)
    trie = _Trie()
    ids = [0]
    pb, pnb = np.zeros(1, dtype), np.full(1, ninf, dtype)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            row = lp[t]
            nb = len(ids)
            tot = np.logaddexp(pb, pnb)
            last = np.array([trie.label[q] for q in ids])
            has = last >= 0
            base = np.repeat(tot[:, None], O - 1, axis=1)
            base[has, last[has]] = pb[has]  # a repeated label extends only the alignments that end in a blank
            ext = base + row[None, :blank]
            stay_pb = tot + row[blank]
            stay_pnb = np.where(has, pnb + row[np.where(has, last, 0)], ninf).astype(dtype)
            alive = np.ones((nb, O), dtype=bool)  # column `blank` is the stay candidate
            slot = {q: i for i, q in enumerate(ids)}
            for j, q in enumerate(ids):  # an extension that IS a beam prefix merges into that prefix's stay candidate
                i = slot.get(trie.parent[q]) if q else None
                if i is not None:
                    stay_pnb[j] = np.logaddexp(stay_pnb[j], ext[i, last[j]])
                    alive[i, last[j]] = False
            cand = np.concatenate([ext, np.logaddexp(stay_pb, stay_pnb)[:, None]], axis=1)
            ii, cc = np.nonzero(alive)
            sc = cand[ii, cc]
            if sc.size > W:
                thr = np.partition(sc, sc.size - W)[sc.size - W]
                sure = np.nonzero(sc > thr)[0]
                tied = np.nonzero(sc == thr)[0]
                if sure.size + tied.size > W:  # the W-th place is tied: shorter, then lexicographically smaller
                    seq = lambda k: trie.labels(ids[ii[k]]) + (() if cc[k] == blank else (int(cc[k]),))
                    tied = np.array(sorted(tied, key=lambda k: (len(seq(k)), seq(k)))[:W - sure.size], dtype=np.int64)
                keep = np.sort(np.concatenate([sure, tied]))
                if keep.size < W:  # NaN scores: fill up with whatever is left, so that the beam stays full
                    rest = np.setdiff1d(np.arange(sc.size), keep)[:W - keep.size]
                    keep = np.sort(np.concatenate([keep, rest]))
                ii, cc = ii[keep], cc[keep]
            stay = cc == blank
            new_ids = [ids[i] if s else trie.extend(ids[i], int(c)) for i, c, s in zip(ii, cc, stay)]
            new_pb = np.where(stay, stay_pb[ii], ninf).astype(dtype)
            new_pnb = np.where(stay, stay_pnb[ii], ext[ii, np.where(stay, 0, cc)]).astype(dtype)
            ids, pb, pnb = new_ids, new_pb, new_pnb
        tot = np.logaddexp(pb, pnb)
    final = [(trie.labels(q), float(s)) for q, s in zip(ids, tot)]
    final.sort(key=lambda e: (-e[1], len(e[0]), e[0]))
    return final


def prefix_beam_search(logits, utt_lens, W, top_paths, dtype=np.float64):
    """numpy restatement of tfk_ctc_beam on logits [sum(utt_lens), O]: (hyps, scores) with hyps[u][n] int32 arrays, best
    first, scores float64 [U, top_paths]; missing paths are empty with score -inf.  dtype: the arithmetic of the recursion."""
    logits = np.asarray(logits)
    hyps, scores, t0 = [], np.full((len(utt_lens), top_paths), -np.inf), 0
    for u, n in enumerate(utt_lens):
        final = _beam_one(log_softmax(logits[t0:t0 + n].astype(dtype)), W, dtype)[:top_paths]
        t0 += n
        hyps.append([np.array(h, dtype=np.int32) for h, _ in final] + [np.zeros(0, np.int32)] * (top_paths - len(final)))
        scores[u, :len(final)] = [s for _, s in final]
    return hyps, scores


def ctc_log_prob(logits, labels):
    """log p(labels | logits) in float64: the forward recursion of the CTC loss, one numpy row per frame"""
    lp = log_softmax(np.asarray(logits, dtype=np.float64))
    T, O = lp.shape
    ext = np.full(2 * len(labels) + 1, O - 1, dtype=np.int64)
    ext[1::2] = labels
    if T == 0:
        return 0.0 if len(labels) == 0 else -np.inf
    skip = np.zeros(ext.size, dtype=bool)
    skip[2:] = (ext[2:] != O - 1) & (ext[2:] != ext[:-2])
    a = np.full(ext.size, -np.inf)
    a[:2] = lp[0, ext[:2]]
    for t in range(1, T):
        s1 = np.concatenate([[-np.inf], a[:-1]])
        s2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], a[:-2]])[:a.size], -np.inf)
        a = np.logaddexp(np.logaddexp(a, s1), s2) + lp[t, ext]
    return float(np.logaddexp(a[-1], a[-2]) if ext.size > 1 else a[-1])


def enumerate_labellings(logits):
    """{labelling: log-probability} by summing all O^T alignments in float64 (tiny T only)"""
    lp = log_softmax(np.asarray(logits, dtype=np.float64))
    T, O = lp.shape
    acc = {}
    for path in itertools.product(range(O), repeat=T):
        lab = tuple(k for k, prev in zip(path, (-1,) + path[:-1]) if k != O - 1 and k != prev)
        acc.setdefault(lab, []).append(sum(lp[t, k] for t, k in enumerate(path)))
    return {lab: float(np.logaddexp.reduce(np.array(v))) for lab, v in acc.items()}


def enumeration_cases(count=40, T=6, seed=100):
    rng = np.random.default_rng(seed)
    return [2.0 * rng.standard_normal((T, 3)) for _ in range(count)]


def peaky_logits(rng, T, O, labels_per_utt, scale=6.0):
    """host-made logits of the decode benchmark's kind: a few frames per label stand out, the blank dominates the rest"""
    z = rng.standard_normal((T, O)) * 1.5
    z[:, O - 1] += scale
    for t in rng.choice(T, size=labels_per_utt, replace=False):
        z[t, rng.integers(0, O - 1)] += 2.0 * scale * rng.random() + 0.5 * scale
    return z.astype(np.float32)


def test_ctc_log_prob_equals_the_oracle():
    from oracle.ctc_oracle import ctc_loss_and_grad
    rng = np.random.default_rng(1)
    for T, O, S in ((7, 4, 3), (12, 5, 0), (9, 3, 6), (5, 6, 1)):
        z = 2.0 * rng.standard_normal((T, O))
        lab = rng.integers(0, O - 1, size=S)
        if S == 6:
            lab[2] = lab[3]  # a repeated label
        want = -ctc_loss_and_grad(z, lab)[0]
        assert abs(ctc_log_prob(z, lab) - want) <= 1e-12 * max(1.0, abs(want))
    assert ctc_log_prob(np.zeros((2, 3)), [0, 0]) == -np.inf  # too short: a a needs three frames
    assert ctc_log_prob(np.zeros((0, 3)), []) == 0.0


def test_unpruned_beam_equals_exhaustive_enumeration():
    """2 labels + blank, T = 6: at most 127 prefixes, W = 128 prunes nothing -- the N-best list is the enumeration's"""
    for z in enumeration_cases():
        want = sorted(enumerate_labellings(z).items(), key=lambda e: (-e[1], len(e[0]), e[0]))
        hyps, scores = prefix_beam_search(z, [6], 128, 127)
        n = len(want)  # the labellings that fit into 6 frames; the beam's other prefixes have probability zero
        assert [tuple(h.tolist()) for h in hyps[0][:n]] == [lab for lab, _ in want]
        assert np.abs(scores[0, :n] - np.array([s for _, s in want])).max() <= 1e-12
        assert n < 127 and np.all(scores[0, n:] == -np.inf)
        assert want[0][1] - want[1][1] > 1e-3  # (so the GPU version of this test needs no exclusions)
        assert abs(np.logaddexp.reduce(scores[0])) < 1e-12  # the labellings' probabilities sum to one


def test_known_answers():
    O, b = 4, 3
    big = lambda classes: 20.0 * _one_hot(classes, O)
    best = lambda z, lens, W=8: [h[0].tolist() for h in prefix_beam_search(z, lens, W, 1)[0]]
    assert best(big([b, b, b]), [3]) == [[]]           # blank-dominant frames: the empty path
    assert best(big([1, 1]), [2]) == [[1]]             # a a -> a
    assert best(big([1, b, 1]), [3]) == [[1, 1]]       # a blank a -> a a
    assert best(big([2, 2, 2, b]), [2, 0, 2]) == [[2], [], [2]]  # boundaries; a zero-frame utterance
    hyps, scores = prefix_beam_search(big([1]), [0, 1], 8, 3)
    assert [h.tolist() for h in hyps[0]] == [[], [], []] and scores[0].tolist() == [0.0, -np.inf, -np.inf]
    assert [h.tolist() for h in hyps[1]][0] == [1] and np.isfinite(scores[1]).all()  # (), (0), (1), (2) survive one frame
    # one frame, W = 2: two prefixes survive, the third path is padding
    hyps, scores = prefix_beam_search(big([1]), [1], 2, 2)
    assert len(hyps[0]) == 2 and np.isfinite(scores[0]).all()
    # W = 1 on one-hot-like logits is best-path decoding
    rng = np.random.default_rng(2)
    classes = rng.integers(0, O, size=60)
    z = big(classes) + rng.standard_normal((60, O)).astype(np.float32)
    lens = [25, 0, 35]
    assert best(z, lens, 1) == [h.tolist() for h in best_path(z, lens)]


def test_beam_beats_best_path():
    """two frames, p(a) = 0.4, p(blank) = 0.6 each: the best alignment is blank blank (0.36), but a has three alignments
    (a a, a blank, blank a: 0.16 + 0.24 + 0.24 = 0.64)"""
    z = np.log(np.array([[0.4, 0.6], [0.4, 0.6]]))
    assert [h.tolist() for h in best_path(z, [2])] == [[]]
    hyps, scores = prefix_beam_search(z, [2], 4, 2)
    assert [h.tolist() for h in hyps[0]] == [[0], []]
    assert np.allclose(np.exp(scores[0]), [0.64, 0.36], rtol=1e-12)
    # W = 1 follows a single prefix and still sums its alignments: () after frame 1 (0.6 > 0.4), then () again
    assert [h.tolist() for h in prefix_beam_search(z, [2], 1, 1)[0][0]] == [[]]


@pytest.mark.parametrize("W", [1, 4, 16, 64])
def test_best_hypothesis_rescored_by_the_ctc_oracle(W):
    """the beam score sums SOME alignments of the labelling: never more than its exact log-probability; equal when unpruned"""
    from oracle.ctc_oracle import ctc_loss_and_grad
    rng = np.random.default_rng(W)
    lens = [14, 9, 1]
    z = 2.0 * rng.standard_normal((sum(lens), 4))
    hyps, scores = prefix_beam_search(z, lens, W, 1)
    t0 = 0
    for u, n in enumerate(lens):
        exact = -ctc_loss_and_grad(z[t0:t0 + n], hyps[u][0])[0]
        assert abs(exact - ctc_log_prob(z[t0:t0 + n], hyps[u][0])) <= 1e-10
        assert exact >= scores[u, 0] - 1e-9
        t0 += n
    if W == 64:  # 3 labels, T = 1: 4 prefixes, nothing pruned
        assert abs(-ctc_loss_and_grad(z[23:], hyps[2][0])[0] - scores[2, 0]) <= 1e-12
    # unpruned at T = 6 (127 prefixes): equal
    z6 = 2.0 * rng.standard_normal((6, 3))
    h, s = prefix_beam_search(z6, [6], 128, 1)
    assert abs(-ctc_loss_and_grad(z6, h[0][0])[0] - s[0, 0]) <= 1e-12


def test_float32_mode_is_close_and_wider_beams_score_no_less():
    rng = np.random.default_rng(3)
    z = (2.0 * rng.standard_normal((60, 12))).astype(np.float32)
    h64, s64 = prefix_beam_search(z, [60], 16, 3)
    h32, s32 = prefix_beam_search(z, [60], 16, 3, dtype=np.float32)
    assert [h.tolist() for h in h64[0]] == [h.tolist() for h in h32[0]]
    assert np.abs(s64 - s32).max() < 1e-4
    assert prefix_beam_search(z, [60], 64, 1)[1][0, 0] >= prefix_beam_search(z, [60], 2, 1)[1][0, 0] - 1e-12


def test_peaky_cfg5_logits_have_clear_winners():
    """the condition the GPU test at cfg5 size asserts before it consults the device, on the same 16 utterances and with the
    same tol: the band of 2 tol below the best float64 score holds one hypothesis for at least 75 % of the utterances"""
    rng = np.random.default_rng(55)
    z = peaky_logits(rng, 16 * 800, 36, 16 * 100)
    lens = [800] * 16
    h64, s64 = prefix_beam_search(z, lens, 100, 8)
    _, s32 = prefix_beam_search(z, lens, 100, 1, dtype=np.float32)
    tol = np.maximum(4 * np.abs(s32[:, 0] - s64[:, 0]).max(), 1e-6 * np.abs(s64[:, 0]))
    crowded = sum(int((s64[u] >= s64[u, 0] - 2 * tol[u]).sum() > 1) for u in range(16))
    assert 4 * crowded <= 16, (tol, s64)
    assert min(h[0].size for h in h64) > 50


# ---- label_errors(beam_width=) over two gloo ranks ----
F, O = 6, 5


class NumpyBeamEngine(object):
    """stand-in for Engine's decoding entries: logits = X @ W of a fixed seeded matrix, decoded by the numpy restatements"""

    def __init__(self):
        self.W = 3.0 * np.random.default_rng(11).standard_normal((F, O)).astype(np.float32)
        self.calls = []

    def _edits(self, hyps, labels, label_lens):
        refs = np.split(np.asarray(labels), np.cumsum(label_lens)[:-1])
        return np.array([levenshtein(h, r) for h, r in zip(hyps, refs)], dtype=np.int32)

    def ctc_greedy(self, X, utt_lens, labels=None, label_lens=None):
        self.calls.append("greedy")
        hyps = best_path(np.asarray(X, dtype=np.float32) @ self.W, utt_lens)
        return hyps, self._edits(hyps, labels, label_lens)

    def ctc_greedy_raw(self, raw, utt_lens, context_width, cmvn=None, labels=None, label_lens=None):
        assert context_width == 0 and cmvn is None
        return self.ctc_greedy(raw, utt_lens, labels, label_lens)

    def ctc_beam(self, X, utt_lens, beam_width=100, top_paths=1, labels=None, label_lens=None):
        self.calls.append("beam%d" % beam_width)
        hyps, scores = prefix_beam_search(np.asarray(X, dtype=np.float32) @ self.W, utt_lens, beam_width, top_paths)
        return hyps, scores.astype(np.float32), self._edits([h[0] for h in hyps], labels, label_lens)

    def ctc_beam_raw(self, raw, utt_lens, context_width, cmvn=None, beam_width=100, top_paths=1, labels=None,
                     label_lens=None):
        assert context_width == 0 and cmvn is None
        return self.ctc_beam(raw, utt_lens, beam_width, top_paths, labels, label_lens)


def _microbatches(num_mb, seed=0):
    from tfkaldi_amd.dataparallel import CtcMicroBatch
    rng = np.random.default_rng(seed)
    out = []
    for i in range(num_mb):
        utt = [int(rng.integers(0, 30)) for _ in range(3)]
        lab = [int(rng.integers(0, 9)) for _ in range(3)]
        X = rng.standard_normal((sum(utt), F)).astype(np.float32)
        labels = rng.integers(0, O - 1, size=sum(lab)).astype(np.int32)
        out.append(CtcMicroBatch(X, np.array(utt, np.int32), labels, np.array(lab, np.int32),
                                 context_width=0 if i % 2 else None))
    return out


def _worker(rank, world, port, num_mb, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      TFK_DIST_BACKEND="gloo")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from tfkaldi_amd.dataparallel import DataParallel, init_from_env
    assert init_from_env()[:2] == (rank, world)
    dp = DataParallel()
    assert dp.enabled and dp.world == world
    got = dp.label_errors(NumpyBeamEngine(), _microbatches(num_mb), beam_width=8)
    assert all(type(v) is int for v in got)
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(got, dtype=np.int64))
    dist.destroy_process_group()


@pytest.mark.parametrize("num_mb", [4, 3, 1])  # even blocks, uneven blocks, one idle rank
def test_beam_label_errors_two_gloo_ranks_equal_serial(tmp_path, num_mb):
    import torch.multiprocessing as mp
    from tfkaldi_amd.dataparallel import DataParallel
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), num_mb, str(tmp_path)), nprocs=world, join=True)
    eng = NumpyBeamEngine()
    serial = DataParallel().label_errors(eng, _microbatches(num_mb), beam_width=8)
    assert eng.calls == ["beam8"] * num_mb
    ref = NumpyBeamEngine()
    want_edits = want_labels = 0
    for mb in _microbatches(num_mb):
        _, _, e = ref.ctc_beam(mb.X, mb.utt_lens, 8, 1, mb.labels, mb.label_lens)
        want_edits += int(e.sum())
        want_labels += int(mb.label_lens.sum())
    assert serial == (want_edits, want_labels) and want_edits > 0
    for rank in range(world):
        assert tuple(np.load(os.path.join(str(tmp_path), "rank%d.npy" % rank)).tolist()) == serial


def test_beam_width_none_is_best_path():
    from tfkaldi_amd.dataparallel import DataParallel
    eng = NumpyBeamEngine()
    none = DataParallel().label_errors(eng, _microbatches(3), beam_width=None)
    assert eng.calls == ["greedy"] * 3
    assert none == DataParallel().label_errors(NumpyBeamEngine(), _microbatches(3))
    with pytest.raises(TypeError):
        DataParallel().label_errors(eng, [(np.zeros((4, F), np.float32), np.zeros(4, np.int32))], beam_width=4)
