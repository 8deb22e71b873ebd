"""CTC forced alignment on the device (tfk_ctc_align / tfk_ctc_align_raw / tfk_ctc_align_logits, csrc/ctc.hip) against the
float64 numpy restatement of tests/test_ctc_align_host.py applied to the SAME logits (the engine's own, or chosen ones
through the stand-alone entry).

Paths: on integer logits every fp32 intermediate of the recursion is exact, so the device's alignment must EQUAL the
restatement's, ties included.  On the engine's own logits the device's path must be valid and its float64 score no worse
than the float64 optimum minus `tol`.  Scores: within `tol` = 4 x the largest |float32 run - float64 run| of the
RESTATEMENT's score on the same inputs (the rule of test_gpu_ctc_beam.py; the factor covers another legitimate fp32
evaluation order), floored at 1e-6 x |score|."""
from ctypes import c_void_p

import numpy as np
import pytest

from test_ctc_align_host import check_valid, integer_logits, path_score, row_lse, viterbi_align
from test_ctc_beam_host import ctc_log_prob
from test_gpu_ctc_beam import KW, _sharpen
from test_gpu_ctc_decode import _refs, _split, _toy_ctc
from util import make_pair

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _device_align_logits(z, utt, refs, lead=3, tail=5):
    """tfk_ctc_align_logits on host logits whose utterances start at row `lead` of a [lead + sum(utt) + tail, O] matrix:
    (the utterances' slices of ali, scores [U]); the rows outside every utterance must keep their sentinel"""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    O, U = z.shape[1], len(utt)
    T = lead + z.shape[0] + tail
    full = np.full((T, O), 50.0, np.float32)  # (what surrounds the utterances must not matter)
    full[lead:lead + z.shape[0]] = z
    seg = (lead + np.concatenate([[0], np.cumsum(utt)])).astype(np.int32)
    lab_off = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
    labels = np.concatenate([np.asarray(r, np.int32) for r in refs] + [np.zeros(1, np.int32)])
    dev = lambda a: torch.from_numpy(a).cuda()
    d_z, d_seg, d_off, d_lab = dev(full), dev(seg), dev(lab_off), dev(labels)
    ali = torch.full((T,), SENTINEL, dtype=torch.int32, device="cuda")
    score = torch.full((U,), 12345.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tfk_ctc_align_logits(c_void_p(stream), c_void_p(d_z.data_ptr()), O, O, T, c_void_p(d_seg.data_ptr()), U,
                                        c_void_p(d_lab.data_ptr()), c_void_p(d_off.data_ptr()), c_void_p(ali.data_ptr()),
                                        c_void_p(score.data_ptr())))
    torch.cuda.synchronize()
    ali, score = ali.cpu().numpy(), score.cpu().numpy()
    assert np.all(ali[:lead] == SENTINEL) and np.all(ali[seg[-1]:] == SENTINEL)
    return [ali[seg[u]:seg[u + 1]].copy() for u in range(U)], score


def _restatement(zs, refs):
    """per utterance the float64 (ali, score) of the restatement, and tol from its own float32 run"""
    r64 = [viterbi_align(z, r) for z, r in zip(zs, refs)]
    s64 = np.array([s for _, s in r64])
    s32 = np.array([viterbi_align(z, r, np.float32)[1] for z, r in zip(zs, refs)])
    finite = np.isfinite(s64)
    assert np.array_equal(finite, np.isfinite(s32))
    diff = np.abs(s32[finite] - s64[finite]).max() if finite.any() else 0.0
    return [a for a, _ in r64], s64, np.maximum(4.0 * diff, 1e-6 * np.abs(np.where(finite, s64, 0.0)))


def _check_exact(name, utt, refs, seed):
    """integer logits: the device's alignment EQUALS the restatement's for every utterance, the score is within tol"""
    rng = np.random.default_rng(seed)
    O = 9
    z = integer_logits(rng, sum(utt), O)
    zs = np.split(z, np.cumsum(utt)[:-1])
    alis, scores = _device_align_logits(z, utt, refs)
    want, s64, tol = _restatement(zs, refs)
    worst = 0.0
    for u in range(len(utt)):
        if want[u] is None:
            assert scores[u] == -np.inf and np.all(alis[u] == -2), (name, u, utt[u], len(refs[u]))
            continue
        assert np.array_equal(alis[u], want[u]), (name, u, utt[u], len(refs[u]), np.nonzero(alis[u] != want[u])[0][:8])
        exact = path_score(zs[u], refs[u], alis[u]) if utt[u] else 0.0
        err = abs(float(scores[u]) - exact)
        worst = max(worst, err)
        assert err <= tol[u], (name, u, scores[u], exact, tol[u])
    print("%s: %d utterances, largest |device - float64| %.3e, tol %.3e ... %.3e" % (name, len(utt), worst, tol.min(), tol.max()))


def _labels(rng, S, repeats=0, O=9):
    """S labels in [0, O - 1) without equal neighbours, then `repeats` positions made equal to their predecessor"""
    lab = rng.integers(0, O - 1, size=S)
    for j in range(1, S):
        while lab[j] == lab[j - 1]:
            lab[j] = rng.integers(0, O - 1)
    for j in rng.choice(np.arange(1, S), size=repeats, replace=False) if repeats else ():
        lab[j] = lab[j - 1]
    return lab.astype(np.int32)


def _min_frames(lab):
    return len(lab) + int(np.sum(np.asarray(lab[1:]) == np.asarray(lab[:-1])))


def test_exact_paths_on_integer_logits_every_frame_count(gpu):
    """frame counts around the prefetch ring (8) and the 64-frame backtrace blocks; empty references, runs of one label, an
    exactly feasible utterance, the same one frame short, a zero-frame utterance in the middle of the batch"""
    rng = np.random.default_rng(300)
    utt, refs = [], []
    for Tn in (1, 2, 3, 7, 8, 9, 10, 16, 17, 63, 64, 65, 127, 128, 129, 300):
        utt.append(Tn)
        refs.append(_labels(rng, int(rng.integers(1, min(Tn // 3, 60) + 1)) if Tn >= 3 else Tn - 1))
    utt += [40, 0, 0, 50, 33, 64]
    refs += [np.zeros(0, np.int32), np.zeros(0, np.int32), np.array([2], np.int32), np.array([4] * 7 + [1] + [4] * 9, np.int32),
             np.array([5] * 17, np.int32), _labels(rng, 21, repeats=6)]
    tight = _labels(rng, 30, repeats=11)
    utt += [_min_frames(tight), _min_frames(tight) - 1, 2 * 63 + 1, 126]
    refs += [tight, tight, _labels(rng, 63), np.array([3] * 63, np.int32)]
    assert max(len(r) for r in refs) == 63  # the smallest register tile
    _check_exact("frame counts", utt, refs, 301)


@pytest.mark.parametrize("S", [64, 127, 128, 255, 256, 511])
def test_exact_paths_on_integer_logits_every_register_tile(gpu, S):
    """the longest reference on both sides of every register tile (63 is covered above) and the limit: just enough frames,
    slack, repeats, one frame short, beside short utterances"""
    rng = np.random.default_rng(S)
    plain, rep = _labels(rng, S), _labels(rng, S, repeats=S // 5)
    utt = [S, 2 * S + 37, _min_frames(rep), _min_frames(rep) + 70, _min_frames(rep) - 1, 5, 0, 3 * S // 2]
    refs = [plain, plain, rep, rep, rep, np.array([1, 1], np.int32), plain[:1], np.array([6] * (S // 2), np.int32)]
    _check_exact("S=%d" % S, utt, refs, 310 + S)


def _engine_case(dtype, O, seed):
    rng = np.random.default_rng(seed)
    eng, _ = make_pair(rng, max_frames=512, compute_dtype=dtype, **dict(KW, output_dim=O))
    _sharpen(eng, rng, 6.0, 3.0)
    utt = [30, 0, 1, 77, 140, 2, 0, 65]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    labels, lab = _refs(np.random.default_rng(seed + 1), len(utt), O, 0, 20)  # (some too long for the 0 / 1 / 2 frames)
    return eng, utt, X, labels, lab


@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
@pytest.mark.parametrize("O", [9, 36])
def test_engine_entry_on_the_engines_logits(gpu, dtype, O):
    """every returned alignment is a valid path whose float64 score is the optimum within tol, the returned score is that
    float64 score within tol, and it never exceeds log p(labels); an utterance without a path is None with -inf"""
    eng, utt, X, labels, lab = _engine_case(dtype, O, 400 + O)
    zs = np.split(eng.posteriors(X, raw_logits=True), np.cumsum(utt)[:-1])
    refs = _split(labels, lab)
    alis, scores = eng.ctc_align(X, utt, labels, lab)
    assert scores.dtype == np.float32 and scores.shape == (len(utt),)
    want, s64, tol = _restatement(zs, refs)
    feasible = 0
    for u in range(len(utt)):
        if want[u] is None:
            assert alis[u] is None and scores[u] == -np.inf, (u, utt[u], lab[u])
            continue
        feasible += 1
        assert alis[u].shape == (utt[u],)
        check_valid(alis[u], refs[u], O)
        mine = path_score(zs[u], refs[u], alis[u]) if utt[u] else 0.0
        total = ctc_log_prob(zs[u], refs[u])
        print("%s O=%d utt %d: T %d labels %d device %.6f its path in float64 %.6f optimum %.6f log p %.6f tol %.2e"
              % (dtype, O, u, utt[u], lab[u], scores[u], mine, s64[u], total, tol[u]))
        assert mine >= s64[u] - tol[u], (u, mine, s64[u], tol[u])
        assert abs(float(scores[u]) - mine) <= tol[u], (u, scores[u], mine, tol[u])
        assert float(scores[u]) <= total + tol[u], (u, scores[u], total)
    assert feasible >= 4
    again = eng.ctc_align(X, utt, labels, lab)  # two identical calls are bit-identical
    assert again[1].tobytes() == scores.tobytes()
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(again[0], alis))
    eng.close()


def test_score_is_bounded_by_the_loss(gpu):
    """score[u] <= log p(labels_u): the best alignment is one term of the sum the loss takes over all alignments"""
    rng = np.random.default_rng(500)
    utt = [60, 9, 131, 200]
    refs = [_labels(rng, 12, repeats=3), _labels(rng, 4), _labels(rng, 40, repeats=5), np.zeros(0, np.int32)]
    z = (2.0 * rng.standard_normal((sum(utt), 9))).astype(np.float32)
    zs = np.split(z, np.cumsum(utt)[:-1])
    alis, scores = _device_align_logits(z, utt, refs)
    _, s64, tol = _restatement(zs, refs)
    for u in range(len(utt)):
        total = ctc_log_prob(zs[u], refs[u])
        print("utt %d: alignment %.6f, log p(labels) %.6f, tol %.2e" % (u, scores[u], total, tol[u]))
        assert np.isfinite(scores[u]) and float(scores[u]) <= total + tol[u]
        check_valid(alis[u], refs[u], 9)
    assert abs(float(scores[3]) - ctc_log_prob(zs[3], refs[3])) <= tol[3]  # no labels: one alignment, the two are equal


def test_alignment_to_the_best_path_is_the_best_path(gpu):
    """aligned to the hypothesis tfk_ctc_greedy returns, the path is the per-frame argmax: its score is the sum of the row
    maxima of the log-softmax, and on frames whose row maximum is unique the emitted class is that argmax"""
    eng, utt, X, _, _ = _engine_case("float32", 9, 600)
    hyps, _ = eng.ctc_greedy(X, utt)
    assert sum(h.size for h in hyps) > 20
    lens = [h.size for h in hyps]
    alis, scores = eng.ctc_align(X, utt, np.concatenate(hyps), lens)
    zs = np.split(eng.posteriors(X, raw_logits=True), np.cumsum(utt)[:-1])
    _, s64, tol = _restatement(zs, hyps)
    for u in range(len(utt)):
        z = zs[u].astype(np.float64)
        want = float((z.max(axis=1) - row_lse(z)).sum()) if utt[u] else 0.0
        assert alis[u] is not None and abs(float(scores[u]) - want) <= tol[u], (u, scores[u], want, tol[u])
        unique = (z == z.max(axis=1, keepdims=True)).sum(axis=1) == 1
        cls = np.where(alis[u] >= 0, hyps[u][np.maximum(alis[u], 0)] if hyps[u].size else 0, 8)
        assert np.array_equal(cls[unique], z.argmax(axis=1)[unique]), u
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
    labels, lab = _refs(np.random.default_rng(9), len(utts), 12, 0, 15)
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)

    def same(a, b):
        return (all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a[0], b[0]))
                and a[1].tobytes() == b[1].tobytes())

    host = eng.ctc_align(np.concatenate([u.spliced() for u in utts]), lens, labels, lab)
    dev = eng.ctc_align_raw(raw, lens, C, labels, lab, cmvn=cmvn_table(utts))
    cuda = eng.ctc_align_raw(torch.from_numpy(raw).cuda(), lens, C, labels, lab, cmvn=cmvn_table(utts))
    assert same(host, dev) and same(host, cuda)
    assert sum(a is not None for a in host[0]) >= 3 and any(a is not None and np.any(a >= 0) for a in host[0])
    eng.close()


def test_limits_are_reported_and_leave_the_engine_usable(gpu):
    import torch
    from tfkaldi_amd import _lib
    rng = np.random.default_rng(13)
    eng, _ = make_pair(rng, max_frames=1024, **KW)
    O = KW["output_dim"]
    utt = np.array([600, 15], np.int32)
    X = rng.standard_normal((615, KW["input_dim"])).astype(np.float32)
    labels, lab = _refs(rng, 2, O, 3, 6)
    good = eng.ctc_align(X, utt, labels, lab)
    ptr = lambda a, on=True: a.ctypes.data_as(c_void_p) if on else c_void_p(None)

    def call(ali=True, score=True, flags=0, lab_vals=labels, lab_lens=lab, lens=utt, X_on=True, lab_on=True, T=615):
        a, s = np.empty(615, np.int32), np.empty(2, np.float32)
        lv, ll = np.ascontiguousarray(lab_vals, np.int32), np.ascontiguousarray(lab_lens, np.int32)
        ul = np.ascontiguousarray(lens, np.int32)
        return eng.lib.tfk_ctc_align(eng._h, ptr(X, X_on), X.shape[1], T, ptr(ul), 2, ptr(lv, lab_on), ptr(ll, lab_on),
                                     ptr(a, ali), ptr(s, score), flags)

    big = rng.integers(0, O - 1, size=512).astype(np.int32)
    cases = [
        ("512 labels", dict(lab_vals=np.concatenate([big, labels[lab[0]:]]), lab_lens=[512, lab[1]]), b"511"),
        ("label >= O - 1", dict(lab_vals=np.where(np.arange(labels.size) == lab[0], O - 1, labels)), b"utterance 1"),
        ("negative label", dict(lab_vals=np.where(np.arange(labels.size) == 0, -1, labels)), b"utterance 0"),
        ("negative label count", dict(lab_lens=[-1, lab[1]]), b"negative"),
        ("negative frame count", dict(lens=[616, -1]), b"negative"),
        ("NULL ali", dict(ali=False), b"NULL"), ("NULL score", dict(score=False), b"NULL"),
        ("NULL X", dict(X_on=False), b"NULL"), ("NULL labels", dict(lab_on=False), b"NULL"),
        ("T = 0", dict(T=0), b"T = 0"), ("utt_len does not sum to T", dict(T=614), b"sum"),
        ("unknown flag", dict(flags=_lib.DEVICE_PTRS), b"flags"), ("raw-only flag", dict(flags=_lib.RAW_DEVICE), b"flags"),
    ]
    for name, kw, word in cases:
        assert call(**kw) != 0, name
        assert word in eng.lib.tfk_last_error(), (name, eng.lib.tfk_last_error())
        again = eng.ctc_align(X, utt, labels, lab)  # the next valid call succeeds, with the same result
        assert again[1].tobytes() == good[1].tobytes() and all(np.array_equal(a, b) for a, b in zip(again[0], good[0])), name
    assert call() == 0
    with pytest.raises(ValueError):
        eng.ctc_align(X, utt, labels, lab[:1])
    eng.close()
    # the stand-alone entry: more than 511 labels, a negative length, labels that would start in front of `labels`
    lib = _lib.load()
    z = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros(8, dtype=torch.int32, device="cuda")
    tab = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    lab_dev = torch.zeros(600, dtype=torch.int32, device="cuda")
    for seg, off, word in (([0, 8], [0, 512], b"511"), ([0, 8, 6], [0, 1, 2], b"negative"), ([0, 4, 8], [0, 2, 1], b"negative"),
                           ([0, 8], [-1, 1], b"lab_off[0]")):
        d_seg, d_off = tab(seg), tab(off)
        assert lib.tfk_ctc_align_logits(c_void_p(0), c_void_p(z.data_ptr()), 4, 4, 8, c_void_p(d_seg.data_ptr()), len(seg) - 1,
                                        c_void_p(lab_dev.data_ptr()), c_void_p(d_off.data_ptr()), c_void_p(out.data_ptr()),
                                        c_void_p(out.data_ptr())) != 0
        assert word in lib.tfk_last_error(), (seg, off, lib.tfk_last_error())
    assert lib.tfk_ctc_align_logits(c_void_p(0), c_void_p(z.data_ptr()), 4, 4, 8, c_void_p(None), 1, c_void_p(lab_dev.data_ptr()),
                                    c_void_p(out.data_ptr()), c_void_p(out.data_ptr()), c_void_p(out.data_ptr())) != 0
    assert b"NULL" in lib.tfk_last_error()


def test_decoder_and_segments_end_to_end(gpu, tmp_path):
    from tfkaldi_amd.neuralNetworks.decoder import Decoder, ctc_segments
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    for _ in range(60):
        tr.update(xs, ys)
    targets = [np.asarray(y).astype(np.int32) for y in ys]
    want = tr.engine.ctc_align(np.concatenate(xs), [len(x) for x in xs], np.concatenate(targets), [t.size for t in targets])
    tr.save_model(str(tmp_path / "model"))
    tr.close()
    dec = Decoder(dnn, F, maxlen)
    dec.restore(str(tmp_path / "model"))
    alis, scores = dec.ctc_align(xs, ys)
    assert scores.tobytes() == want[1].tobytes() and np.all(np.isfinite(scores)) and np.all(scores < 0)
    O = coder.num_labels + 1
    for x, t, a, w in zip(xs, targets, alis, want[0]):
        assert np.array_equal(a, w) and a.shape == (len(x),)
        check_valid(a, t, O)
        segs = ctc_segments(a, t)
        assert [k for k, _, _ in segs] == t.tolist()  # one per label, in order
        assert all(0 <= b < e <= len(x) for _, b, e in segs)  # inside the utterance, not empty
        assert all(p[2] <= q[1] for p, q in zip(segs[:-1], segs[1:]))  # ordered and disjoint
        assert sum(e - b for _, b, e in segs) == int(np.sum(a >= 0))
    got = dec.ctc_align([], [])
    assert got[0] == [] and got[1].shape == (0,)
    dec.close()
