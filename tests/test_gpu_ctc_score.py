"""CTC N-best rescoring on the device (tfk_ctc_score / tfk_ctc_score_raw / tfk_ctc_score_logits, csrc/ctc.hip) against the
float64 numpy restatement of tests/test_ctc_score_host.py applied to the SAME logits (the engine's own, or chosen ones
through the stand-alone entry).

Tolerance everywhere: `tol` = 4 x the largest |float32 run - float64 run| of the RESTATEMENT on the same pairs (the rule of
test_gpu_ctc_align.py and test_gpu_ctc_beam.py; the factor covers another legitimate fp32 evaluation order), floored at
1e-6 x |score|, computed from the restatement alone.  Every case prints the largest |device - float64| beside it."""
from ctypes import c_void_p

import numpy as np
import pytest

from test_ctc_align_host import viterbi_align
from test_ctc_beam_host import peaky_logits, prefix_beam_search
from test_ctc_decode_host import best_path, levenshtein
from test_ctc_score_host import ctc_score_restated, rescore_tol
from test_gpu_ctc_align import _device_align_logits, _labels, _min_frames
from test_gpu_ctc_beam import KW, _sharpen
from test_gpu_ctc_beam_topk import _engine_state
from test_gpu_ctc_decode import _refs, _split, _toy_ctc
from util import make_pair

pytestmark = pytest.mark.gpu

E = np.zeros(0, np.int32)


def _device_score_logits(z, utt, hyps, lead=3, tail=5, pad=3):
    """tfk_ctc_score_logits on host logits whose utterances start at row `lead` (seg[0] > 0) of a [lead + sum(utt) + tail,
    O + pad] matrix (ld > O); hyps[u] = utterance u's list of label arrays.  Returns the scores per utterance.  What
    surrounds the utterances -- rows before and after, columns beyond O -- must not matter."""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    O, U = z.shape[1], len(utt)
    T = lead + z.shape[0] + tail
    full = np.full((T, O + pad), 50.0, np.float32)
    full[:lead, :O] = np.nan  # sentinel rows: a value read from them poisons the result
    full[lead + z.shape[0]:, :O] = np.nan
    full[lead:lead + z.shape[0], :O] = z
    seg = (lead + np.concatenate([[0], np.cumsum(utt)])).astype(np.int32)
    flat = [np.asarray(h, np.int32).reshape(-1) for hs in hyps for h in hs]
    P = len(flat)
    pair_utt = np.repeat(np.arange(U), [len(hs) for hs in hyps]).astype(np.int32)
    lab_off = np.concatenate([[0], np.cumsum([h.size for h in flat])]).astype(np.int32)
    labels = np.concatenate(flat + [np.zeros(1, np.int32)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_z, d_seg, d_utt, d_off, d_lab = dev(full), dev(seg), dev(np.concatenate([pair_utt, [0]]).astype(np.int32)), dev(lab_off), dev(labels)
    score = torch.full((P + 1,), 12345.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tfk_ctc_score_logits(c_void_p(stream), c_void_p(d_z.data_ptr()), O + pad, O, T, c_void_p(d_seg.data_ptr()), U,
                                        c_void_p(d_utt.data_ptr()), P, c_void_p(d_lab.data_ptr()), c_void_p(d_off.data_ptr()),
                                        c_void_p(score.data_ptr())))
    torch.cuda.synchronize()
    score = score.cpu().numpy()
    assert score[P] == 12345.0  # nothing is written beyond the pairs
    return np.split(score[:P], np.cumsum([len(hs) for hs in hyps])[:-1])


def _compare(name, zs, hyps, got):
    """device scores `got` (per utterance) against the restatement on the per-utterance logits zs: -inf where it says -inf,
    within tol elsewhere.  Returns (float64 scores per utterance, tol per utterance)."""
    pairs_z = [zs[u] for u, hs in enumerate(hyps) for _ in hs]
    flat = [h for hs in hyps for h in hs]
    s64, tol = rescore_tol(pairs_z, flat)
    dev = np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in got]) if flat else np.zeros(0)
    assert dev.shape == s64.shape
    worst = 0.0
    for p in range(len(flat)):
        if s64[p] == -np.inf:
            assert dev[p] == -np.inf, (name, p, zs and pairs_z[p].shape, len(flat[p]), dev[p])
            continue
        err = abs(dev[p] - s64[p])
        worst = max(worst, err)
        assert err <= tol[p], (name, p, pairs_z[p].shape[0], len(flat[p]), dev[p], s64[p], tol[p])
    print("%s: %d pairs (%d feasible), largest |device - float64| %.3e, tol %.3e ... %.3e"
          % (name, len(flat), int(np.isfinite(s64).sum()), worst, tol.min() if len(flat) else 0, tol.max() if len(flat) else 0))
    cuts = np.cumsum([len(hs) for hs in hyps])[:-1]
    return np.split(s64, cuts), np.split(tol, cuts)


def _check_logits(name, z, utt, hyps):
    zs = np.split(np.asarray(z, np.float32), np.cumsum(utt)[:-1])
    got = _device_score_logits(z, utt, hyps)
    return got, _compare(name, zs, hyps, got)


def test_frame_counts_around_the_prefetch_ring(gpu):
    """frame counts around the ring of 8 rows and beyond, one utterance of 1600 frames (the offset's precision); ld > O,
    sentinel rows before and after, seg[0] > 0 (all in _device_score_logits)"""
    rng = np.random.default_rng(1500)
    utt, hyps = [], []
    for Tn in (1, 2, 3, 7, 8, 9, 10, 16, 17, 63, 64, 65, 129, 300, 1600):
        utt.append(Tn)
        longest = max(min(Tn // 3, 60), 1)
        hyps.append([_labels(rng, int(rng.integers(1, longest + 1))) if Tn >= 3 else _labels(rng, 1), E,
                     _labels(rng, longest, repeats=min(longest // 4, max(longest - 1, 0)))])
    z = (2.0 * rng.standard_normal((sum(utt), 9))).astype(np.float32)
    got, (s64, _) = _check_logits("frame counts", z, utt, hyps)
    assert all(np.isfinite(s).all() for s in s64[3:]) and s64[-1].min() < -2000.0  # (where fp32 alone resolves only 1e-4)


def test_pair_layout_in_one_batch(gpu):
    """several pairs per utterance with different lengths, an empty hypothesis, hyp_count = 0 in the middle, a zero-frame
    utterance with S = 0 and S > 0, runs of one label, repeats, an exactly feasible pair and the same pair one frame short"""
    rng = np.random.default_rng(1501)
    tight = _labels(rng, 12, repeats=5)
    need = _min_frames(tight)
    utt = [40, 25, 0, 33, need, need - 1, 50, 0]
    hyps = [[_labels(rng, 3), _labels(rng, 13, repeats=2), E, _labels(rng, 1), _labels(rng, 20)],
            [],  # no hypothesis for this utterance
            [E, np.array([2], np.int32)],  # no frames: 0 and -inf
            [np.array([5] * 9, np.int32), np.array([4] * 3 + [1] + [4] * 4, np.int32), np.array([5] * 17, np.int32)],
            [tight, tight[:-1]], [tight, tight[:-1]],
            [_labels(rng, 21, repeats=6), E, E, _labels(rng, 2)],
            []]
    z = (2.0 * rng.standard_normal((sum(utt), 9))).astype(np.float32)
    got, (s64, _) = _check_logits("pair layout", z, utt, hyps)
    assert got[2].tolist() == [0.0, -np.inf] and got[1].size == 0 and got[7].size == 0
    assert np.isfinite(got[4][0]) and got[5][0] == -np.inf and np.isfinite(got[5][1])  # feasible / one frame short
    assert np.isfinite(got[3][2])  # a run of 17 equal labels needs 17 + 16 frames and has exactly 33
    assert got[6][1] == got[6][2]  # the same pair twice: the same bits


@pytest.mark.parametrize("S", [63, 64, 127, 128, 255, 256, 511])
def test_every_register_tile(gpu, S):
    """the longest hypothesis on both sides of every register tile and at the limit, beside short hypotheses of the same
    utterance: just enough frames, slack, one frame short"""
    rng = np.random.default_rng(1510 + S)
    plain, rep = _labels(rng, S), _labels(rng, S, repeats=S // 5)
    short = [np.array([1, 1], np.int32), E, _labels(rng, 7)]
    utt = [S, S + 41, _min_frames(rep), _min_frames(rep) + 70, _min_frames(rep) - 1, 5]
    hyps = [[plain] + short, short + [plain], [rep] + short, [short[0], rep, short[2]], [rep] + short, short]
    z = (2.0 * rng.standard_normal((sum(utt), 9))).astype(np.float32)
    got, (s64, _) = _check_logits("S=%d" % S, z, utt, hyps)
    assert np.isfinite(got[0][0]) and np.isfinite(got[1][3]) and np.isfinite(got[2][0]) and np.isfinite(got[3][1])
    assert got[4][0] == -np.inf and np.isfinite(got[4][1])


@pytest.mark.parametrize("scale", [6.0, 12.0])
def test_peaky_logits(gpu, scale):
    """a trained model's logits: the blank dominates, a few frames per label stand out -- between two re-centrings the state
    values fall far.  Hypotheses: the best path, the best path with a label dropped / doubled / changed, the empty one."""
    rng = np.random.default_rng(1520 + int(scale))
    utt = [300, 120, 64, 9]
    z = np.concatenate([peaky_logits(rng, n, 36, max(n // 8, 1), scale) for n in utt])
    hyps = []
    for h in best_path(z, utt):
        h = np.asarray(h, np.int32)
        alt = [h, E]
        if h.size >= 2:
            alt += [np.delete(h, h.size // 2), np.insert(h, 1, h[1]), np.where(np.arange(h.size) == 0, (h[0] + 1) % 35, h).astype(np.int32)]
        hyps.append(alt)
    assert sum(hs[0].size for hs in hyps) > 40
    _, (s64, _) = _check_logits("peaky scale %g" % scale, z, utt, hyps)
    assert min(s.min() for s in s64) < -100.0  # unlikely hypotheses are scored too, far below the best


def _engine_case(dtype, O, seed, sharpen=(6.0, 3.0)):
    rng = np.random.default_rng(seed)
    eng, _ = make_pair(rng, max_frames=512, compute_dtype=dtype, **dict(KW, output_dim=O))
    _sharpen(eng, rng, *sharpen)
    utt = [30, 0, 1, 77, 140, 2, 0, 65]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    labels, lab = _refs(np.random.default_rng(seed + 1), len(utt), O, 0, 20)  # (some too long for the 0 / 1 / 2 frames)
    return eng, utt, X, labels, lab


def _flatten(hyps):
    flat = [np.asarray(h, np.int32).reshape(-1) for hs in hyps for h in hs]
    return [len(hs) for hs in hyps], np.concatenate(flat + [E]).astype(np.int32), [h.size for h in flat]


@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
@pytest.mark.parametrize("O", [9, 36])
def test_engine_entry_on_the_engines_logits(gpu, dtype, O):
    """the references, the beam's N-best and the empty hypothesis on the engine's own logits: scores within tol of the
    restatement, edits equal to levenshtein; score of the references = -(eval loss x label count); two calls agree bit for
    bit; parameters, accumulators, moments and statistics are byte-identical around a call"""
    eng, utt, X, labels, lab = _engine_case(dtype, O, 1600 + O, (12.0, 3.0) if O == 36 else (6.0, 3.0))
    refs = _split(labels, lab)
    found, beam = eng.ctc_beam(X, utt, beam_width=10, top_paths=3)[:2]
    hyps = [[refs[u]] + [h for h, s in zip(found[u], beam[u]) if s > -np.inf] + [E] for u in range(len(utt))]
    counts, hl, hn = _flatten(hyps)
    scores, edits = eng.ctc_score(X, utt, counts, hl, hn, labels, lab)
    assert all(s.dtype == np.float32 and s.shape == (c,) for s, c in zip(scores, counts))
    assert all(e.dtype == np.int32 and e.shape == (c,) for e, c in zip(edits, counts))
    zs = np.split(eng.posteriors(X, raw_logits=True), np.cumsum(utt)[:-1])
    s64, tol = _compare("%s O=%d" % (dtype, O), zs, hyps, scores)
    for u in range(len(utt)):
        assert edits[u].tolist() == [levenshtein(h, refs[u]) for h in hyps[u]], u
        assert edits[u][0] == 0
    again = eng.ctc_score(X, utt, counts, hl, hn, labels, lab)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[0], scores))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again[1], edits))
    none = eng.ctc_score(X, utt, counts, hl, hn)  # without references: the same scores, no edits
    assert none[1] is None and all(a.tobytes() == b.tobytes() for a, b in zip(none[0], scores))
    # the loss of the feasible utterances, summed by the loss kernels: eval loss is per label
    ok = [u for u in range(len(utt)) if utt[u] > 0 and np.isfinite(s64[u][0])]
    assert len(ok) >= 4
    sub_utt, sub_lab = [utt[u] for u in ok], [int(lab[u]) for u in ok]
    rows = np.concatenate([np.arange(sum(utt[:u]), sum(utt[:u + 1])) for u in ok])
    eng.eval_accumulate_ctc(X[rows], sub_utt, np.concatenate([refs[u] for u in ok]), sub_lab)
    loss_sum = eng.eval_finish() * sum(sub_lab)
    mine = sum(float(scores[u][0]) for u in ok)
    tol_sum = sum(float(tol[u][0]) for u in ok) + 1e-6 * abs(loss_sum)  # (+ the float rounding of the loss's own sum)
    print("%s O=%d: sum of reference scores %.6f, -(eval loss x labels) %.6f, tol %.2e" % (dtype, O, mine, -loss_sum, tol_sum))
    assert abs(mine + loss_sum) <= tol_sum
    # something in every buffer a decoding call must leave alone: a training micro-batch (utterance 3) is pending
    first = sum(utt[:3])
    eng.accumulate_ctc(X[first:first + utt[3]], [utt[3]], refs[3], [int(lab[3])])
    state0 = _engine_state(eng)
    assert any(np.frombuffer(state0[k], np.float32).any() for k in state0 if k.startswith("gW"))
    around = eng.ctc_score(X, utt, counts, hl, hn, labels, lab)
    state1 = _engine_state(eng)
    assert sorted(state0) == sorted(state1) and all(state0[k] == state1[k] for k in state0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(around[0] + around[1], scores + edits))
    eng.close()


def test_raw_entry_equals_host_spliced_bit_for_bit(gpu):
    import torch
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(1700)
    D, C = 4, 2
    eng, _ = make_pair(rng, max_frames=256, **dict(KW, input_dim=D * (2 * C + 1), output_dim=12))
    _sharpen(eng, rng, 4.0, 2.0)
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 5, 63, 17)]
    lens = [u.shape[0] for u in utts]
    labels, lab = _refs(np.random.default_rng(1701), len(utts), 12, 0, 15)
    refs = _split(labels, lab)
    hyps = [[r, r[:r.size // 2], E] for r in refs]
    hyps[1] = []
    counts, hl, hn = _flatten(hyps)
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)

    def same(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0])) and all(x.tobytes() == y.tobytes() for x, y in zip(a[1], b[1]))

    host = eng.ctc_score(np.concatenate([u.spliced() for u in utts]), lens, counts, hl, hn, labels, lab)
    dev = eng.ctc_score_raw(raw, lens, C, counts, hl, hn, labels, lab, cmvn=cmvn_table(utts))
    cuda = eng.ctc_score_raw(torch.from_numpy(raw).cuda(), lens, C, counts, hl, hn, labels, lab, cmvn=cmvn_table(utts))
    assert same(host, dev) and same(host, cuda)
    assert sum(int(np.isfinite(s).sum()) for s in host[0]) >= 6 and host[0][1].size == 0
    eng.close()


def test_bounds_beam_score_and_alignment_score(gpu):
    """score >= the beam's score of the same hypothesis (the alignments that survived pruning are some of all), score >= the
    alignment score (the best path is one term of the sum); equal for an empty hypothesis (one alignment)"""
    eng, utt, X, _, _ = _engine_case("float32", 9, 1800)
    zs = np.split(eng.posteriors(X, raw_logits=True), np.cumsum(utt)[:-1])
    z = np.concatenate(zs)
    for W in (2, 10):
        found, beam = eng.ctc_beam(X, utt, beam_width=W, top_paths=min(W, 4))[:2]
        hyps = [[h for h, s in zip(hs, sc) if s > -np.inf] for hs, sc in zip(found, beam)]
        scores = eng.ctc_score(X, utt, *_flatten(hyps))[0]
        s64, tol = _compare("bounds W=%d" % W, zs, hyps, scores)
        gap = 0.0
        for u in range(len(utt)):
            for n in range(len(hyps[u])):
                assert float(scores[u][n]) >= float(beam[u][n]) - tol[u][n], (W, u, n, scores[u][n], beam[u][n], tol[u][n])
                gap = max(gap, float(scores[u][n]) - float(beam[u][n]))
        print("W=%d: largest exact minus beam score %.4f nats" % (W, gap))
    # against the alignment of the same pairs, one pair per utterance, on the stand-alone entries
    rng = np.random.default_rng(1801)
    refs = [_labels(rng, min(n // 3, 20)) if n >= 3 else E for n in utt]
    refs[3] = E  # an empty hypothesis on 77 frames
    _, ali = _device_align_logits(z, utt, refs)
    got = _device_score_logits(z, utt, [[r] for r in refs])
    s64, tol = _compare("bounds align", zs, [[r] for r in refs], got)
    for u in range(len(utt)):
        assert float(got[u][0]) >= float(ali[u]) - tol[u][0], (u, got[u][0], ali[u])
        if refs[u].size == 0 and utt[u]:
            a64 = viterbi_align(zs[u], refs[u])[1]
            assert abs(float(got[u][0]) - a64) <= tol[u][0] and abs(float(got[u][0]) - float(ali[u])) <= 2 * tol[u][0]
    eng.close()


def test_reranking_dense_gaussian_logits(gpu):
    """8 x 40 frames, O = 9, W = 3, top_paths = 3: narrow beams under-count by nats and the order changes.  The test first
    asserts its own precondition from the float64 restatement alone, then requires the device's order to equal it."""
    from tfkaldi_amd.neuralNetworks.decoder import ctc_rerank
    rng = np.random.default_rng(1900)
    U, Tn, O, W = 8, 40, 9, 3
    utt = [Tn] * U
    z = (2.0 * rng.standard_normal((U * Tn, O))).astype(np.float32)
    zs = np.split(z, U)
    found, beam = prefix_beam_search(z, utt, W, W)
    hyps = [[h for h, s in zip(hs, sc) if s > -np.inf] for hs, sc in zip(found, beam)]
    assert all(len(hs) == W for hs in hyps)
    s64, tol = rescore_tol([zs[u] for u in range(U) for _ in hyps[u]], [h for hs in hyps for h in hs])
    s64, tol = s64.reshape(U, W), tol.reshape(U, W)
    want = [ctc_rerank(hyps[u], s64[u])[0] for u in range(U)]
    moved = sum(int(o[0] != 0) for o in want)
    clear = [u for u in range(U)
             if all(s64[u][a] - s64[u][b] >= 2 * max(tol[u][a], tol[u][b]) for a, b in zip(want[u][:-1], want[u][1:]))]
    print("re-ranking: %d of %d utterances change their best hypothesis, %d with clear gaps, smallest gap %.3e, tol %.3e"
          % (moved, U, len(clear), min(s64[u][a] - s64[u][b] for u in range(U) for a, b in zip(want[u][:-1], want[u][1:])),
             tol.max()))
    assert moved >= 2 and 4 * (U - len(clear)) <= U
    got = _device_score_logits(z, utt, hyps)
    _compare("re-ranking", zs, hyps, got)
    for u in clear:
        assert ctc_rerank(hyps[u], got[u])[0].tolist() == want[u].tolist(), (u, got[u], s64[u])


def test_edits_and_oracle_rate(gpu):
    """edits = levenshtein for every pair, a reference of 511 labels, an empty hypothesis and an empty reference included;
    the oracle rate (the list's best hypothesis) <= the rescored rate <= what the restatement gives for it"""
    from tfkaldi_amd.neuralNetworks.decoder import ctc_rerank
    rng = np.random.default_rng(2000)
    eng, _ = make_pair(rng, max_frames=1024, **KW)
    _sharpen(eng, rng, 6.0, 3.0)
    O = KW["output_dim"]
    utt = [600, 40, 80, 25]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    refs = [rng.integers(0, O - 1, size=511).astype(np.int32), E, _labels(rng, 12), _labels(rng, 5)]
    found, beam = eng.ctc_beam(X, utt, beam_width=8, top_paths=4)[:2]
    hyps = [[h for h, s in zip(hs, sc) if s > -np.inf] + [E] for hs, sc in zip(found, beam)]
    hyps[0].append(rng.integers(0, O - 1, size=300).astype(np.int32))  # 300 labels on 600 frames against 511
    hyps[0].append(refs[0][:290])
    scores, edits = eng.ctc_score(X, utt, *_flatten(hyps), np.concatenate(refs), [r.size for r in refs])
    zs = np.split(eng.posteriors(X, raw_logits=True), np.cumsum(utt)[:-1])
    s64, tol = _compare("edits", zs, hyps, scores)
    total = sum(r.size for r in refs)
    oracle = rescored = restated = 0
    for u in range(len(utt)):
        want = [levenshtein(h, refs[u]) for h in hyps[u]]
        assert edits[u].tolist() == want, (u, edits[u], want)
        oracle += min(want)
        rescored += want[ctc_rerank(hyps[u], scores[u])[0][0]]
        restated += want[ctc_rerank(hyps[u], s64[u])[0][0]]
    assert edits[1].tolist() == [h.size for h in hyps[1]] and edits[0][-3] == 511  # empty reference; empty hypothesis
    print("label error rates: oracle %.4f, rescored %.4f, restatement %.4f" % (oracle / total, rescored / total, restated / total))
    assert oracle <= rescored <= restated
    eng.close()


@pytest.mark.parametrize("with_lm", [False, True])
def test_decoder_rescore_end_to_end(gpu, tmp_path, with_lm):
    from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM
    from tfkaldi_amd.neuralNetworks.decoder import Decoder, ctc_rerank
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    for _ in range(30):
        tr.update(xs, ys)
    targets = [np.asarray(y).astype(np.int32) for y in ys]
    lm = NgramLM.from_label_sequences(targets, coder.num_labels, 2, weight=0.8, label_bonus=0.2, end_of_sequence=True) \
        if with_lm else None
    plain = tr.label_errors(xs, ys, beam_width=6)
    rescored = tr.label_errors(xs, ys, beam_width=6, lm=lm, rescore_paths=4)
    assert rescored[1] == plain[1] == sum(t.size for t in targets) and 0 <= rescored[0]
    tr.save_model(str(tmp_path / "model"))
    tr.close()
    dec = Decoder(dnn, F, maxlen)
    dec.restore(str(tmp_path / "model"))
    for topk in (None, 5):
        hyps, scores, am, rank, post = dec.ctc_rescore(xs, beam_width=6, top_paths=4, lm=lm, label_topk=topk)
        if lm is None:
            found, beam = dec.ctc_beam_search(xs, 6, 4, topk)
        else:
            found, beam, _ = dec.ctc_beam_search_lm(xs, lm, 6, 4, topk)
        kept = [[h for h, s in zip(hs, sc) if s > -np.inf] for hs, sc in zip(found, beam)]
        exact = dec.ctc_score(xs, kept)[0]  # the same pass over the same pairs: the same bits
        for u in range(len(xs)):
            assert len(hyps[u]) == len(kept[u]) and sorted(rank[u].tolist()) == list(range(len(kept[u])))
            assert all(np.array_equal(h, kept[u][r]) for h, r in zip(hyps[u], rank[u]))
            assert am[u].dtype == np.float32 and am[u].tobytes() == exact[u][rank[u]].tobytes()
            order, want, wpost = ctc_rerank(kept[u], exact[u], lm)
            assert order.tolist() == rank[u].tolist() and np.array_equal(want, scores[u]) and np.array_equal(wpost, post[u])
            assert np.all(np.diff(scores[u]) <= 0) and abs(post[u].sum() - 1.0) <= 1e-12
        if topk is None:  # what label_errors(rescore_paths=) counted: the edits of the new best hypotheses
            assert rescored[0] == sum(levenshtein(h[0], t) for h, t in zip(hyps, targets))
    got = dec.ctc_score(xs, [[t] for t in targets], refs=targets)
    assert all(e.tolist() == [0] for e in got[1]) and all(np.isfinite(s).all() for s in got[0])
    assert dec.ctc_rescore([]) == ([], [], [], [], []) and dec.ctc_score([], []) == ([], None)
    dec.close()


def test_no_frames_at_all_does_not_call_the_engine(gpu):
    rng = np.random.default_rng(2100)
    eng, _ = make_pair(rng, max_frames=64, **KW)
    X = np.zeros((0, KW["input_dim"]), np.float32)
    scores, edits = eng.ctc_score(X, [0, 0], [2, 1], [1, 2], [0, 2, 0], [3], [1, 0])
    assert scores[0].tolist() == [0.0, -np.inf] and scores[1].tolist() == [0.0]
    assert edits[0].tolist() == [1, 2] and edits[1].tolist() == [0]
    assert eng.ctc_score(X, [0], [0], [], [])[0][0].size == 0
    with pytest.raises(ValueError):
        eng.ctc_score(X, [0, 0], [1], [], [0])
    with pytest.raises(ValueError):
        eng.ctc_score(X, [0], [2], [1], [1])
    eng.close()


def test_limits_are_reported_and_leave_the_engine_usable(gpu):
    import torch
    from tfkaldi_amd import _lib
    rng = np.random.default_rng(2200)
    eng, _ = make_pair(rng, max_frames=1024, **KW)
    O = KW["output_dim"]
    utt = np.array([600, 15], np.int32)
    X = rng.standard_normal((615, KW["input_dim"])).astype(np.float32)
    refs, ref_len = _refs(rng, 2, O, 3, 6)
    counts = np.array([2, 1], np.int32)
    hl, hn = _refs(rng, 3, O, 2, 5)
    good = eng.ctc_score(X, utt, counts, hl, hn, refs, ref_len)
    ptr = lambda a, on=True: a.ctypes.data_as(c_void_p) if on else c_void_p(None)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)

    def call(score=True, edits=True, flags=0, cnt=counts, lab_vals=hl, lab_lens=hn, lens=utt, X_on=True, lab_on=True,
             len_on=True, cnt_on=True, ref_on=True, T=615):
        n = max(int(np.sum(np.maximum(cnt, 0))), 1)
        s, d = np.empty(n, np.float32), np.empty(n, np.int32)
        return eng.lib.tfk_ctc_score(eng._h, ptr(X, X_on), X.shape[1], T, ptr(i32(lens)), 2, ptr(i32(cnt), cnt_on),
                                     ptr(i32(lab_vals), lab_on), ptr(i32(lab_lens), len_on), ptr(refs, ref_on),
                                     ptr(ref_len, ref_on), ptr(s, score), ptr(d, edits), flags)

    big = rng.integers(0, O - 1, size=512).astype(np.int32)
    cases = [
        ("512 labels", dict(lab_vals=np.concatenate([hl[:hn[0]], big, hl[hn[0] + hn[1]:]]), lab_lens=[hn[0], 512, hn[2]]),
         b"utterance 0, hypothesis 1 has 512 labels (limit 511)"),
        ("label >= O - 1", dict(lab_vals=np.where(np.arange(hl.size) == hn[0] + hn[1], O - 1, hl)), b"utterance 1, hypothesis 0: label"),
        ("negative label", dict(lab_vals=np.where(np.arange(hl.size) == 0, -1, hl)), b"utterance 0, hypothesis 0: label -1"),
        ("negative label count", dict(lab_lens=[hn[0], -1, hn[2]]), b"negative"),
        ("negative hypothesis count", dict(cnt=[-1, 1]), b"negative hypothesis count"),
        ("negative frame count", dict(lens=[616, -1]), b"negative"),
        ("too many pairs", dict(cnt=[1 << 20, 1]), b"more than 1048576"),
        ("edits without references", dict(ref_on=False), b"edits without references"),
        ("NULL score", dict(score=False), b"NULL"), ("NULL X", dict(X_on=False), b"NULL"),
        ("NULL labels", dict(lab_on=False), b"NULL"), ("NULL label_len", dict(len_on=False), b"NULL"),
        ("NULL hyp_count", dict(cnt_on=False), b"NULL"),
        ("T = 0", dict(T=0), b"T = 0"), ("utt_len does not sum to T", dict(T=614), b"sum"),
        ("unknown flag", dict(flags=_lib.DEVICE_PTRS), b"flags"), ("raw-only flag", dict(flags=_lib.RAW_DEVICE), b"flags"),
    ]
    for name, kw, word in cases:
        assert call(**kw) != 0, name
        assert word in eng.lib.tfk_last_error(), (name, eng.lib.tfk_last_error())
        again = eng.ctc_score(X, utt, counts, hl, hn, refs, ref_len)  # the next valid call succeeds, with the same result
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again[0] + again[1], good[0] + good[1])), name
    assert call() == 0 and call(edits=False, ref_on=False) == 0
    assert call(cnt=[0, 0], score=False, edits=False, lab_on=False, len_on=False, ref_on=False) == 0  # P == 0 writes nothing
    eng.close()
    # the stand-alone entry
    lib = _lib.load()
    z = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    tab = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")
    lab_dev = torch.zeros(600, dtype=torch.int32, device="cuda")

    def logits_call(seg, pair_utt, off, P=None, seg_on=True):
        d_seg, d_utt, d_off = tab(seg), tab(pair_utt), tab(off)
        return lib.tfk_ctc_score_logits(c_void_p(0), c_void_p(z.data_ptr()), 4, 4, 8, c_void_p(d_seg.data_ptr() if seg_on else None),
                                        len(seg) - 1, c_void_p(d_utt.data_ptr()), len(pair_utt) if P is None else P,
                                        c_void_p(lab_dev.data_ptr()), c_void_p(d_off.data_ptr()), c_void_p(out.data_ptr()))

    for args, word in ((([0, 8], [0], [0, 512]), b"511"), (([0, 8, 6], [0, 1], [0, 1, 2]), b"negative"),
                       (([0, 4, 8], [0, 1], [0, 2, 1]), b"negative"), (([0, 4, 8], [0, 2], [0, 1, 2]), b"names utterance 2"),
                       (([0, 4, 9], [0, 1], [0, 1, 2]), b"outside [0, T = 8]")):
        assert logits_call(*args) != 0
        assert word in lib.tfk_last_error(), (args, lib.tfk_last_error())
    assert logits_call([0, 8], [0], [0, 1], P=(1 << 20) + 1) != 0 and b"1048576" in lib.tfk_last_error()
    assert logits_call([0, 8], [0], [0, 1], seg_on=False) != 0 and b"NULL" in lib.tfk_last_error()
    assert logits_call([0, 8], [0], [0, 1], P=0) == 0 and logits_call([0, 8], [0, 0], [0, 1, 1]) == 0
    torch.cuda.synchronize()
    assert out[0].item() < 0 and out[1].item() < 0 and out[2].item() == 0  # P = 2 wrote two scores
