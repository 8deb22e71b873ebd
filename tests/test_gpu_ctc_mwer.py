"""MWER training of a CTC model on the device (tfk_ctc_mwer_logits, tfk_accumulate_ctc_mwer and its variants, csrc/ctc.hip):
the expected number of label errors over an N-best list and its gradient against the float64 restatement of
tests/test_ctc_mwer_host.py applied to the SAME logits (chosen ones through the stand-alone entry, the oracle's train-mode
logits for the engine entries).

Tolerances (none of them comes from a device figure):
  scores    rescore_tol of tests/test_ctc_score_host.py, per pair (tol_s below: the largest among an utterance's pairs)
  edits     exact
  risk[u]   2 tol_s D_u + 1e-6 |R_u|, D_u = max_i |e_i - R_u| of the float64 run
  dLogits   rtol 1e-4 + (a + 4 tol_s) D_u + a ctc_weight per row of utterance u; a = 2e-5 below 200 frames per batch, 2e-4
            from there on (the dLogits bound of tests/test_gpu_ctc.py, applied to each posterior term: the weighted sum of
            posteriors carries at most a sum|w_i| <= a D_u; the weights inherit the scores' error through the list's
            softmax, sum_i |dw_i| <= 4 tol_s D_u)
  row sums  64 O 6e-8 (D_u + ctc_weight): the fp32 rounding of that many terms
The last two also carry the float64 run's OWN rounding, 4 x 2.3e-16 x N x max e_i: where every hypothesis of a list has the
same e_i, R_u equals it only up to that rounding, D_u is of that size instead of zero, and neither side's weights sum to
zero more exactly than that.
Every case prints its largest errors beside the bounds (`ctc-mwer` lines under pytest -s; recorded in
profiles/ctc_mwer_edges.txt)."""
from ctypes import c_void_p

import numpy as np
import pytest

from oracle.ctc_oracle import ctc_batch
from test_ctc_decode_host import levenshtein
from test_ctc_mwer_host import mwer_restated
from test_ctc_score_host import rescore_tol
from test_gpu_ctc_align import _labels, _min_frames
from test_gpu_ctc_beam import KW
from test_gpu_ctc_beam_topk import _engine_state
from test_gpu_ctc_score import _device_score_logits
from tfkaldi_amd.neuralNetworks.ctc_mwer import pair_tables
from util import assert_close, engine_grads, engine_params, make_pair

pytestmark = pytest.mark.gpu

E = np.zeros(0, np.int32)
SENT = 12345.0


def _device_mwer(z, utt, hyps, refs, cw=0.0, grad=True, lead=3, tail=5, pad=3, dpad=2):
    """tfk_ctc_mwer_logits on host logits whose utterances start at row `lead` (seg[0] > 0) of a [lead + sum(utt) + tail,
    O + pad] matrix (ld > O) with NaN sentinel rows before and after; hyps[u] = utterance u's list of label arrays, refs[u]
    its reference.  Returns (risk [U], scores per utterance, edits per utterance, dlogits [sum(utt), O] or None); what lies
    around the outputs -- rows outside the utterances, the element after each output -- must come back untouched, and the
    padding columns of dlogits as zeros."""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    O, U, rows = z.shape[1], len(utt), z.shape[0]
    T = lead + rows + tail
    full = np.full((T, O + pad), 50.0, np.float32)
    full[:lead, :O] = np.nan  # sentinel rows: a value read from them poisons the result
    full[lead + rows:, :O] = np.nan
    full[lead:lead + rows, :O] = z
    seg = (lead + np.concatenate([[0], np.cumsum(utt)])).astype(np.int32)
    flat = [np.asarray(h, np.int32).reshape(-1) for hs in hyps for h in hs]
    P = len(flat)
    pair_utt = np.repeat(np.arange(U), [len(hs) for hs in hyps]).astype(np.int32)
    lab_off = 7 + np.concatenate([[0], np.cumsum([h.size for h in flat])]).astype(np.int32)  # (lab_off[0] > 0)
    labels = np.concatenate([np.full(7, 1 << 20, np.int32)] + flat + [np.zeros(1, np.int32)])
    rflat = [np.asarray(r, np.int32).reshape(-1) for r in refs]
    ref_off = np.concatenate([[0], np.cumsum([r.size for r in rflat])]).astype(np.int32)
    ref_labels = np.concatenate(rflat + [np.zeros(1, np.int32)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_z, d_seg, d_utt, d_off, d_lab = dev(full), dev(seg), dev(np.concatenate([pair_utt, [0]]).astype(np.int32)), dev(lab_off), dev(labels)
    d_roff, d_rlab = dev(ref_off), dev(ref_labels)
    risk = torch.full((U + 1,), SENT, dtype=torch.float32, device="cuda")
    score = torch.full((P + 1,), SENT, dtype=torch.float32, device="cuda")
    edits = torch.full((P + 1,), -777, dtype=torch.int32, device="cuda")
    dlog = torch.full((T, O + dpad), SENT, dtype=torch.float32, device="cuda") if grad else None
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tfk_ctc_mwer_logits(c_void_p(stream), c_void_p(d_z.data_ptr()), O + pad, O, T, c_void_p(d_seg.data_ptr()), U,
                                       c_void_p(d_utt.data_ptr()), P, c_void_p(d_lab.data_ptr()), c_void_p(d_off.data_ptr()),
                                       c_void_p(d_rlab.data_ptr()), c_void_p(d_roff.data_ptr()), float(cw),
                                       c_void_p(dlog.data_ptr() if grad else None), O + dpad, c_void_p(risk.data_ptr()),
                                       c_void_p(score.data_ptr()), c_void_p(edits.data_ptr())))
    torch.cuda.synchronize()
    risk, score, edits = risk.cpu().numpy(), score.cpu().numpy(), edits.cpu().numpy()
    assert risk[U] == SENT and score[P] == SENT and edits[P] == -777  # nothing is written beyond the outputs
    assert np.array_equal(d_z.cpu().numpy(), full, equal_nan=True)  # the logits are not overwritten
    cuts = np.cumsum([len(hs) for hs in hyps])[:-1]
    if grad:
        dlog = dlog.cpu().numpy()
        assert np.all(dlog[:lead] == SENT) and np.all(dlog[lead + rows:] == SENT)  # rows outside the utterances
        assert np.all(dlog[lead:lead + rows, O:] == 0.0)  # the ld - O padding columns
        dlog = dlog[lead:lead + rows, :O]
    return risk[:U], np.split(score[:P], cuts), np.split(edits[:P], cuts), dlog


def _restate(z, utt, hyps, refs, cw):
    zs = np.split(np.asarray(z, np.float32), np.cumsum(utt)[:-1])
    return zs, [mwer_restated(zs[u], hyps[u], refs[u], cw) for u in range(len(utt))]


def _compare(name, z, utt, hyps, refs, cw, got, a=None):
    """device outputs `got` against the restatement; returns the restatement per utterance"""
    risk, scores, edits, dlog = got
    zs, want = _restate(z, utt, hyps, refs, cw)
    a = (2e-5 if sum(utt) < 200 else 2e-4) if a is None else a
    s64, tol = rescore_tol([zs[u] for u, hs in enumerate(hyps) for _ in hs], [h for hs in hyps for h in hs])
    cuts = np.cumsum([len(hs) for hs in hyps])[:-1]
    tols = np.split(tol, cuts)
    worst = dict(score=0.0, risk=0.0, dlog=0.0, rowsum=0.0)
    bound = dict(score=0.0, risk=0.0, dlog=0.0, rowsum=0.0)
    first = 0
    O = np.asarray(z).shape[1]
    for u in range(len(utt)):
        loss64, grad64, R, sc64, ed64, w64 = want[u]
        assert edits[u].tolist() == ed64.tolist(), (name, u)
        for i in range(len(hyps[u])):
            if sc64[i] == -np.inf:
                assert scores[u][i] == -np.inf, (name, u, i, scores[u][i])
                continue
            err = abs(float(scores[u][i]) - sc64[i])
            worst["score"], bound["score"] = max(worst["score"], err), max(bound["score"], tols[u][i])
            assert err <= tols[u][i], (name, u, i, scores[u][i], sc64[i], tols[u][i])
        D = float(np.abs(ed64 - R).max()) if len(hyps[u]) else 0.0
        tol_s = float(tols[u].max()) if len(hyps[u]) else 0.0
        rb = 2 * tol_s * D + 1e-6 * abs(R)
        worst["risk"], bound["risk"] = max(worst["risk"], abs(float(risk[u]) - R)), max(bound["risk"], rb)
        assert abs(float(risk[u]) - R) <= rb, (name, u, risk[u], R, rb)
        if dlog is not None and utt[u]:
            rows = dlog[first:first + utt[u]].astype(np.float64)
            own = 4 * 2.3e-16 * len(hyps[u]) * max(float(ed64.max()) if len(hyps[u]) else 0.0, 1.0)  # (see the module docstring)
            db = (a + 4 * tol_s) * D + a * cw + own
            err = np.abs(rows - grad64) - 1e-4 * np.abs(grad64)
            worst["dlog"], bound["dlog"] = max(worst["dlog"], float(np.abs(rows - grad64).max())), max(bound["dlog"], db)
            assert err.max() <= db, (name, u, float(np.abs(rows - grad64).max()), db)
            sb = 64 * O * 6e-8 * (D + cw) + own
            worst["rowsum"], bound["rowsum"] = max(worst["rowsum"], float(np.abs(rows.sum(axis=1)).max())), max(bound["rowsum"], sb)
            assert np.abs(rows.sum(axis=1)).max() <= sb, (name, u, np.abs(rows.sum(axis=1)).max(), sb)
        first += utt[u]
    print("ctc-mwer %-24s U %2d T %4d P %3d S max %3d cw %.2f | score %.1e (tol %.1e) risk %.1e (%.1e) dlogits %.1e (%.1e) "
          "row sum %.1e (%.1e)" % (name, len(utt), sum(utt), sum(len(hs) for hs in hyps),
                                   max([len(h) for hs in hyps for h in hs] + [0]), cw, worst["score"], bound["score"],
                                   worst["risk"], bound["risk"], worst["dlog"], bound["dlog"], worst["rowsum"], bound["rowsum"]))
    return want


def _check(name, z, utt, hyps, refs, cw=0.0):
    got = _device_mwer(z, utt, hyps, refs, cw)
    return got, _compare(name, z, utt, hyps, refs, cw, got)


def _logits(rng, T, O=9):
    return (2.0 * rng.standard_normal((T, O))).astype(np.float32)


def _other(rng, hyps, S, O=9):
    """a reference of about S labels that equals none of the hypotheses"""
    while True:
        r = _labels(rng, max(S, 1), O=O)
        if not any(np.array_equal(r, h) for h in hyps):
            return r


# ---- the stand-alone entry ----

def test_frame_counts_around_the_prefetch_ring(gpu):
    """frame counts around the ring of 8 rows and beyond; per list a short hypothesis, the empty one and one with repeats;
    the reference differs from all of them"""
    rng = np.random.default_rng(5000)
    utt, hyps, refs = [], [], []
    for Tn in (1, 2, 3, 7, 8, 9, 10, 16, 17, 63, 64, 65, 300):
        utt.append(Tn)
        longest = max(min(Tn // 3, 40), 1)
        hs = [_labels(rng, int(rng.integers(1, longest + 1))) if Tn >= 3 else _labels(rng, 1), E,
              _labels(rng, longest, repeats=min(longest // 4, max(longest - 1, 0)))]
        if Tn % 2 == 0:
            hs.append(_labels(rng, max(longest // 2, 1)))
        hyps.append(hs)
        refs.append(_other(rng, hs, longest))
    z = _logits(rng, sum(utt))
    got, want = _check("frame counts", z, utt, hyps, refs)
    assert all(np.isfinite(w[3]).sum() >= 2 for w in want[2:])
    assert max(np.abs(w[1]).max() for w in want) > 1e-2  # (not a check of zeros)


def test_pair_layout_in_one_batch(gpu):
    rng = np.random.default_rng(5001)
    tight = _labels(rng, 12, repeats=5)
    need = _min_frames(tight)
    same = _labels(rng, 4)
    ref6 = np.array([1, 2, 3, 4], np.int32)
    equal = [np.array([1, 2, 3, 5], np.int32), np.array([0, 2, 3, 4], np.int32), np.array([1, 2, 4], np.int32)]  # edits 1, 1, 1
    utt = [40, 25, 0, 33, need, need - 1, 50, 0, 6, 30, 28]
    hyps = [[_labels(rng, 3), _labels(rng, 13, repeats=2), E, _labels(rng, 1), _labels(rng, 20)],  # very different lengths
            [],  # no hypothesis for this utterance
            [E, np.array([2], np.int32)],  # no frames: score 0 and -inf
            [_labels(rng, 5)],  # a single hypothesis: rows exactly zero
            [tight, tight[:-1]], [tight, tight[:-1]],  # exactly feasible / the same pair one frame short
            [_labels(rng, 21, repeats=6), same, same, _labels(rng, 2)],  # the same hypothesis twice
            [np.array([3], np.int32)],  # no frames, S > 0 only
            [_labels(rng, 7), _labels(rng, 9)],  # only infeasible pairs on 6 frames
            [_labels(rng, int(rng.integers(0, 9))) for _ in range(40)],  # the fold's pair loop
            equal]
    refs = [_labels(rng, 6), _labels(rng, 4), E, _labels(rng, 5), tight[:-2], tight[:-2], _labels(rng, 8), E, _labels(rng, 2),
            _labels(rng, 6), ref6]
    z = _logits(rng, sum(utt))
    (risk, scores, edits, dlog), want = _check("pair layout", z, utt, hyps, refs)
    row = np.concatenate([[0], np.cumsum(utt)])
    rows = lambda u: dlog[row[u]:row[u + 1]]
    assert risk[1] == 0.0 and np.all(rows(1) == 0.0)  # hyp_count = 0
    assert scores[2].tolist() == [0.0, -np.inf] and risk[2] == 0.0 and scores[7].tolist() == [-np.inf] and risk[7] == 0.0
    assert np.all(rows(3) == 0.0) and risk[3] == edits[3][0]  # a single hypothesis
    assert np.isfinite(scores[4]).all() and scores[5][0] == -np.inf and np.isfinite(scores[5][1])
    assert np.all(rows(5) == 0.0) and risk[5] == edits[5][1]  # one feasible pair left: weight 0
    assert scores[6][1] == scores[6][2] and want[6][5][1] == want[6][5][2]  # the same pair twice, counted twice
    assert np.all(scores[8] == -np.inf) and risk[8] == 0.0 and np.all(rows(8) == 0.0)  # only infeasible pairs
    assert len(hyps[9]) == 40 and np.abs(rows(9)).max() > 1e-2
    assert edits[10].tolist() == [1, 1, 1] and abs(risk[10] - 1.0) <= 1e-6  # equal edits: zero within the bound (in _compare)
    assert np.abs(want[10][1]).max() <= 1e-15


@pytest.mark.parametrize("S", [63, 64, 127, 128, 255, 511])
def test_every_register_tile(gpu, S):
    """the longest hypothesis on both sides of every register tile and at the limit, beside short ones of the same utterance"""
    rng = np.random.default_rng(5010 + S)
    plain, rep = _labels(rng, S), _labels(rng, S, repeats=S // 5)
    short = [np.array([1, 1], np.int32), E, _labels(rng, 7)]
    utt = [S + 41, _min_frames(rep) + 41, S + 41]
    # (the third list holds long hypotheses only, one label apart: comparable scores, D_u <= 1, so the long rows are checked
    # against a bound of the size of `a`, where the first two lists give them almost no weight)
    hyps = [[plain] + short, [short[0], rep, short[2]], [plain, np.delete(plain, S // 2), np.delete(plain, 0)]]
    refs = [plain[:S - 3], _labels(rng, 9), plain]
    z = _logits(rng, sum(utt))
    (risk, scores, edits, dlog), want = _check("S=%d" % S, z, utt, hyps, refs)
    assert np.isfinite(scores[0][0]) and np.isfinite(scores[1][1]) and edits[0][0] == 3


@pytest.mark.parametrize("O", [2, 65, 130])
def test_class_layout(gpu, O):
    """one label and the blank; the lane-strided row loops across 64 and 128 classes"""
    rng = np.random.default_rng(5020 + O)
    lab = lambda n: (np.zeros(n, np.int32) if O == 2 else _labels(rng, n, O=O))
    utt = [30, 45]
    hyps = [[lab(3), E, lab(5), lab(1)], [lab(6), lab(2), lab(4) if O > 2 else lab(7)]]
    if O > 2:
        hyps[1][0][:2] = [O - 2, 63]  # the last label class, and one in the second 64
        hyps[0][2][0] = 64 if O > 65 else O - 2
    refs = [lab(4) if O > 2 else lab(2), lab(3)]
    z = _logits(rng, sum(utt), O)
    got, want = _check("O=%d" % O, z, utt, hyps, refs, cw=0.5 if O == 65 else 0.0)
    assert max(np.abs(w[1]).max() for w in want) > 1e-2


def test_ctc_term_alone_equals_the_ctc_loss(gpu):
    """ctc_weight = 1 and no hypothesis anywhere: dlogits are the CTC loss's, at the tolerances of tests/test_gpu_ctc.py"""
    rng = np.random.default_rng(5030)
    utt = [30, 17, 44, 9]
    refs = [_labels(rng, 5), _labels(rng, 3), _labels(rng, 11, repeats=3), E]
    z = _logits(rng, sum(utt))
    risk, scores, edits, dlog = _device_mwer(z, utt, [[] for _ in utt], refs, cw=1.0)
    loss, want, n = ctc_batch(z.astype(np.float64), utt, np.concatenate(refs), [r.size for r in refs], fast=True)
    print("ctc-mwer ctc term alone: dlogits %.1e (atol 2e-5)" % np.abs(dlog - want).max())
    assert_close("dlogits", dlog, want, rtol=1e-4, atol=2e-5)
    assert np.all(risk == 0.0) and np.isfinite(loss)


def test_ctc_term_with_hypotheses_and_an_infeasible_reference(gpu):
    rng = np.random.default_rng(5031)
    utt = [40, 12, 33]
    long_ref = _labels(rng, 14)  # 12 frames cannot hold 14 labels
    hyps = [[_labels(rng, 4), E, _labels(rng, 9, repeats=2)], [_labels(rng, 3), E, _labels(rng, 2)], [_labels(rng, 6), _labels(rng, 1)]]
    refs = [_labels(rng, 5), long_ref, _labels(rng, 7)]
    z = _logits(rng, sum(utt))
    (risk, scores, edits, dlog), want = _check("ctc_weight 0.3", z, utt, hyps, refs, cw=0.3)
    assert want[1][0] == np.inf and np.isfinite(want[0][0]) and np.isfinite(want[2][0])  # +inf from that utterance ...
    mwer_only = mwer_restated(np.split(z, np.cumsum(utt)[:-1])[1], hyps[1], refs[1], 0.0)[1]
    assert np.array_equal(want[1][1], mwer_only) and np.abs(mwer_only).max() > 1e-3  # ... and its MWER rows stay


def test_invariants(gpu):
    """two calls agree bit for bit; dlogits == NULL returns the same risk, score and edits; the scores are tfk_ctc_score_logits'"""
    rng = np.random.default_rng(5040)
    utt = [50, 0, 21, 130]
    hyps = [[_labels(rng, int(rng.integers(0, 12))) for _ in range(7)], [E], [_labels(rng, 3), _labels(rng, 30)],
            [_labels(rng, int(rng.integers(5, 40)), repeats=2) for _ in range(5)]]
    refs = [_labels(rng, 6), E, _labels(rng, 4), _labels(rng, 25)]
    z = _logits(rng, sum(utt))
    a = _device_mwer(z, utt, hyps, refs, cw=0.2)
    b = _device_mwer(z, utt, hyps, refs, cw=0.2)
    c = _device_mwer(z, utt, hyps, refs, cw=0.2, grad=False)
    flat = lambda g: [g[0]] + list(g[1]) + list(g[2])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flat(a), flat(b))) and a[3].tobytes() == b[3].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flat(a), flat(c))) and c[3] is None
    _compare("invariants", z, utt, hyps, refs, 0.2, a)
    zs = np.split(z, np.cumsum(utt)[:-1])
    s64, tol = rescore_tol([zs[u] for u, hs in enumerate(hyps) for _ in hs], [h for hs in hyps for h in hs])
    other = np.concatenate(_device_score_logits(z, utt, hyps))
    mine = np.concatenate(a[1])
    fin = np.isfinite(s64)
    assert np.array_equal(np.isfinite(mine), fin) and np.array_equal(np.isfinite(other), fin)
    assert np.all(np.abs(mine[fin].astype(np.float64) - other[fin]) <= tol[fin])


def test_shapes_beyond_the_limits_are_refused(gpu):
    """more LDS than a launch can get, more lattice states than the index range: a message, not a failed launch"""
    import torch
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    rng = np.random.default_rng(5050)
    with pytest.raises(EngineError, match="LDS"):
        _device_mwer(_logits(rng, 4, 17000), [4], [[E, np.array([1], np.int32)]], [E])
    lib = _lib.load()
    U, P, Tn = 1, 1 << 20, 8200  # 2^20 pairs x 8200 frames x 128 states > 2^33
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_z, d_seg = dev(np.zeros((Tn, 2), np.float32)), dev(np.array([0, Tn], np.int32))
    d_utt, d_off, d_roff = dev(np.zeros(P, np.int32)), dev(np.zeros(P + 1, np.int32)), dev(np.zeros(2, np.int32))
    out = torch.zeros(P + 1, dtype=torch.float32, device="cuda")
    ed = torch.zeros(P + 1, dtype=torch.int32, device="cuda")
    rc = lib.tfk_ctc_mwer_logits(c_void_p(torch.cuda.current_stream().cuda_stream), c_void_p(d_z.data_ptr()), 2, 2, Tn,
                                 c_void_p(d_seg.data_ptr()), U, c_void_p(d_utt.data_ptr()), P, None, c_void_p(d_off.data_ptr()), None,
                                 c_void_p(d_roff.data_ptr()), 0.0, None, 2, c_void_p(out.data_ptr()), c_void_p(out.data_ptr()),
                                 c_void_p(ed.data_ptr()))
    with pytest.raises(EngineError, match="lattice states"):
        _lib.check(rc)
    # ... and the entry still serves a good call
    _check("after refusals", _logits(rng, 20), [20], [[E, np.array([1, 2], np.int32)]], [np.array([1], np.int32)])


# ---- the engine entries ----

def _engine_case(dtype, seed=5100):
    """test_gpu_ctc.py's net with three utterances, their references and hypothesis lists"""
    rng = np.random.default_rng(seed)
    eng, oracle = make_pair(rng, max_frames=512, compute_dtype=dtype, **KW)
    utt = [60, 35, 48]
    refs = [_labels(rng, 9, repeats=1), _labels(rng, 5), _labels(rng, 7)]
    hyps = [[refs[0], np.delete(refs[0], 2), E, _labels(rng, 12)], [_labels(rng, 4), refs[1][:3]], [_labels(rng, 6), refs[2], _labels(rng, 2)]]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    return eng, oracle, utt, X, refs, hyps


def _tables(refs, hyps):
    return (np.concatenate(refs).astype(np.int32), np.array([r.size for r in refs], np.int32)) + pair_tables(hyps)


def _restated_batch(z, utt, hyps, refs, cw):
    zs, want = _restate(z, utt, hyps, refs, cw)
    return sum(w[0] for w in want), np.concatenate([w[1] for w in want]), want


@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
def test_training_call(gpu, dtype):
    """dLogits, batch_loss, num_frames and the step's average against the restatement on the oracle's train-mode logits of
    the same pass; the parameter gradients against the oracle's backward pass from the restated dLogits (in bf16 mode the
    output layer's dW is computed from the twin of dLogits the gradient kernel writes: its gradient is the check on the twin).
    fp32: the bounds above, loss rtol 2e-5 and the gradient tolerances of tests/test_gpu_ctc.py; bf16: those of
    tests/test_gpu_bf16_mode.py (relative Frobenius error <= 2e-3, loss rtol 5e-4)."""
    from tfkaldi_amd import _lib
    eng, oracle, utt, X, refs, hyps = _engine_case(dtype)
    cw, T = 0.3, sum(utt)
    labels, lab, counts, hl, hn = _tables(refs, hyps)
    eng.accumulate_ctc_mwer(X, utt, labels, lab, counts, hl, hn, ctc_weight=cw)
    z = oracle.forward_logits(X)
    loss, dlog, want = _restated_batch(z, utt, hyps, refs, cw)
    oracle.backward_from_dlogits(dlog, loss, int(lab.sum()))
    got_loss, got_n = eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES)
    got_dlog, got = eng.debug_fetch(_lib.DBG_LOGITS, 0, T), engine_grads(eng)
    keys = [k for k in oracle.G if not (k.startswith("b") and not k.startswith("beta") and k != "b%d" % oracle.L)]
    fro = lambda g, w: float(np.linalg.norm(np.asarray(g, np.float64) - w) / max(np.linalg.norm(w), 1e-30))
    print("ctc-mwer training %-12s loss %.1e dlogits max %.1e fro %.1e | gradients fro %s"
          % (dtype, abs(got_loss - loss) / loss, np.abs(got_dlog - dlog).max(), fro(got_dlog, dlog),
             " ".join("%s %.1e" % (k, fro(got[k], oracle.G[k])) for k in keys)))
    assert got_n == lab.sum() and np.abs(dlog).max() > 1e-2
    if dtype == "bfloat16":
        np.testing.assert_allclose(got_loss, loss, rtol=5e-4)
        assert fro(got_dlog, dlog) <= 2e-3
        for k in keys:
            assert fro(got[k], oracle.G[k]) <= 2e-3, (k, fro(got[k], oracle.G[k]))
    else:
        assert_close("batch_loss", got_loss, loss, 2e-5, 0)
        _compare("training " + dtype, z, utt, hyps, refs, cw, (np.array([w[2] for w in want]), [w[3] for w in want],
                                                              [w[4] for w in want], got_dlog))
        for k in keys:
            w = oracle.G[k]
            assert_close("G[%s]" % k, got[k], w, rtol=2e-4, atol=2e-5 * max(np.abs(w).max(), 1e-3))
    avg = eng.apply()
    np.testing.assert_allclose(avg, got_loss / got_n, rtol=1e-6)
    eng.close()


def test_raw_entries_equal_the_plain_ones_bit_for_bit(gpu):
    from tfkaldi_amd import _lib
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(5200)
    D, C = 4, 2
    eng, _ = make_pair(rng, max_frames=256, **dict(KW, input_dim=D * (2 * C + 1)))
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 5, 63)]
    lens = [u.shape[0] for u in utts]
    refs = [_labels(rng, 6), _labels(rng, 2), _labels(rng, 9)]
    hyps = [[refs[0], E, _labels(rng, 4)], [], [_labels(rng, 8), _labels(rng, 3)]]
    labels, lab, counts, hl, hn = _tables(refs, hyps)
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)
    spliced = np.concatenate([u.spliced() for u in utts])
    out = []
    for train in (True, False):
        for how in ("plain", "raw"):
            eng.eval_finish()
            if how == "plain":
                eng.accumulate_ctc_mwer(spliced, lens, labels, lab, counts, hl, hn, ctc_weight=0.2, train=train)
            else:
                eng.accumulate_ctc_mwer_raw(raw, lens, C, labels, lab, counts, hl, hn, ctc_weight=0.2, cmvn=cmvn_table(utts),
                                            train=train)
            out.append((eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES),
                        eng.debug_fetch(_lib.DBG_LOGITS, 0, sum(lens)).tobytes()))
        assert out[-1] == out[-2] and np.isfinite(out[-1][0]) and out[-1][1] == lab.sum()
    assert out[0][2] != out[2][2]  # (training left dLogits, evaluation the logits)
    eng.close()


def test_eval_variant(gpu):
    """the loss on evaluation-mode logits; parameters, G and the moments untouched; inside a step, between an accumulate and
    the apply, the step finishes as if nothing had been evaluated"""
    from tfkaldi_amd import _lib
    eng, _, utt, X, refs, hyps = _engine_case("float32", 5300)
    twin, _, _, _, _, _ = _engine_case("float32", 5300)
    cw = 0.3
    labels, lab, counts, hl, hn = _tables(refs, hyps)
    state0 = _engine_state(eng)
    eng.accumulate_ctc_mwer(X, utt, labels, lab, counts, hl, hn, ctc_weight=cw, train=False)
    z = eng.posteriors(X, raw_logits=True)
    loss, _, _ = _restated_batch(z, utt, hyps, refs, cw)
    got = eng.eval_finish() * lab.sum()
    print("ctc-mwer eval: loss %.6f, restated %.6f" % (got, loss))
    np.testing.assert_allclose(got, loss, rtol=2e-5)
    state1 = _engine_state(eng)
    assert sorted(state0) == sorted(state1) and all(state0[k] == state1[k] for k in state0)
    for e in (eng, twin):  # a step of two micro-batches; `eng` evaluates in between
        e.accumulate_ctc_mwer(X, utt, labels, lab, counts, hl, hn, ctc_weight=cw)
        if e is eng:
            e.accumulate_ctc_mwer(X[:utt[0]], utt[:1], refs[0], lab[:1], counts[:1], hl[:int(hn[:counts[0]].sum())], hn[:counts[0]],
                                  ctc_weight=1.0, train=False)
            assert np.isfinite(e.eval_finish())  # (reports the evaluation's sums and puts the step's back)
        e.accumulate_ctc(X, utt, labels, lab, last=True)
    a, b = eng.apply(), twin.apply()
    assert a == b
    pa, pb = engine_params(eng), engine_params(twin)
    assert all(pa[k].tobytes() == pb[k].tobytes() for k in pa)
    eng.close()
    twin.close()


BAD = {
    "a negative hypothesis count": (lambda t: t["counts"].__setitem__(1, -1), "utterance 1 has a negative hypothesis count"),
    "a negative hypothesis length": (lambda t: t["hn"].__setitem__(4, -2), "utterance 1, hypothesis 0 has a negative length"),
    "a label out of range": (lambda t: t["hl"].__setitem__(int(t["hn"][:5].sum()), 8), "utterance 1, hypothesis 1: label 8 outside"),
    "a negative label": (lambda t: t["hl"].__setitem__(0, -1), "utterance 0, hypothesis 0: label -1 outside"),
    "a reference label out of range": (lambda t: t["labels"].__setitem__(0, 8), "utterance 0: reference label 8 outside"),
    "a negative ctc_weight": (lambda t: t.__setitem__("cw", -0.5), "ctc_weight"),
    "a ctc_weight that is not finite": (lambda t: t.__setitem__("cw", float("inf")), "ctc_weight"),
    "a hypothesis over 511 labels": (None, "utterance 2, hypothesis 1 has 512 labels"),
    "hyp_count is NULL": (None, "NULL"),
}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_argument_errors(gpu, kind):
    """refused with the utterance and the hypothesis named; the accumulators are untouched and a correct batch trains after"""
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    eng, _, utt, X, refs, hyps = _engine_case("float32", 5400)
    if kind == "a hypothesis over 511 labels":
        hyps[2][1] = np.zeros(512, np.int32)
    labels, lab, counts, hl, hn = _tables(refs, hyps)
    good = dict(labels=labels.copy(), lab=lab.copy(), counts=counts.copy(), hl=hl.copy(), hn=hn.copy(), cw=0.1)
    if kind == "a hypothesis over 511 labels":
        good = None
    eng.accumulate_ctc(X, utt, labels, lab)  # something in the accumulators
    before = (eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES), {k: v.tobytes() for k, v in engine_grads(eng).items()})
    t = dict(labels=labels, lab=lab, counts=counts, hl=hl, hn=hn, cw=0.1)
    fn, message = BAD[kind]
    if fn is not None:
        fn(t)
    with pytest.raises(EngineError, match=message):
        if kind == "hyp_count is NULL":
            ptr = lambda a: a.ctypes.data_as(c_void_p)
            ul = np.asarray(utt, np.int32)
            _lib.check(eng.lib.tfk_accumulate_ctc_mwer(eng._h, ptr(X), X.shape[1], X.shape[0], ptr(ul), ul.size, ptr(labels), ptr(lab),
                                                       None, ptr(hl), ptr(hn), 0.1, 0))
        else:  # (past the binding's own checks: straight to the C entry)
            ptr = lambda a: a.ctypes.data_as(c_void_p)
            ul = np.asarray(utt, np.int32)
            _lib.check(eng.lib.tfk_accumulate_ctc_mwer(eng._h, ptr(X), X.shape[1], X.shape[0], ptr(ul), ul.size, ptr(t["labels"]),
                                                       ptr(t["lab"]), ptr(t["counts"]), ptr(t["hl"]), ptr(t["hn"]), t["cw"], 0))
    after = (eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES), {k: v.tobytes() for k, v in engine_grads(eng).items()})
    assert before == after
    if good is None:
        hyps[2][1] = E
        labels, lab, counts, hl, hn = _tables(refs, hyps)
        good = dict(labels=labels, lab=lab, counts=counts, hl=hl, hn=hn, cw=0.1)
    eng.accumulate_ctc_mwer(X, utt, good["labels"], good["lab"], good["counts"], good["hl"], good["hn"], ctc_weight=good["cw"],
                            last=True)
    assert np.isfinite(eng.apply())
    eng.close()


def test_update_mwer_descends(gpu, tmp_path):
    """CTCTrainer.update_mwer end to end.  A first step with a fixed list moves the output layer against the restated gradient
    (Adam's first update is -lr g / (|g| + eps) element by element, so the inner product of the change with g is negative);
    then, on a model that has learnt to decode and with the trainer's own search, the loss of one fixed batch does not go up
    from the first to the last of 5 steps (a direction check, not a rate)."""
    from test_gpu_ctc_decode import _toy_ctc
    from tfkaldi_amd import _lib
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 3, seed=11)
    tr.initialize()
    inputs, targets = disp.get_batch()
    inputs, targets = inputs[:3], targets[:3]
    eng = tr.engine
    refs = [np.asarray(t, np.int32).reshape(-1) for t in targets]
    hyps = [[r, r[:max(r.size // 2, 1)], E] for r in refs]
    W0, b0 = eng.get(_lib.WEIGHTS, eng.L).astype(np.float64), eng.get(_lib.BIASES, eng.L).astype(np.float64)
    first = tr.update_mwer(inputs, targets, ctc_weight=0.01, hyps=hyps)
    utt = [len(x) for x in inputs]
    H = eng.debug_fetch(_lib.DBG_HIDDEN, eng.L - 1, sum(utt)).astype(np.float64)  # the train-mode input of the output layer
    loss, dlog, _ = _restated_batch(H @ W0 + b0, utt, hyps, refs, 0.01)
    np.testing.assert_allclose(first, loss / sum(r.size for r in refs), rtol=1e-4)
    dW = eng.get(_lib.WEIGHTS, eng.L).astype(np.float64) - W0
    inner = float((dW * (H.T @ dlog)).sum())
    print("ctc-mwer descent: loss %.6f (restated %.6f), <parameter change, restated output-layer gradient> = %.3e"
          % (first, loss / sum(r.size for r in refs), inner))
    assert inner < 0.0
    # The criterion is meant for a model that already decodes: from a random one the N best are noise, the reference has no
    # share of the list's probability and the list changes from step to step.  So: 150 steps on the likelihood first, then
    # a learning rate small enough for descent (3e-3 / 8).
    for _ in range(150):
        tr.update(inputs, targets)
    for _ in range(3):
        tr.halve_learning_rate()
    losses = [tr.update_mwer(inputs, targets, beam_width=8, top_paths=4, add_reference=True) for _ in range(5)]
    print("ctc-mwer descent: %s" % " ".join("%.5f" % l for l in losses))
    assert all(np.isfinite(losses)) and losses[-1] <= losses[0]
    ev = tr.evaluate_mwer(inputs, targets, beam_width=8, top_paths=4, add_reference=True)
    assert np.isfinite(ev) and ev >= 0.0
    tr.close()
