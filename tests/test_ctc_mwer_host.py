"""The MWER criterion (expected label errors over an N-best list, include/tfkaldi_hip.h at tfk_accumulate_ctc_mwer) on the
host: a float64 restatement built from the CTC oracle, its gradient formula against central differences, the package's
expected_label_errors / pair_tables against it and against known answers, and the Python plumbing (argument checks of
CTCTrainer.update_mwer, the dispatch of a CtcMwerMicroBatch) with a stub engine.  No GPU."""
import numpy as np
import pytest

from oracle.ctc_oracle import ctc_loss_and_grad_vec, log_softmax
from test_ctc_decode_host import levenshtein
from tfkaldi_amd.neuralNetworks.ctc_mwer import expected_label_errors, pair_tables

E = np.zeros(0, np.int32)


def mwer_restated(z, hyps, ref, ctc_weight=0.0):
    """float64 statement of the criterion for ONE utterance: logits z [T, O], hyps = a list of label arrays, ref = the
    reference.  Returns (loss, grad [T, O], risk, scores [N], edits [N], weights [N]):
      scores_i = log p(hyps_i | z) (-inf: infeasible), edits_i = Levenshtein(hyps_i, ref),
      p = softmax of the scores over the list, risk = sum p e, weights = p (e - risk),
      loss = risk + ctc_weight * -log p(ref | z), grad = sum_i weights_i occ_i + ctc_weight * (softmax - occ_ref)
    with occ = softmax - (the CTC oracle's gradient): the state posteriors folded onto the classes."""
    z = np.asarray(z, dtype=np.float64)
    soft = np.exp(log_softmax(z)) if z.shape[0] else np.zeros_like(z)
    N = len(hyps)
    scores, occ = np.full(N, -np.inf), []
    for i, h in enumerate(hyps):
        loss, g = ctc_loss_and_grad_vec(z, np.asarray(h, dtype=np.int64).reshape(-1))
        scores[i] = -loss if np.isfinite(loss) else -np.inf
        occ.append(soft - g if np.isfinite(loss) else np.zeros_like(z))
    edits = np.array([levenshtein(list(np.asarray(h).reshape(-1)), list(np.asarray(ref).reshape(-1))) for h in hyps],
                     dtype=np.int64)
    ok = scores > -np.inf
    p = np.zeros(N)
    if ok.any():
        ex = np.where(ok, np.exp(np.where(ok, scores, 0.0) - scores[ok].max()), 0.0)
        p = ex / ex.sum()
    risk = float((p * edits).sum())
    w = p * (edits - risk)
    grad = np.zeros_like(z)
    for wi, o in zip(w, occ):
        grad += wi * o
    loss = risk
    if ctc_weight > 0:
        ref_loss, g = ctc_loss_and_grad_vec(z, np.asarray(ref, dtype=np.int64).reshape(-1))
        loss = loss + ctc_weight * ref_loss  # (+inf for a reference its utterance is too short for; g is zero then)
        grad += ctc_weight * g
    return loss, grad, risk, scores, edits, w


def _draw(rng, k):
    T, O = int(rng.integers(3, 14)), int(rng.integers(2, 7))
    z = 2.0 * rng.standard_normal((T, O))
    lab = lambda n: rng.integers(0, O - 1, size=n).astype(np.int32)
    ref = lab(int(rng.integers(1, max(T // 3, 1) + 1)))
    N = int(rng.integers(1, 7))
    hyps = [lab(int(rng.integers(0, max(T // 3, 1) + 1))) for _ in range(N)]
    if k % 2 == 0:  # at least two feasible hypotheses with different edits
        hyps = [ref.copy(), E] + hyps[:4]
    return z, hyps, ref, (0.0, 0.3)[k % 3 == 0]


def _case(rng, k):
    """a random case; one whose list has two feasible hypotheses with different edits is drawn again until the list is not
    degenerate -- no single edit count holds more than 90% of the list's probability -- so that its gradient is not
    vanishingly small by construction (a property of the inputs, read off the scores)"""
    while True:
        z, hyps, ref, cw = _draw(rng, k)
        _, _, _, scores, edits, _ = mwer_restated(z, hyps, ref)
        ok = np.isfinite(scores)
        mixed = ok.sum() >= 2 and np.unique(edits[ok]).size >= 2
        if not mixed and k % 2 == 1:
            return z, hyps, ref, cw
        if mixed:
            p = expected_label_errors(scores, edits)[1]
            if max(p[edits == e].sum() for e in np.unique(edits)) <= 0.9:
                return z, hyps, ref, cw


def test_gradient_formula_against_central_differences():
    """dL/dz = sum_i w_i occ_i + ctc_weight (softmax - occ_ref) against (L(z + h) - L(z - h)) / 2h, h = 1e-5: at most 1e-8
    apart on 24 random cases (T <= 13, O in 2..6, 1..6 hypotheses, with and without the CTC term)"""
    rng = np.random.default_rng(4100)
    h, worst, sure = 1e-5, 0.0, 0
    for k in range(24):
        z, hyps, ref, cw = _case(rng, k)
        loss, grad, risk, scores, edits, w = mwer_restated(z, hyps, ref, cw)
        assert np.isfinite(loss)
        num = np.zeros_like(z)
        for t in range(z.shape[0]):
            for c in range(z.shape[1]):
                zp, zm = z.copy(), z.copy()
                zp[t, c] += h
                zm[t, c] -= h
                num[t, c] = (mwer_restated(zp, hyps, ref, cw)[0] - mwer_restated(zm, hyps, ref, cw)[0]) / (2 * h)
        err = np.abs(num - grad).max()
        worst = max(worst, err)
        assert err <= 1e-8, (k, err)
        assert np.abs(grad.sum(axis=1)).max() <= 1e-13, k  # every row sums to zero: both parts are differences of distributions
        feasible = np.isfinite(scores)
        if feasible.sum() >= 2 and np.unique(edits[feasible]).size >= 2:
            sure += 1
            assert np.abs(grad).max() > 1e-2, (k, np.abs(grad).max())  # (not a check of zeros)
    print("central differences: largest |numeric - analytic| %.2e over 24 cases, %d with a non-trivial list" % (worst, sure))
    assert sure >= 12


def test_expected_label_errors_known_answers():
    risk, p, w = expected_label_errors([-3.0, -3.0], [0, 2])
    assert risk == 1.0 and p.tolist() == [0.5, 0.5] and w.tolist() == [-0.5, 0.5]
    risk, p, w = expected_label_errors([-7.5], [4])
    assert risk == 4.0 and p.tolist() == [1.0] and w.tolist() == [0.0]
    risk, p, w = expected_label_errors([-1.0, -2.0, -30.0], [3, 3, 3])
    assert abs(risk - 3.0) <= 1e-15 and np.abs(w).max() <= 1e-15
    risk, p, w = expected_label_errors([-np.inf, -np.inf], [1, 2])
    assert risk == 0.0 and p.tolist() == [0.0, 0.0] and w.tolist() == [0.0, 0.0]
    risk, p, w = expected_label_errors([], [])
    assert risk == 0.0 and p.size == 0 and w.size == 0
    risk, p, w = expected_label_errors([-2.0, -np.inf, -2.0], [1, 100, 3])
    assert p[1] == 0.0 and w[1] == 0.0 and risk == 2.0 and w.tolist() == [-0.5, 0.0, 0.5]
    assert p.dtype == np.float64 and w.dtype == np.float64
    risk, p, w = expected_label_errors(np.array([-2000.0, -2001.0], np.float32), [0, 5])  # far below exp's range: relative
    assert abs(p[0] - 1.0 / (1.0 + np.exp(-1.0))) <= 1e-15 and abs(risk - 5.0 * p[1]) <= 1e-15
    with pytest.raises(ValueError):
        expected_label_errors([0.0, 1.0], [1])
    with pytest.raises(ValueError):
        expected_label_errors([np.nan], [1])


def test_expected_label_errors_against_the_restatement():
    rng = np.random.default_rng(4101)
    for k in range(30):
        z, hyps, ref, _ = _case(rng, k)
        if k % 5 == 0:
            hyps = hyps + [np.zeros(z.shape[0] + 1, np.int32)]  # an infeasible pair
        _, _, risk, scores, edits, w = mwer_restated(z, hyps, ref)
        got_risk, p, got_w = expected_label_errors(scores, edits)
        assert abs(got_risk - risk) <= 1e-12 * max(risk, 1.0)
        assert np.abs(got_w - w).max() <= 1e-12 * max(np.abs(edits).max(), 1)
        assert abs(got_w.sum()) <= 1e-15 * max(np.abs(edits).max(), 1) * len(hyps)
        assert abs(p.sum() - 1.0) <= 1e-15 * len(hyps) and np.all(p[~np.isfinite(scores)] == 0.0)


def test_weights_sum_to_zero():
    rng = np.random.default_rng(4102)
    for _ in range(50):
        n = int(rng.integers(1, 7))
        _, _, w = expected_label_errors(-10.0 * rng.random(n), np.ones(n) if n == 3 else rng.integers(0, 2, n))
        assert abs(w.sum()) <= 1e-15


def test_pair_tables():
    a, b, c = np.array([1, 2], np.int64), np.array([3], np.int32), [4, 4, 0]
    refs = [np.array([1, 2]), np.array([7]), np.array([4, 4, 0]), E]
    counts, labels, lens = pair_tables([[a, b], [], [c, E], [E]])
    assert counts.dtype == labels.dtype == lens.dtype == np.int32
    assert counts.tolist() == [2, 0, 2, 1] and lens.tolist() == [2, 1, 3, 0, 0] and labels.tolist() == [1, 2, 3, 4, 4, 0]
    assert np.concatenate([[0], np.cumsum(lens)]).tolist() == [0, 2, 3, 6, 6, 6]  # the offsets the engine derives
    counts, labels, lens = pair_tables([[a, b], [], [c, E], [E]], refs, add_reference=True)
    # utterance 0 and 2 list their reference already, 1 gains it, 3's (empty) reference is its (empty) hypothesis
    assert counts.tolist() == [2, 1, 2, 1] and lens.tolist() == [2, 1, 1, 3, 0, 0] and labels.tolist() == [1, 2, 3, 7, 4, 4, 0]
    counts, labels, lens = pair_tables([[b], [b]], [np.array([3, 3]), np.array([3])], add_reference=True)
    assert counts.tolist() == [2, 1] and lens.tolist() == [1, 2, 1]  # [3] is not [3, 3]
    counts, labels, lens = pair_tables([[], []])
    assert counts.tolist() == [0, 0] and labels.size == 0 and lens.size == 0 and labels.dtype == np.int32
    with pytest.raises(ValueError):
        pair_tables([[a]], None, add_reference=True)
    with pytest.raises(ValueError):
        pair_tables([[a]], [a, b])


def test_update_mwer_argument_checks():
    """refused with ValueError before anything reaches the device (the trainer here has no engine at all)"""
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    tr = object.__new__(CTCTrainer)
    X, y = [np.zeros((5, 3), np.float32)], [np.array([1], np.int32)]
    for fn in (tr.update_mwer, tr.evaluate_mwer):
        with pytest.raises(ValueError, match="top_paths"):
            fn(X, y, beam_width=4, top_paths=8)
        with pytest.raises(ValueError, match="top_paths"):
            fn(X, y, beam_width=4, top_paths=0)
        with pytest.raises(ValueError, match="beam_width"):
            fn(X, y, lm=object())
        with pytest.raises(ValueError, match="language model"):
            fn(X, y, lm=object(), hyps=[[E]])
        with pytest.raises(ValueError, match="label_topk"):
            fn(X, y, label_topk=3, hyps=[[E]])
        with pytest.raises(ValueError, match="beam_width"):
            fn(X, y)
        with pytest.raises(ValueError, match="hypothesis lists"):
            fn(X, y, hyps=[[E], [E]])
        with pytest.raises(ValueError, match="ctc_weight"):
            fn(X, y, beam_width=4, ctc_weight=-1.0)
        with pytest.raises(ValueError, match="ctc_weight"):
            fn(X, y, beam_width=4, ctc_weight=float("nan"))
    assert tr.evaluate_mwer(None, None, beam_width=4) is None


class _StubEngine(object):
    """records its calls; the searches return two utterances' 3 paths, the last of each a padding path (score -inf)"""

    def __init__(self):
        self.calls = []

    def _search(self, name, args, kw):
        self.calls.append((name, args, kw))
        found = [[np.array([1, 2], np.int32), np.array([1], np.int32), E], [np.array([0], np.int32), E, E]]
        score = [np.array([-1.0, -2.0, -np.inf], np.float32), np.array([-0.5, -3.0, -np.inf], np.float32)]
        return found, score, None

    def ctc_beam(self, *args, **kw):
        return self._search("ctc_beam", args, kw)

    def ctc_beam_lm(self, *args, **kw):
        return self._search("ctc_beam_lm", args, kw) + (None,)

    def ctc_beam_raw(self, *args, **kw):
        return self._search("ctc_beam_raw", args, kw)

    def accumulate_ctc_mwer(self, *args, **kw):
        self.calls.append(("accumulate_ctc_mwer", args, kw))

    def accumulate_ctc_mwer_raw(self, *args, **kw):
        self.calls.append(("accumulate_ctc_mwer_raw", args, kw))

    def accumulate_ctc(self, *args, **kw):
        self.calls.append(("accumulate_ctc", args, kw))


def test_dispatch_of_a_mwer_microbatch():
    from tfkaldi_amd.dataparallel import CtcMicroBatch, CtcMwerMicroBatch, _accumulate, _eval_accumulate
    X, utt = np.zeros((9, 4), np.float32), np.array([5, 4], np.int32)
    ref, ref_len = np.array([1, 2, 3], np.int32), np.array([2, 1], np.int32)
    # search settings: decode first, then accumulate; padding paths dropped; the reference joins the list that lacks it
    eng = _StubEngine()
    mb = CtcMwerMicroBatch(X, utt, ref, ref_len, beam_width=8, top_paths=3, add_reference=True, ctc_weight=0.25)
    _accumulate(eng, mb, True)
    assert [c[0] for c in eng.calls] == ["ctc_beam", "accumulate_ctc_mwer"]
    assert eng.calls[0][2] == {"beam_width": 8, "top_paths": 3}
    args, kw = eng.calls[1][1:]
    assert args[0] is X and args[2] is ref
    counts, labels, lens = args[4:7]
    assert counts.tolist() == [2, 3] and lens.tolist() == [2, 1, 1, 0, 1] and labels.tolist() == [1, 2, 1, 0, 3]
    assert kw == {"ctc_weight": 0.25, "last": True, "train": True}
    # with a model and label pruning, evaluation
    eng = _StubEngine()
    lm = object()
    mb = CtcMwerMicroBatch(X, utt, ref, ref_len, beam_width=8, lm=lm, label_topk=5)
    assert mb.top_paths == 8
    _eval_accumulate(eng, mb)
    assert [c[0] for c in eng.calls] == ["ctc_beam_lm", "accumulate_ctc_mwer"]
    assert eng.calls[0][2] == {"beam_width": 8, "top_paths": 8, "lm": lm, "label_topk": 5}
    assert eng.calls[1][1][4].tolist() == [2, 2] and eng.calls[1][2] == {"ctc_weight": 0.0, "last": False, "train": False}
    # pair tables given: no search; unspliced frames go to the raw entry
    eng = _StubEngine()
    counts, labels, lens = pair_tables([[E], [np.array([3], np.int32), E]])
    mb = CtcMwerMicroBatch(X, utt, ref, ref_len, context_width=2, cmvn=None, hyp_counts=counts, hyp_labels=labels, hyp_lens=lens)
    _accumulate(eng, mb, False)
    assert [c[0] for c in eng.calls] == ["accumulate_ctc_mwer_raw"]
    assert eng.calls[0][1][2] == 2 and eng.calls[0][1][5] is counts and eng.calls[0][2]["last"] is False
    # ... and with add_reference the tables are rebuilt with the references in them
    eng = _StubEngine()
    mb = CtcMwerMicroBatch(X, utt, ref, ref_len, hyp_counts=counts, hyp_labels=labels, hyp_lens=lens, add_reference=True)
    _accumulate(eng, mb, True)
    assert eng.calls[0][1][4].tolist() == [2, 2] and eng.calls[0][1][6].tolist() == [0, 2, 1, 0]
    # a plain CTC micro-batch still goes where it went
    eng = _StubEngine()
    _accumulate(eng, CtcMicroBatch(X, utt, ref, ref_len), True)
    assert [c[0] for c in eng.calls] == ["accumulate_ctc"]
    for bad in (dict(), dict(beam_width=4, hyp_counts=counts, hyp_labels=labels, hyp_lens=lens), dict(hyp_counts=counts),
                dict(beam_width=4, top_paths=5)):
        with pytest.raises(ValueError):
            CtcMwerMicroBatch(X, utt, ref, ref_len, **bad)
