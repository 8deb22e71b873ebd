"""Which Engine method a training micro-batch reaches, and with which arguments: _accumulate / _eval_accumulate /
_label_errors of tfkaldi_amd.dataparallel over a recording stand-in engine, for every kind of micro-batch, spliced and
unspliced, training and evaluation -- the exact sequence of (method, positional arguments, keywords).  Then CTCTrainer over
the same stand-in: which utterances' flags and hypothesis lists each micro-batch carries, and the refusals.  No GPU."""
import numpy as np
import pytest

from tfkaldi_amd.dataparallel import (CtcMicroBatch, CtcMmiMicroBatch, CtcMwerMicroBatch, CtcWildMicroBatch, DataParallel,
                                      RawMicroBatch, StackedRawMicroBatches, _accumulate, _eval_accumulate, _label_errors)
from tfkaldi_amd.neuralNetworks.ctc_lm import GraphLM
from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer

E = np.zeros(0, np.int32)


class RecordingEngine(object):
    """every public method exists, records (name, args, kw) and answers as the engine would: the searches find, for two
    utterances, 3 paths each of which the last is a padding path (score -inf); ctc_score scores every pair it is given"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def method(*args, **kw):
            self.calls.append((name, args, kw))
            if name.startswith("ctc_beam"):
                found = [[np.array([1, 2], np.int32), np.array([1], np.int32), E], [np.array([0], np.int32), E, E]]
                score = [np.array([-1.0, -2.0, -np.inf], np.float32), np.array([-0.5, -3.0, -np.inf], np.float32)]
                edits = np.array([1, 2], np.int32) if "labels" in kw else None
                return (found, score, None, edits) if "_lm" in name else (found, score, edits)
            if name.startswith("ctc_greedy"):
                return [np.array([1], np.int32), E], np.array([3, 1], np.int32)
            if name.startswith("ctc_score"):
                counts = args[3] if name.endswith("_raw") else args[2]
                return ([np.linspace(-2.0, -1.0, n).astype(np.float32) for n in counts],  # (the LAST pair scores best)
                        [np.arange(n, dtype=np.int32) + 1 for n in counts])
            return 0.0 if name in ("apply", "eval_finish", "apply_end") else None
        return method


def _same(got, want):
    if isinstance(want, np.ndarray):
        return got is want
    if isinstance(want, list):
        return np.asarray(got).tolist() == want and not isinstance(got, (int, float))
    return got is want or (type(got) is type(want) and got == want)


def _assert_calls(eng, want):
    assert [c[0] for c in eng.calls] == [w[0] for w in want]
    for (name, args, kw), (_, want_args, want_kw) in zip(eng.calls, want):
        assert len(args) == len(want_args) and all(_same(a, w) for a, w in zip(args, want_args)), (name, args)
        assert sorted(kw) == sorted(want_kw) and all(_same(kw[k], want_kw[k]) for k in want_kw), (name, kw)


X, UTT = np.zeros((9, 4), np.float32), np.array([5, 4], np.int32)
REF, REF_LEN = np.array([1, 2, 3], np.int32), np.array([2, 1], np.int32)
CMVN = np.ones((2, 2, 4), np.float32)
WILD = np.array([1, 0, 1, 0, 1], np.uint8)
COUNTS, HYP_LABELS, HYP_LENS = np.array([1, 2], np.int32), np.array([3], np.int32), np.array([0, 1, 0], np.int32)
# what the stand-in's search leaves after its padding paths are dropped: [1 2], [1] | [0], []
FOUND = ([2, 2], [1, 2, 1, 0], [2, 1, 1, 0])
FOUND_WITH_REFERENCE = ([2, 3], [1, 2, 1, 0, 3], [2, 1, 1, 0, 1])
GRAPH = GraphLM(np.zeros((1, 5), np.float32), np.zeros((1, 5), np.int64), start=0)
LM = object()

RAW = [pytest.param(False, id="spliced"), pytest.param(True, id="unspliced")]
PASSES = [pytest.param("train_last", id="last"), pytest.param("train", id="not_last"), pytest.param("eval", id="eval")]


def _run(mb, how):
    eng = RecordingEngine()
    if how == "eval":
        assert _eval_accumulate(eng, mb) is None
    else:
        assert _accumulate(eng, mb, how == "train_last") is None
    return eng


def _frames(raw):
    """(constructor keywords, positional arguments in front of the labels, the raw form's cmvn keyword)"""
    if raw:
        return dict(context_width=2, cmvn=CMVN), (X, UTT, 2, REF, REF_LEN), dict(cmvn=CMVN)
    return {}, (X, UTT, REF, REF_LEN), {}


@pytest.mark.parametrize("how", PASSES)
@pytest.mark.parametrize("raw", RAW)
def test_plain_ctc(raw, how):
    ctor, args, cmvn = _frames(raw)
    eng = _run(CtcMicroBatch(X, UTT, REF, REF_LEN, **ctor), how)
    if raw:  # (evaluation of unspliced frames goes through the training method's train switch, and gives no `last`)
        kw = dict(cmvn, train=False) if how == "eval" else dict(cmvn, last=how == "train_last")
        _assert_calls(eng, [("accumulate_ctc_raw", args, kw)])
    elif how == "eval":
        _assert_calls(eng, [("eval_accumulate_ctc", args, {})])
    else:
        _assert_calls(eng, [("accumulate_ctc", args, dict(last=how == "train_last"))])


@pytest.mark.parametrize("how", PASSES)
@pytest.mark.parametrize("raw", RAW)
def test_wild(raw, how):
    ctor, args, cmvn = _frames(raw)
    eng = _run(CtcWildMicroBatch(X, UTT, REF, REF_LEN, wild=WILD, penalty=0.5, **ctor), how)
    kw = dict(cmvn, wild=WILD, penalty=0.5, last=how == "train_last", train=how != "eval")
    _assert_calls(eng, [("accumulate_ctc_wild_raw" if raw else "accumulate_ctc_wild", args, kw)])


@pytest.mark.parametrize("how", PASSES)
@pytest.mark.parametrize("raw", RAW)
def test_mmi(raw, how):
    ctor, args, cmvn = _frames(raw)
    eng = _run(CtcMmiMicroBatch(X, UTT, REF, REF_LEN, GRAPH, lm_scale=0.5, ctc_weight=0.25, **ctor), how)
    kw = dict(cmvn, lm_scale=0.5, ctc_weight=0.25, last=how == "train_last", train=how != "eval")
    _assert_calls(eng, [("ctc_set_den", (GRAPH,), {}), ("accumulate_ctc_mmi_raw" if raw else "accumulate_ctc_mmi", args, kw)])


@pytest.mark.parametrize("how", PASSES)
@pytest.mark.parametrize("raw", RAW)
def test_mwer_with_its_tables(raw, how):
    ctor, args, cmvn = _frames(raw)
    eng = _run(CtcMwerMicroBatch(X, UTT, REF, REF_LEN, hyp_counts=COUNTS, hyp_labels=HYP_LABELS, hyp_lens=HYP_LENS,
                                 ctc_weight=0.25, **ctor), how)
    kw = dict(cmvn, ctc_weight=0.25, last=how == "train_last", train=how != "eval")
    _assert_calls(eng, [("accumulate_ctc_mwer_raw" if raw else "accumulate_ctc_mwer", args + (COUNTS, HYP_LABELS, HYP_LENS), kw)])
    # add_reference: the tables are rebuilt with the references in them
    eng = _run(CtcMwerMicroBatch(X, UTT, REF, REF_LEN, hyp_counts=COUNTS, hyp_labels=HYP_LABELS, hyp_lens=HYP_LENS,
                                 add_reference=True, **ctor), how)
    kw = dict(kw, ctc_weight=0.0)
    _assert_calls(eng, [("accumulate_ctc_mwer_raw" if raw else "accumulate_ctc_mwer",
                         args + ([2, 2], [1, 2, 3], [0, 2, 1, 0]), kw)])


@pytest.mark.parametrize("search", [dict(), dict(lm=LM), dict(label_topk=5), dict(lm=LM, label_topk=5)],
                         ids=["beam", "lm", "topk", "lm_topk"])
@pytest.mark.parametrize("how", PASSES)
@pytest.mark.parametrize("raw", RAW)
def test_mwer_with_its_search(raw, how, search):
    ctor, args, cmvn = _frames(raw)
    eng = _run(CtcMwerMicroBatch(X, UTT, REF, REF_LEN, beam_width=8, top_paths=3, ctc_weight=0.25, **ctor, **search), how)
    entry = ("ctc_beam_lm" if "lm" in search else "ctc_beam") + ("_raw" if raw else "")
    kw = dict(cmvn, ctc_weight=0.25, last=how == "train_last", train=how != "eval")
    _assert_calls(eng, [(entry, (X, UTT), dict(search, beam_width=8, top_paths=3, **ctor)),
                        ("accumulate_ctc_mwer_raw" if raw else "accumulate_ctc_mwer", args + FOUND, kw)])
    # top_paths defaults to the beam width; add_reference reaches pair_tables
    mb = CtcMwerMicroBatch(X, UTT, REF, REF_LEN, beam_width=8, add_reference=True, **ctor, **search)
    assert mb.top_paths == 8
    eng = _run(mb, how)
    _assert_calls(eng, [(entry, (X, UTT), dict(search, beam_width=8, top_paths=8, **ctor)),
                        ("accumulate_ctc_mwer_raw" if raw else "accumulate_ctc_mwer", args + FOUND_WITH_REFERENCE,
                         dict(kw, ctc_weight=0.0))])


@pytest.mark.parametrize("how", PASSES)
def test_frame_level_microbatches(how):
    y, lens = np.arange(9, dtype=np.int32), np.array([5, 4], np.int32)
    last = dict() if how == "eval" else dict(last=how == "train_last")
    pre = "eval_" if how == "eval" else ""
    for cmvn in (None, CMVN):
        eng = _run(RawMicroBatch(X, y, lens, 2, cmvn), how)
        _assert_calls(eng, [(pre + "accumulate_raw", (X, y, lens, 2), dict(last, cmvn=cmvn))])
        eng = _run(StackedRawMicroBatches(X, y, lens, 2, cmvn, (1, 1)), how)
        _assert_calls(eng, [(pre + "accumulate_stacked_raw", (X, y, lens, 2, [1, 1]), dict(last, cmvn=cmvn))])
    eng = _run((X, y), how)
    _assert_calls(eng, [(pre + "accumulate", (X, y), last)])


# ---- _label_errors: greedy, beam, beam + lm + topk, rescoring; spliced and unspliced ----
@pytest.mark.parametrize("raw", RAW)
def test_label_errors_reach_the_search_entries(raw):
    ctor, _, cmvn = _frames(raw)
    tail = "_raw" if raw else ""
    mb = CtcMicroBatch(X, UTT, REF, REF_LEN, **ctor)
    refs = dict(ctor, labels=REF, label_lens=REF_LEN)
    eng = RecordingEngine()
    assert _label_errors(eng, mb) == (4, 3)
    _assert_calls(eng, [("ctc_greedy" + tail, (X, UTT), refs)])
    eng = RecordingEngine()
    assert _label_errors(eng, mb, beam_width=8) == (3, 3)
    _assert_calls(eng, [("ctc_beam" + tail, (X, UTT), dict(refs, beam_width=8))])
    eng = RecordingEngine()
    assert _label_errors(eng, mb, beam_width=8, lm=LM, label_topk=5) == (3, 3)
    _assert_calls(eng, [("ctc_beam_lm" + tail, (X, UTT), dict(refs, beam_width=8, lm=LM, label_topk=5))])
    eng = RecordingEngine()
    assert _label_errors(eng, mb, beam_width=8, label_topk=5) == (3, 3)
    _assert_calls(eng, [("ctc_beam" + tail, (X, UTT), dict(refs, beam_width=8, label_topk=5))])
    # rescoring: the N best without their padding paths go to ctc_score as pairs; the stand-in ranks the last pair best
    eng = RecordingEngine()
    assert _label_errors(eng, mb, beam_width=8, rescore_paths=3) == (4, 3)
    score_args = (X, UTT) + ((2,) if raw else ()) + ([2, 2], [1, 2, 1, 0], [2, 1, 1, 0])
    _assert_calls(eng, [("ctc_beam" + tail, (X, UTT), dict(ctor, beam_width=8, top_paths=3)),
                        ("ctc_score" + tail, score_args, dict(cmvn, ref_labels=REF, ref_lens=REF_LEN))])
    eng = RecordingEngine()
    _label_errors(eng, mb, beam_width=8, lm=None, label_topk=5, rescore_paths=2)
    assert eng.calls[0][0] == "ctc_beam" + tail and eng.calls[0][2] == dict(ctor, beam_width=8, top_paths=2, label_topk=5)
    with pytest.raises(TypeError, match="label errors need CTC micro-batches"):
        _label_errors(RecordingEngine(), (X, np.zeros(9, np.int32)))


REFUSALS = [(dict(rescore_paths=3), "rescoring re-ranks the N best of a beam search: give beam_width with rescore_paths"),
            (dict(lm=LM), "a language model ranks the prefixes of a beam search: give beam_width with lm"),
            (dict(label_topk=4), "label_topk prunes a beam search: give beam_width with label_topk"),
            (dict(rescore_paths=3, lm=LM, label_topk=4),
             "rescoring re-ranks the N best of a beam search: give beam_width with rescore_paths"),
            (dict(lm=LM, label_topk=4), "a language model ranks the prefixes of a beam search: give beam_width with lm")]


@pytest.mark.parametrize("kw, message", REFUSALS)
def test_a_search_setting_without_a_beam_is_refused_alike_by_both(kw, message):
    eng = RecordingEngine()
    tr = _trainer(eng, 2)
    with pytest.raises(ValueError) as a:
        _label_errors(eng, (X, None), **kw)  # (before it looks at the micro-batch)
    with pytest.raises(ValueError) as b:
        tr.label_errors(None, None, **kw)  # (before its None for missing data)
    assert str(a.value) == str(b.value) == message and eng.calls == []
    assert tr.label_errors(None, None) is None and tr.label_errors(None, None, beam_width=4, **kw) is None


# ---- CTCTrainer over the stand-in ----
def _trainer(engine, per_minibatch):
    tr = CTCTrainer.__new__(CTCTrainer)  # (the constructor creates a device engine)
    tr.engine, tr.dp, tr.numutterances_per_minibatch = engine, DataParallel(), per_minibatch
    tr.loss_kind, tr.summarywriter = "ctc", None
    return tr


# 5 utterances, 2 per micro-batch: groups (0, 1), (2, 3), (4); the middle one holds only zero-frame utterances
LENS = [3, 2, 0, 0, 4]
XS = [np.full((n, 4), u, np.float32) for u, n in enumerate(LENS)]
YS = [np.array(s, np.int32) for s in ([1], [2, 3], [0], E, [1, 1])]


def test_each_microbatch_gets_its_own_utterances_gap_flags():
    flags = [np.array(f, bool) for f in ([1, 0], [0, 1, 1], [1, 1], [1], [0, 0, 1])]
    for fn, passes in (("update_wild", [(False, True), (True, True)]), ("evaluate_wild", [(False, False)] * 2)):
        eng = RecordingEngine()
        assert getattr(_trainer(eng, 2), fn)(XS, YS, wild=flags, penalty=0.5) == 0.0
        calls = [c for c in eng.calls if c[0] == "accumulate_ctc_wild"]
        assert len(calls) == 2 and [c[0] for c in eng.calls if c[0].startswith("accumulate")] == ["accumulate_ctc_wild"] * 2
        assert [(c[2]["last"], c[2]["train"]) for c in calls] == passes
        assert [c[1][1].tolist() for c in calls] == [[3, 2], [4]] and [c[1][3].tolist() for c in calls] == [[1, 2], [2]]
        assert [c[1][0][:, 0].tolist() for c in calls] == [[0, 0, 0, 1, 1], [4, 4, 4, 4]]
        assert [c[2]["wild"].tolist() for c in calls] == [[1, 0, 0, 1, 1], [0, 0, 1]]
        assert all(c[2]["wild"].dtype == np.uint8 and c[2]["penalty"] == 0.5 for c in calls)


def test_each_microbatch_gets_its_own_utterances_hypotheses():
    hyps = [[np.array([1], np.int32)], [np.array([2], np.int32), E], [np.array([4, 4, 4], np.int32)], [],
            [np.array([1, 1], np.int32), np.array([3], np.int32), E]]
    for fn, passes in (("update_mwer", [(False, True), (True, True)]), ("evaluate_mwer", [(False, False)] * 2)):
        eng = RecordingEngine()
        assert getattr(_trainer(eng, 2), fn)(XS, YS, hyps=hyps, ctc_weight=0.25) == 0.0
        assert [c[0] for c in eng.calls if c[0] not in ("apply", "eval_finish")] == ["accumulate_ctc_mwer"] * 2
        calls = eng.calls[:2]
        assert [(c[2]["last"], c[2]["train"], c[2]["ctc_weight"]) for c in calls] == [p + (0.25,) for p in passes]
        assert [c[1][1].tolist() for c in calls] == [[3, 2], [4]]
        assert [[a.tolist() for a in c[1][4:7]] for c in calls] == [[[1, 2], [1, 2], [1, 1, 0]], [[3], [1, 1, 3], [2, 1, 0]]]
    # the search settings instead: every micro-batch carries them, top_paths defaulting to the beam width
    eng = RecordingEngine()
    tr = _trainer(eng, 2)
    tr.update_mwer(XS[:2], YS[:2], beam_width=4, lm=LM, label_topk=3)
    assert [c[0] for c in eng.calls] == ["ctc_beam_lm", "accumulate_ctc_mwer", "apply"]
    assert eng.calls[0][2] == dict(beam_width=4, top_paths=4, lm=LM, label_topk=3)
    assert eng.calls[1][2] == dict(ctc_weight=0.01, last=True, train=True)


def test_a_batch_without_frames_names_the_method():
    eng = RecordingEngine()
    tr = _trainer(eng, 2)
    xs, ys = [np.zeros((0, 4), np.float32)] * 2, [E] * 2
    tail = ": the batch holds no frames (no micro-batch could be built from 2 utterance(s))"
    for name, step in (("Trainer.update", lambda: tr.update(xs, ys)),
                       ("CTCTrainer.update_mwer", lambda: tr.update_mwer(xs, ys, beam_width=4)),
                       ("CTCTrainer.update_mmi", lambda: tr.update_mmi(xs, ys, GRAPH)),
                       ("CTCTrainer.update_wild", lambda: tr.update_wild(xs, ys))):
        with pytest.raises(ValueError) as err:
            step()
        assert str(err.value) == name + tail
    assert eng.calls == []
    # evaluation of such a batch is no error: nothing is accumulated
    assert tr.evaluate(xs, ys) == tr.evaluate_mwer(xs, ys, beam_width=4) == tr.evaluate_mmi(xs, ys, GRAPH) == 0.0
    assert tr.evaluate_wild(xs, ys) == 0.0 and [c[0] for c in eng.calls] == ["eval_finish"] * 4


def test_the_steps_are_summarised_and_return_the_loss(tmp_path):
    import json
    eng = RecordingEngine()
    tr = _trainer(eng, 2)
    eng.global_step = 7
    tr.start_visualization(str(tmp_path))
    assert tr.update(XS, YS) == tr.update_wild(XS, YS) == tr.update_mmi(XS, YS, GRAPH) == 0.0
    assert tr.update_mwer(XS[:2], YS[:2], beam_width=2) == 0.0 and tr.evaluate_wild(XS, YS) == 0.0
    tr.summarywriter.close()
    lines = [json.loads(l) for l in open(str(tmp_path / "summaries.jsonl"))]
    assert len(lines) == 4 and all(l["step"] == 7 and l["loss"] == 0.0 for l in lines)  # (one per update, none per evaluation)


def test_update_mwer_refuses_its_arguments_in_todays_order():
    tr = _trainer(RecordingEngine(), 2)
    for fn in (tr.update_mwer, tr.evaluate_mwer):
        with pytest.raises(ValueError, match=r"top_paths 9 outside \[1, beam_width = 4\]"):
            fn(XS, YS, beam_width=4, top_paths=9, ctc_weight=-1.0)
        with pytest.raises(ValueError, match="top_paths 0 outside"):
            fn([np.zeros((0, 4), np.float32)], [E], beam_width=4, top_paths=0)  # (also where no micro-batch is built)
        with pytest.raises(ValueError, match="language model"):
            fn(XS, YS, lm=LM, hyps=[[E]] * 5, ctc_weight=-1.0)
        with pytest.raises(ValueError) as err:
            fn(XS, YS, beam_width=4, ctc_weight=-1.0)
        assert str(err.value) == "ctc_weight -1.0 must be finite and >= 0"
    for fn in (tr.update_mmi, tr.evaluate_mmi):
        with pytest.raises(ValueError) as err:
            fn(XS, YS, GRAPH, lm_scale=float("nan"), ctc_weight=-1.0)
        assert str(err.value) == "lm_scale nan must be finite and >= 0"
    assert tr.engine.calls == []


def test_a_non_numeric_weight_is_a_value_error():
    """NEW BEHAVIOUR: only update_wild turned a non-number into the ValueError with the standard text; update_mwer and
    update_mmi let np.isfinite raise TypeError.  One helper now does what update_wild did for all of them."""
    tr = _trainer(RecordingEngine(), 2)
    with pytest.raises(ValueError) as err:
        tr.update_wild(XS, YS, penalty="soft")
    assert str(err.value) == "penalty 'soft' must be finite and >= 0"
    with pytest.raises(ValueError) as err:
        tr.update_mwer(XS, YS, beam_width=4, ctc_weight="heavy")
    assert str(err.value) == "ctc_weight 'heavy' must be finite and >= 0"
    with pytest.raises(ValueError) as err:
        tr.evaluate_mmi(XS, YS, GRAPH, lm_scale=None)
    assert str(err.value) == "lm_scale None must be finite and >= 0"
    assert tr.engine.calls == []
