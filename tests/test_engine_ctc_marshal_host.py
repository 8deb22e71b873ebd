"""What Engine's CTC training methods hand to the C ABI, without the library: every one of the 16 tfk_[eval_]accumulate_ctc*
entries is reached through its public method over a recording stand-in for Engine.lib, and the entry's name, its argument
count (against _lib.SYMBOLS), its scalars and the bytes behind each pointer AT CALL TIME are compared with literals.  Then
the order of the refusals: a call that is wrong in two places raises the first message, given as a literal.  No GPU."""
import ctypes

import numpy as np
import pytest

from tfkaldi_amd import _lib
from tfkaldi_amd.engine import Engine

HANDLE = 0x5A5A0


class RecordingLib(object):
    """stands in for the loaded library: any attribute is an entry that records (name, arguments) and returns 0.  A pointer
    argument is read back while the call is running -- as many bytes as the array `want` holds at its position -- so an
    array that did not outlive the marshalling, or the wrong array, shows; NULL is None, another pointer its address."""

    def __init__(self):
        self.calls, self.want = [], ()

    def __getattr__(self, name):
        def entry(*args):
            seen = []
            for k, a in enumerate(args):
                want = self.want[k] if k < len(self.want) else None
                if not isinstance(a, ctypes.c_void_p):
                    seen.append(a)
                elif a.value is None:
                    seen.append(None)
                elif isinstance(want, np.ndarray):
                    seen.append(ctypes.string_at(a.value, want.nbytes))
                else:
                    seen.append(a.value)
            self.calls.append((name, seen))
            return 0
        return entry


def _engine():
    eng = Engine.__new__(Engine)  # (the constructor loads the library and creates a device engine)
    eng.lib, eng._h, eng.O, eng._den_table = RecordingLib(), ctypes.c_void_p(HANDLE), 5, None
    return eng


# 2 utterances of 3 and 4 frames, 4 features, 1 and 2 labels: the smallest shapes that tell the arguments apart
X = np.arange(28, dtype=np.float32).reshape(7, 4) / 8
UTT = np.array([3, 4], np.int32)
LABELS = np.array([2, 0, 1], np.int32)
LAB = np.array([1, 2], np.int32)
WILD = np.array([1, 0, 0, 1, 1], np.uint8)          # label_lens[u] + 1 flags per utterance
COUNTS = np.array([1, 2], np.int32)                 # MWER pair tables: 3 hypotheses of 1, 0 and 2 labels
HYP_LABELS = np.array([3, 1, 2], np.int32)
HYP_LENS = np.array([1, 0, 2], np.int32)
CMVN = (np.arange(16, dtype=np.float32).reshape(2, 2, 4) + 1) / 4

# per criterion: (stem, the method's own arguments as the caller gives them, what the entry receives for them)
CRITERIA = {
    "": ("", {}, []),
    "wild": ("_wild", dict(wild=WILD, penalty=0.5), [WILD, 0.5]),
    "wild_none": ("_wild", dict(wild=None, penalty=0.25), [None, 0.25]),
    "mwer": ("_mwer", dict(hyp_counts=COUNTS, hyp_labels=HYP_LABELS, hyp_lens=HYP_LENS, ctc_weight=0.25),
             [COUNTS, HYP_LABELS, HYP_LENS, 0.25]),
    "mmi": ("_mmi", dict(lm_scale=0.5, ctc_weight=0.125), [0.5, 0.125]),
}


def _seen(want):
    return [w.tobytes() if isinstance(w, np.ndarray) else w for w in want]


def _call(method, args, kw, want):
    eng = _engine()
    eng.lib.want = want
    assert getattr(eng, method)(*args, **kw) is None
    (name, seen), = eng.lib.calls
    return name, seen


@pytest.mark.parametrize("kind", sorted(CRITERIA))
@pytest.mark.parametrize("last, train, flags", [(True, True, 2), (False, True, 0), (True, False, 0), (False, False, 0)])
def test_spliced_entries(kind, last, train, flags):
    stem, own, received = CRITERIA[kind]
    want = [HANDLE, X, 4, 7, UTT, 2, LABELS, LAB] + received + [flags]
    if stem == "":  # (accumulate_ctc has no train switch: evaluation is eval_accumulate_ctc, which has no `last`)
        name, seen = (_call("accumulate_ctc", (X, UTT, LABELS, LAB), dict(last=last), want) if train else
                      _call("eval_accumulate_ctc", (X, UTT, LABELS, LAB), {}, want))
    else:
        name, seen = _call("accumulate_ctc" + stem, (X, UTT, LABELS, LAB), dict(own, last=last, train=train), want)
    assert name == ("tfk_accumulate_ctc" if train else "tfk_eval_accumulate_ctc") + stem
    assert len(seen) == len(_lib.SYMBOLS[name][1])
    assert seen == _seen(want)


@pytest.mark.parametrize("kind", sorted(CRITERIA))
@pytest.mark.parametrize("cmvn", [None, CMVN], ids=["no_cmvn", "cmvn"])
@pytest.mark.parametrize("last, train, flags", [(True, True, 2), (False, True, 0), (True, False, 0)])
def test_raw_entries(kind, cmvn, last, train, flags):
    stem, own, received = CRITERIA[kind]
    want = [HANDLE, X, 4, 7, UTT, 2, 3, cmvn, LABELS, LAB] + received + [flags]
    name, seen = _call("accumulate_ctc%s_raw" % stem, (X, UTT, 3, LABELS, LAB), dict(own, last=last, cmvn=cmvn, train=train),
                       want)
    assert name == ("tfk_accumulate_ctc" if train else "tfk_eval_accumulate_ctc") + stem + "_raw"
    assert len(seen) == len(_lib.SYMBOLS[name][1])
    assert seen == _seen(want)


def test_the_eval_aliases_and_the_positional_forms():
    """eval_accumulate_ctc_{mmi,wild} are the train=False calls; the criterion's arguments are also taken by position"""
    want = [HANDLE, X, 4, 7, UTT, 2, LABELS, LAB, 0.5, 0.125, 0]
    assert _call("eval_accumulate_ctc_mmi", (X, UTT, LABELS, LAB, 0.5, 0.125), {}, want) == (
        "tfk_eval_accumulate_ctc_mmi", _seen(want))
    want = [HANDLE, X, 4, 7, UTT, 2, LABELS, LAB, WILD, 0.5, 0]
    assert _call("eval_accumulate_ctc_wild", (X, UTT, LABELS, LAB, WILD, 0.5), {}, want) == (
        "tfk_eval_accumulate_ctc_wild", _seen(want))
    want = [HANDLE, X, 4, 7, UTT, 2, LABELS, LAB, COUNTS, HYP_LABELS, HYP_LENS, 0.25, 2]
    assert _call("accumulate_ctc_mwer", (X, UTT, LABELS, LAB, COUNTS, HYP_LABELS, HYP_LENS, 0.25, True), {}, want) == (
        "tfk_accumulate_ctc_mwer", _seen(want))
    # the defaults: no flags, no wildcard, penalty / ctc_weight 0, lm_scale 1
    want = [HANDLE, X, 4, 7, UTT, 2, LABELS, LAB, None, 0.0, 0]
    assert _call("accumulate_ctc_wild", (X, UTT, LABELS, LAB), {}, want)[1] == _seen(want)
    want = [HANDLE, X, 4, 7, UTT, 2, 1, None, LABELS, LAB, 1.0, 0.0, 0]
    assert _call("accumulate_ctc_mmi_raw", (X, UTT, 1, LABELS, LAB), {}, want)[1] == _seen(want)


def test_inputs_are_converted_before_they_are_handed_over():
    """lists, float64 frames, bool flags: the entry sees float32 / int32 / uint8 bytes"""
    want = [HANDLE, X, 4, 7, UTT, 2, 3, CMVN, LABELS, LAB, WILD, 0.5, 2]
    name, seen = _call("accumulate_ctc_wild_raw", (X.astype(np.float64), UTT.tolist(), 3.0, LABELS.tolist(), LAB.astype(np.int64)),
                       dict(wild=WILD.astype(bool), penalty=np.float32(0.5), last=1, cmvn=CMVN.astype(np.float64)), want)
    assert name == "tfk_accumulate_ctc_wild_raw" and seen == _seen(want)
    assert type(seen[6]) is int and type(seen[11]) is float


def test_all_16_entries_are_reached():
    reached = set()
    for stem, own, _ in CRITERIA.values():
        for train in (True, False):
            eng = _engine()
            if stem == "":
                eng.accumulate_ctc(X, UTT, LABELS, LAB) if train else eng.eval_accumulate_ctc(X, UTT, LABELS, LAB)
            else:
                getattr(eng, "accumulate_ctc" + stem)(X, UTT, LABELS, LAB, train=train, **own)
            getattr(eng, "accumulate_ctc%s_raw" % stem)(X, UTT, 1, LABELS, LAB, train=train, **own)
            reached.update(name for name, _ in eng.lib.calls)
    assert reached == {n for n in _lib.SYMBOLS if "accumulate_ctc" in n} and len(reached) == 16


# ---- the order of the refusals: _ctc_args, then the criterion's own arguments, then the cmvn table ----
BAD_UTT = np.array([3, 3], np.int32)
FRAMES_MESSAGE = "CTC micro-batch: frames (7, 4) / utterance lengths / labels do not match"
BAD_CMVN = np.zeros((2, 2, 3), np.float32)


def _refused(method, args, kw, message):
    eng = _engine()
    with pytest.raises(ValueError) as err:
        getattr(eng, method)(*args, **kw)
    assert str(err.value) == message
    assert eng.lib.calls == []


@pytest.mark.parametrize("raw", [False, True], ids=["spliced", "raw"])
def test_frames_against_lengths_comes_before_the_criterions_arguments(raw):
    tail, ctx = ("_raw", (2,)) if raw else ("", ())
    args = (X, BAD_UTT) + ctx + (LABELS, LAB)
    _refused("accumulate_ctc_wild" + tail, args, dict(wild=WILD, penalty=-1.0), FRAMES_MESSAGE)
    _refused("accumulate_ctc_mwer" + tail, args + (COUNTS, HYP_LABELS, HYP_LENS), dict(ctc_weight=float("nan")), FRAMES_MESSAGE)
    _refused("accumulate_ctc_mmi" + tail, args, dict(lm_scale=-1.0), FRAMES_MESSAGE)
    _refused("accumulate_ctc_mmi" + tail, args, dict(ctc_weight=float("inf"), train=False), FRAMES_MESSAGE)
    if raw:
        _refused("accumulate_ctc_raw", args, dict(cmvn=BAD_CMVN), FRAMES_MESSAGE)
    else:
        _refused("accumulate_ctc", args, {}, FRAMES_MESSAGE)
        _refused("eval_accumulate_ctc", args, {}, FRAMES_MESSAGE)
        _refused("eval_accumulate_ctc_wild", args + (WILD, -1.0), {}, FRAMES_MESSAGE)
        _refused("eval_accumulate_ctc_mmi", args + (-1.0,), {}, FRAMES_MESSAGE)


def test_the_criterions_arguments_come_before_the_cmvn_table():
    args = (X, UTT, 2, LABELS, LAB)
    _refused("accumulate_ctc_wild_raw", args, dict(wild=WILD, penalty=-1.0, cmvn=BAD_CMVN), "penalty -1.0 must be finite and >= 0")
    _refused("accumulate_ctc_wild_raw", args, dict(wild=WILD[:4], penalty=0.0, cmvn=BAD_CMVN),
             "CTC micro-batch: 4 gap flags for 2 sequences of 3 labels (one more than labels each: 5)")
    _refused("accumulate_ctc_mwer_raw", args + (COUNTS, HYP_LABELS, HYP_LENS), dict(ctc_weight=-0.5, cmvn=BAD_CMVN),
             "ctc_weight -0.5 must be finite and >= 0")
    _refused("accumulate_ctc_mwer_raw", args + (COUNTS[:1], HYP_LABELS, HYP_LENS), dict(cmvn=BAD_CMVN),
             "hypotheses: 1 counts (smallest 1) for 2 utterances")
    _refused("accumulate_ctc_mmi_raw", args, dict(lm_scale=float("nan"), cmvn=BAD_CMVN), "lm_scale nan must be finite and >= 0")
    _refused("accumulate_ctc_mmi_raw", args, dict(ctc_weight=float("inf"), cmvn=BAD_CMVN, train=False),
             "ctc_weight inf must be finite and >= 0")
    for method, more in (("accumulate_ctc_raw", ()), ("accumulate_ctc_wild_raw", ()), ("accumulate_ctc_mmi_raw", ()),
                         ("accumulate_ctc_mwer_raw", (COUNTS, HYP_LABELS, HYP_LENS))):
        _refused(method, args + more, dict(cmvn=BAD_CMVN), "cmvn table (2, 2, 3), expected (2, 2, 4)")


def test_the_criterions_arguments_are_refused_in_signature_order():
    args = (X, UTT, LABELS, LAB)
    _refused("accumulate_ctc_wild", args, dict(wild=WILD[:4], penalty=-1.0),
             "CTC micro-batch: 4 gap flags for 2 sequences of 3 labels (one more than labels each: 5)")
    _refused("accumulate_ctc_mwer", args + (COUNTS, HYP_LABELS, HYP_LENS[:2]), dict(ctc_weight=-1.0),
             "hypotheses: 2 label counts (sum 1) for 3 hypotheses and 3 labels")
    _refused("accumulate_ctc_mmi", args, dict(lm_scale=-2.0, ctc_weight=-1.0), "lm_scale -2.0 must be finite and >= 0")


# ---- the frame-level raw forms beside them: eval_accumulate_raw and the two stacked ones ----
Y = np.array([4, 0, 1, 3, 3, 2, 0], np.int32)
SEG = np.array([1, 1], np.int32)


def test_frame_level_raw_entries():
    want = [HANDLE, X, 4, Y, 7, UTT, 2, 3, CMVN, 0]
    assert _call("eval_accumulate_raw", (X, Y, UTT, 3), dict(cmvn=CMVN), want) == ("tfk_eval_accumulate_raw", _seen(want))
    want = [HANDLE, X, 4, Y, 7, UTT, 2, 3, None, SEG, 2, 2]
    assert _call("accumulate_stacked_raw", (X, Y, UTT, 3, [1, 1]), dict(last=True), want) == (
        "tfk_accumulate_stacked_raw", _seen(want))
    want = [HANDLE, X, 4, Y, 7, UTT, 2, 3, CMVN, SEG, 2, 0]
    assert _call("eval_accumulate_stacked_raw", (X, Y, UTT, 3, [1, 1]), dict(cmvn=CMVN), want) == (
        "tfk_eval_accumulate_stacked_raw", _seen(want))
    for name in ("tfk_eval_accumulate_raw", "tfk_accumulate_stacked_raw", "tfk_eval_accumulate_stacked_raw"):
        assert len(_lib.SYMBOLS[name][1]) == (10 if name == "tfk_eval_accumulate_raw" else 12)
    # the cmvn table is refused before the targets, as it was
    for method, more in (("accumulate_stacked_raw", ([1, 1],)), ("eval_accumulate_stacked_raw", ([1, 1],))):
        _refused(method, (X, Y[:6], UTT, 3) + more, dict(cmvn=BAD_CMVN), "cmvn table (2, 2, 3), expected (2, 2, 4)")
        _refused(method, (X, Y[:6], UTT, 3) + more, {}, "targets (6,) do not match 7 frames")


def test_eval_accumulate_raw_refuses_short_targets():
    """NEW BEHAVIOUR (the one hole the refactor closes): eval_accumulate_raw never compared len(y) with the frame count, so
    the C entry, which cannot know y's length, read a short y past its end on the host.  It now refuses as accumulate_raw and
    both stacked raw forms always did, and no call is made."""
    _refused("eval_accumulate_raw", (X, Y[:6], UTT, 3), {}, "targets (6,) do not match 7 frames")
    _refused("eval_accumulate_raw", (X, Y[:6], UTT, 3), dict(cmvn=BAD_CMVN), "cmvn table (2, 2, 3), expected (2, 2, 4)")
