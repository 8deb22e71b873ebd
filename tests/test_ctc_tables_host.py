"""The host checks of the CTC entries' small tables and the layout of a CtcBatch in one allocation (csrc/ctc_tables.h) on the
CPU, through tools/ctc_tables_check.cpp, which calls the functions the library calls and captures what tfk_last_error would
return.  Every expected message is a literal here, written out from the format strings the entries had before the checks were
shared; none is produced by the code under test.  Each case runs for at least two of the family names the messages open with.
"""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if shutil.which(c):
            return c
    return None


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ctc_tables") / "ctc_tables_check")
    subprocess.run([cc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "tfkaldi_amd", "csrc"),
                    os.path.join(ROOT, "tools", "ctc_tables_check.cpp"), "-o", exe], check=True)

    def run(commands):
        r = subprocess.run([exe], input="".join(c + "\n" for c in commands), capture_output=True, text=True, check=True)
        lines = r.stdout.split("\n")
        assert len(lines) == len(commands) + 1 and lines[-1] == ""
        return [l.split(";") for l in lines[:-1]]
    return run


def _arr(v):
    return "NULL" if v is None else " ".join(str(x) for x in v) if len(v) else "-"


def _ok(got, *outputs):
    assert got[0] == "0" and got[1] == "", got
    assert tuple(got[2:]) == tuple(str(o) for o in outputs), got


def _refused(got, message):
    assert got[0] == "-1", got
    assert got[1] == message, got


def test_utterance_bounds(tool):
    def seg(fam, whole, T, v):
        return "seg;%s;%d;%d;%s" % (fam, whole, T, _arr(v))
    for fam in ("CTC align", "CTC wild", "CTC score", "CTC spot", "CTC MWER", "CTC MMI"):
        got = tool([seg(fam, 0, 8, [0, 8]), seg(fam, 1, 8, [0, 8]),
                    seg(fam, 0, 8, [0, 8, 6]), seg(fam, 1, 8, [0, 8, 6]),
                    seg(fam, 0, 8, [1, 8]), seg(fam, 1, 8, [1, 8]),
                    seg(fam, 0, 8, [0, 9]), seg(fam, 1, 8, [0, 9]),
                    seg(fam, 0, 8, [2, 4, 4, 7]), seg(fam, 0, 8, [-1, 8])])
        _ok(got[0])
        _ok(got[1])
        _refused(got[2], "%s: utterance 1 has a negative length" % fam)
        _refused(got[3], "%s: utterance 1 has a negative length" % fam)
        _ok(got[4])  # a sub-range of the logits
        _refused(got[5], "%s: seg = [1, 8] is not [0, T = 8]" % fam)  # the form of tfk_ctc_mmi_logits
        _refused(got[6], "%s: seg = [0, 9] outside [0, T = 8]" % fam)
        _refused(got[7], "%s: seg = [0, 9] is not [0, T = 8]" % fam)
        _ok(got[8])  # an empty utterance in the middle
        _refused(got[9], "%s: seg = [-1, 8] outside [0, T = 8]" % fam)


def test_label_offsets(tool):
    def off(fam, noun, limit, v, unit="utterance"):
        return "off;%s;%s;%s;%d;%s" % (fam, unit, noun, limit, _arr(v))
    for fam in ("CTC align", "CTC wild", "CTC MMI"):
        got = tool([off(fam, "", 511, [0, 2, 1]), off(fam, " reference", 511, [0, 2, 1]), off(fam, "", 511, [-1, 1]),
                    off(fam, "", 511, [0, 512]), off(fam, "", 511, [0, 511]), off(fam, "", -1, [0, 512]),
                    off(fam, "", 511, [3, 3, 5, 5]), off(fam, "", 511, [0, 1, 0], unit="pair")])
        _refused(got[0], "%s: utterance 1 has a negative length" % fam)
        _refused(got[1], "%s: utterance 1 has a negative reference length" % fam)  # (MWER's and MMI's references)
        _refused(got[2], "%s: lab_off[0] = -1 < 0" % fam)
        _refused(got[3], "%s: 512 labels in one utterance (limit 511)" % fam)
        assert "511" in got[3][1]
        _ok(got[4], 511)
        _ok(got[5], 512)  # no limit here: the entry's own limits function refuses it (ctc_align_limits, ctc_score_limits)
        _ok(got[6], 2)
        _refused(got[7], "%s: pair 1 has a negative length" % fam)


def test_pair_tables(tool):
    def pairs(fam, U, ordered, utt, off):
        return "pairs;%s;%d;%d;%s;%s" % (fam, U, ordered, _arr(utt), _arr(off))
    for fam in ("CTC score", "CTC spot", "CTC MWER"):
        got = tool([pairs(fam, 2, 0, [0, 2], [0, 1, 2]), pairs(fam, 2, 0, [1, 0], [0, 1, 2]), pairs(fam, 2, 1, [1, 0], [0, 1, 2]),
                    pairs(fam, 2, 0, [], [0]), pairs(fam, 2, 1, [], [0]), pairs(fam, 2, 1, [0, 0, 1], [4, 4, 9, 10]),
                    pairs(fam, 2, 0, [0, -1], [0, 1, 2]), pairs(fam, 2, 0, [0, 1], [0, 3, 2]), pairs(fam, 2, 0, [0, 1], [-2, 0, 1])])
        _refused(got[0], "%s: pair 1 names utterance 2 outside [0, 2)" % fam)
        _ok(got[1], 1)
        _refused(got[2], "%s: pair 1: the pairs are not ordered by utterance" % fam)  # (what MWER requires)
        _ok(got[3], 0)
        _ok(got[4], 0)
        _ok(got[5], 5)
        _refused(got[6], "%s: pair 1 names utterance -1 outside [0, 2)" % fam)
        _refused(got[7], "%s: pair 1 has a negative length" % fam)
        _refused(got[8], "%s: lab_off[0] = -2 < 0" % fam)


def test_transcripts(tool):
    O, T = 4, 8  # labels in [0, 3): 3 is the blank

    def trans(fam, utt, lens, labels, wild=None, T=-1, limit=511):
        return "trans;%s;%d;%d;%d;%s;%s;%s;%s" % (fam, O, limit, T, _arr(utt), _arr(lens), _arr(labels), _arr(wild))
    for fam in ("CTC align", "CTC wild"):
        got = tool([trans(fam, [4, 4], [1, 2], [0, 1, 2]),
                    trans(fam, [4, 4], [1, 2], [0, 1, O - 1]),
                    trans(fam, [4, 4], [1, 2], [-1, 1, 2]),
                    trans(fam, [4, 4], [1, 2], [0, 1, 2], wild=[0, 1, 0, 2, 0]),
                    trans(fam, [4, 4], [1, 2], [0, 1, 2], wild=[0, 1, 1, 0, 1]),
                    trans(fam, [4, 3], [1, 2], [0, 1, 2], T=T),
                    trans(fam, [4, 3], [1, 2], [0, 1, 2]),
                    trans(fam, [4, 4], [1, 2], [0, 1, 2], T=T),
                    trans(fam, [4, 4], [1, 2], None),
                    trans(fam, [4, 4], [0, 0], None, T=T),
                    trans(fam, [4, -1], [1, 2], [0, 1, 2]),
                    trans(fam, [4, 4], [-1, 2], [0, 1, 2]),
                    trans(fam, [4, 600], [1, 512], ["513*0"]),
                    trans(fam, [4, 600], [1, 511], ["512*0"])])
        _ok(got[0], 3)
        _refused(got[1], "%s: utterance 1: label 3 outside [0, 3)" % fam)
        _refused(got[2], "%s: utterance 0: label -1 outside [0, 3)" % fam)
        _refused(got[3], "%s: utterance 1, gap 1: wild is 2, not 0 or 1" % fam)
        _ok(got[4], 3)
        _refused(got[5], "%s: utterance lengths sum to 7, expected T = 8" % fam)
        _ok(got[6], 3)  # (the sum is only checked where it is asked for)
        _ok(got[7], 3)
        _refused(got[8], "%s: labels is NULL" % fam)
        _ok(got[9], 0)
        _refused(got[10], "%s: utterance 1 has a negative length" % fam)
        _refused(got[11], "%s: utterance 0 has a negative length" % fam)
        _refused(got[12], "%s: utterance 1 has 512 labels (limit 511)" % fam)
        _ok(got[13], 512)


def test_pair_builder(tool):
    O = 4

    def count(fam, noun, counts, utt, most=1 << 20):
        return "count;%s;%s;%d;%s;%s" % (fam, noun, most, _arr(counts), _arr(utt))

    def build(fam, noun, name_pair, counts, lens, labels, wild=None):
        return "build;%s;%s;%d;%d;511;%s;%s;%s;%s" % (fam, noun, name_pair, O, _arr(counts), _arr(lens), _arr(labels), _arr(wild))
    # (family, noun, whether the pair is named, how a message names utterance 1's second sequence, which is pair 2)
    for fam, noun, name_pair, who in (("CTC score", "hypothesis", 0, "utterance 1, hypothesis 1"),
                                      ("CTC MWER", "hypothesis", 0, "utterance 1, hypothesis 1"),
                                      ("CTC spot", "pattern", 1, "utterance 1, pattern 1 (pair 2)")):
        got = tool([count(fam, noun, [2, 0, 1], [3, 3, 3]), count(fam, noun, [2, -1, 1], [3, 3, 3]),
                    count(fam, noun, [2, 0, 1], [3, 3, -3]), count(fam, noun, [1 << 20, 1], [3, 3]), count(fam, noun, [0, 0], [3, 3]),
                    build(fam, noun, name_pair, [2, 0, 1], [1, 2, 1], [0, 1, 2, 0]),
                    build(fam, noun, name_pair, [1, 2], [1, 1, 512], ["514*0"]),
                    build(fam, noun, name_pair, [1, 2], [1, 1, -1], [0, 0]),
                    build(fam, noun, name_pair, [1, 2], [1, 1, 2], [0, 0, 1, O - 1]),
                    build(fam, noun, name_pair, [1, 2], [1, 1, 2], None),
                    build(fam, noun, name_pair, [1, 2], [0, 0, 0], None),
                    build(fam, noun, name_pair, [1, 2], [1, 1, 2], [0, 0, 1, 2], wild=[0, 0, 0, 0, 0, 1, 2])])
        _ok(got[0], 3)
        _refused(got[1], "%s: utterance 1 has a negative %s count" % (fam, noun))
        _refused(got[2], "%s: utterance 2 has a negative length" % fam)
        _refused(got[3], "%s: more than 1048576 (utterance, %s) pairs in one call" % (fam, noun))
        _ok(got[4], 0)
        _ok(got[5], 2, 4, "0 0 2", "0 1 3 4")  # longest, labels, pair_utt, the running offsets
        _refused(got[6][:2], "%s: %s has 512 labels (limit 511)" % (fam, who))
        _refused(got[7][:2], "%s: %s has a negative length" % (fam, who))
        _refused(got[8][:2], "%s: %s: label 3 outside [0, 3)" % (fam, who))
        _refused(got[9][:2], "%s: labels is NULL" % fam)
        _ok(got[10], 0, 0, "0 1 1", "0 0 0 0")
        _refused(got[11][:2], "%s: %s, gap 2: wild is 2, not 0 or 1" % (fam, who))


def test_batch_layout(tool):
    """ctc_batch_layout against the byte counts tfk_ctc_wild_loss_logits and tfk_ctc_mmi_logits computed by hand before it was
    shared: [off T, offb T, logz U doubles | post T ld, lp / ab / bb T sext, lse T floats], and for MMI with G(y) (U doubles) in
    front, g (T ld) behind post and the CTC losses (U) and logw (here 7 floats) behind lse"""
    names = ("lead", "off", "offb", "logz", "post", "mid", "lp", "ab", "bb", "lse", "tail")
    shapes = list(itertools.product((1, 3), (1, 2), (2, 5), (64, 128), (False, True)))
    nlogw = 7
    extra = lambda T, U, ld, mmi: (U, T * ld, U + nlogw) if mmi else (0, 0, 0)  # noqa: E731
    got = tool(["layout;%d;%d;%d;%d;%d;%d;%d" % ((T, U, ld, sext) + extra(T, U, ld, mmi)) for T, U, ld, sext, mmi in shapes])
    for (T, U, ld, sext, mmi), line in zip(shapes, got):
        v = [int(x) for x in line[0].split()]
        at, total = dict(zip(names, v)), v[-1]
        lead, mid, tail = extra(T, U, ld, mmi)
        size = dict(lead=8 * lead, off=8 * T, offb=8 * T, logz=8 * U, post=4 * T * ld, mid=4 * mid, lp=4 * T * sext, ab=4 * T * sext,
                    bb=4 * T * sext, lse=4 * T, tail=4 * tail)
        what = (T, U, ld, sext, mmi, at, total)
        for n in names:
            assert at[n] % (8 if n in ("lead", "off", "offb", "logz") else 4) == 0, what  # aligned to its element
            assert at[n] + size[n] <= total, what  # inside the allocation
        for a, b in itertools.combinations(names, 2):  # pairwise disjoint
            assert at[a] + size[a] <= at[b] or at[b] + size[b] <= at[a], (a, b, what)
        if mmi:
            dbl = (2 * U + 2 * T) * 8
            flt = (2 * T * ld + 3 * T * sext + T + U + nlogw) * 4
            assert total == dbl + flt, what
            assert at["lead"] == 0 and at["off"] == 8 * U, what  # G(y) first
        else:
            assert total == (2 * T + U) * 8 + (T * ld + 3 * T * sext + T) * 4, what
            assert at["off"] == 0, what
        # the order of the regions: doubles first, then the float regions
        assert [at[n] for n in names] == sorted(at[n] for n in names), what
