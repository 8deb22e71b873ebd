"""CTC alignment with wildcard gaps and keyword spotting on the device (tfk_ctc_align_wild / tfk_ctc_spot and their _raw and
_logits forms, csrc/ctc.hip) against the numpy restatement of tests/test_ctc_align_wild_host.py applied to the SAME logits.

Paths, start and end: on integer logits every fp32 intermediate of the recursion is exact, so they must EQUAL the
restatement's, ties included.  Scores and free: within `tol` = 4 x the largest |float32 run - float64 run| of the restatement
over the same cases, floored at 1e-6 x |score| (the rule of test_gpu_ctc_score.py).  Every test prints a line "ctc_wild_edges:"
with the largest |device - float64| beside that bound; profiles/ctc_wild_edges.txt is the table of those lines."""
from ctypes import c_void_p

import numpy as np
import pytest

from test_ctc_align_host import check_valid, integer_logits, row_lse
from test_ctc_align_wild_host import span, wild_align, wild_path_score, wild_spot
from test_ctc_decode_host import best_path
from test_gpu_ctc_align import SENTINEL, _engine_case, _labels, _min_frames
from test_gpu_ctc_beam import KW, _sharpen
from test_gpu_ctc_decode import E2E_STEPS, _refs, _split, _toy_ctc
from util import make_pair

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tables(z, utt, seqs, flags, lead, tail):
    """device copies of the logits (the utterances start at row `lead`, junk around them), seg, labels, lab_off and the
    flags (None: a NULL pointer; else one array per sequence, laid out at lab_off[i] + i)"""
    z = np.ascontiguousarray(z, dtype=np.float32)
    full = np.full((lead + z.shape[0] + tail, z.shape[1]), 50.0, np.float32)  # (what surrounds the utterances must not matter)
    full[lead:lead + z.shape[0]] = z
    seg = (lead + np.concatenate([[0], np.cumsum(utt)])).astype(np.int32)
    lab_off = np.concatenate([[0], np.cumsum([len(r) for r in seqs])]).astype(np.int32)
    labels = np.concatenate([np.asarray(r, np.int32) for r in seqs] + [np.zeros(1, np.int32)])
    wild = None if flags is None else _dev(np.concatenate([np.asarray(f).astype(np.uint8) for f in flags] + [np.zeros(1, np.uint8)]))
    return full, _dev(full), seg, _dev(seg), _dev(labels), _dev(lab_off), wild


def _p(t):
    return c_void_p(None if t is None else t.data_ptr())


def _device_align(z, utt, refs, flags, lead=3, tail=5, plain=False):
    """tfk_ctc_align_wild_logits (plain: tfk_ctc_align_logits) on host logits: (the utterances' slices of ali, score [U], free
    [U] or None); the rows outside every utterance must keep their sentinel"""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    full, d_z, seg, d_seg, d_lab, d_off, d_wild = _tables(z, utt, refs, flags, lead, tail)
    T, O, U = full.shape[0], full.shape[1], len(utt)
    ali = torch.full((T,), SENTINEL, dtype=torch.int32, device="cuda")
    score = torch.full((U,), 12345.0, dtype=torch.float32, device="cuda")
    free = torch.full((U,), 12345.0, dtype=torch.float32, device="cuda")
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    if plain:
        _lib.check(lib.tfk_ctc_align_logits(stream, _p(d_z), O, O, T, _p(d_seg), U, _p(d_lab), _p(d_off), _p(ali), _p(score)))
    else:
        _lib.check(lib.tfk_ctc_align_wild_logits(stream, _p(d_z), O, O, T, _p(d_seg), U, _p(d_lab), _p(d_off), _p(d_wild),
                                                 _p(ali), _p(score), _p(free)))
    torch.cuda.synchronize()
    ali, score = ali.cpu().numpy(), score.cpu().numpy()
    assert np.all(ali[:lead] == SENTINEL) and np.all(ali[seg[-1]:] == SENTINEL)
    return [ali[seg[u]:seg[u + 1]].copy() for u in range(U)], score, None if plain else free.cpu().numpy()


def _device_spot(z, utt, pair_utt, pats, flags, lead=3, tail=5):
    """tfk_ctc_spot_logits on host logits: (score [P], start [P], end [P], free [U])"""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    full, d_z, seg, d_seg, d_lab, d_off, d_wild = _tables(z, utt, pats, flags, lead, tail)
    T, O, U, P = full.shape[0], full.shape[1], len(utt), len(pats)
    d_utt = _dev(np.asarray(list(pair_utt) + [0], np.int32))
    score = torch.full((P + 1,), 12345.0, dtype=torch.float32, device="cuda")
    start = torch.full((P + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    end = torch.full((P + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    free = torch.full((U,), 12345.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.tfk_ctc_spot_logits(c_void_p(torch.cuda.current_stream().cuda_stream), _p(d_z), O, O, T, _p(d_seg), U,
                                       _p(d_utt), P, _p(d_lab), _p(d_off), _p(d_wild), _p(score), _p(start), _p(end), _p(free)))
    torch.cuda.synchronize()
    score, start, end = score.cpu().numpy(), start.cpu().numpy(), end.cpu().numpy()
    assert score[P] == 12345.0 and start[P] == SENTINEL and end[P] == SENTINEL  # nothing is written past the pairs
    return score[:P], start[:P], end[:P], free.cpu().numpy()


def _flags(rng, mode, seqs):
    """one flag array per sequence: "none", "ends", "all" or "random" """
    out = []
    for s in seqs:
        f = np.ones(len(s) + 1, np.uint8) if mode in ("ends", "all") else np.zeros(len(s) + 1, np.uint8)
        if mode == "ends":
            f[1:-1] = 0
        if mode == "random":
            f = rng.integers(0, 2, size=len(s) + 1).astype(np.uint8)
        out.append(f)
    return out


def _restatement(zs, refs, flags):
    """per utterance the float64 (ali, score, free) of the restatement, and tol for score and free from its float32 run"""
    r64 = [wild_align(z, r, f) for z, r, f in zip(zs, refs, flags)]
    r32 = [wild_align(z, r, f, np.float32) for z, r, f in zip(zs, refs, flags)]
    s64, f64 = np.array([r[1] for r in r64]), np.array([r[2] for r in r64])
    s32, f32 = np.array([r[1] for r in r32]), np.array([r[2] for r in r32])
    finite = np.isfinite(s64)
    assert np.array_equal(finite, np.isfinite(s32))
    diff = max(np.abs(s32[finite] - s64[finite]).max() if finite.any() else 0.0, np.abs(f32 - f64).max())
    return [r[0] for r in r64], s64, f64, np.maximum(4.0 * diff, 1e-6 * np.abs(np.where(finite, s64, f64)))


def _check_exact(name, z, utt, refs, flags):
    """integer logits: the device's alignment EQUALS the restatement's for every utterance; score and free within tol"""
    zs = np.split(z, np.cumsum(utt)[:-1])
    alis, scores, free = _device_align(z, utt, refs, flags)
    want, s64, f64, tol = _restatement(zs, refs, flags)
    worst = worst_free = 0.0
    for u in range(len(utt)):
        worst_free = max(worst_free, abs(float(free[u]) - f64[u]))
        assert abs(float(free[u]) - f64[u]) <= tol[u], (name, u, free[u], f64[u], tol[u])
        if want[u] is None:
            assert scores[u] == -np.inf and np.all(alis[u] == -2), (name, u, utt[u], len(refs[u]))
            continue
        assert np.array_equal(alis[u], want[u]), (name, u, utt[u], len(refs[u]), np.nonzero(alis[u] != want[u])[0][:8])
        exact = wild_path_score(zs[u], refs[u], flags[u], alis[u]) if utt[u] else 0.0
        worst = max(worst, abs(float(scores[u]) - exact))
        assert abs(float(scores[u]) - exact) <= tol[u], (name, u, scores[u], exact, tol[u])
        assert float(scores[u]) <= float(free[u]) + tol[u]
    print("ctc_wild_edges: %-28s %3d utterances  |score - float64| %.3e  |free - float64| %.3e  bound %.3e ... %.3e"
          % (name, len(utt), worst, worst_free, tol.min(), tol.max()))
    return alis, scores, free


def _frame_case(seed=800):
    """every frame count 0 ... 20 and the edges of the 64-frame back-trace block, random labels (the smallest register tile)"""
    rng = np.random.default_rng(seed)
    utt = list(range(21)) + [63, 64, 65, 129]
    refs = [_labels(rng, int(rng.integers(1, min(Tn // 2, 40) + 1))) if Tn >= 2 else np.zeros(0, np.int32) for Tn in utt]
    refs[5], refs[12] = np.zeros(0, np.int32), np.array([2, 2, 2, 2], np.int32)  # an empty reference, a run of one label
    refs[2] = np.array([1, 1], np.int32)  # one frame short: a a needs three
    assert max(len(r) for r in refs) <= 63
    return integer_logits(rng, sum(utt), 9), utt, refs


def _tile_case(S):
    """the longest reference at a register tile's edge: the fewest frames that fit and 37 more, twice (for two flag modes), and
    one utterance a frame short"""
    rng = np.random.default_rng(S)
    rep = _labels(rng, S, repeats=S // 5)
    need = _min_frames(rep)
    utt = [need, need + 37, need, need + 37, need - 1]
    return integer_logits(rng, sum(utt), 9), utt, [rep] * 5


@pytest.mark.parametrize("mode", ["none", "ends", "all", "random"])
def test_exact_paths_on_integer_logits_every_frame_count(gpu, mode):
    z, utt, refs = _frame_case()
    alis, scores, _ = _check_exact("frames, flags " + mode, z, utt, refs, _flags(np.random.default_rng(801), mode, refs))
    assert scores[0] == 0.0 and alis[0].size == 0 and scores[2] == -np.inf and np.all(alis[2] == -2)


@pytest.mark.parametrize("S", [63, 64, 127, 128, 255, 256, 511])
def test_exact_paths_on_integer_logits_every_register_tile(gpu, S):
    z, utt, refs = _tile_case(S)
    rng = np.random.default_rng(810 + S)
    flags = _flags(rng, "ends", refs[:2]) + _flags(rng, "random", refs[2:4]) + _flags(rng, "ends", refs[4:])
    alis, scores, _ = _check_exact("S=%d" % S, z, utt, refs, flags)
    assert scores[4] == -np.inf and np.all(alis[4] == -2) and np.all(np.isfinite(scores[:4]))


def test_no_flags_equal_the_plain_alignment_bit_for_bit(gpu):
    """wild == NULL and all flags zero: ali and the bytes of score are tfk_ctc_align_logits' on the cases of the two tests above"""
    for z, utt, refs in [_frame_case()] + [_tile_case(S) for S in (63, 64, 127, 128, 255, 256, 511)]:
        plain = _device_align(z, utt, refs, None, plain=True)
        for flags in (None, _flags(None, "none", refs)):
            got = _device_align(z, utt, refs, flags)
            assert got[1].tobytes() == plain[1].tobytes()
            assert all(np.array_equal(a, b) for a, b in zip(got[0], plain[0]))


def _spot_against_align(name, z, utt, pats, flags, pair_utt=None):
    """tfk_ctc_spot_logits on the pairs (utterance, pattern) -- all of them unless pair_utt / pats name the pairs -- against
    tfk_ctc_align_wild_logits of every pair's pattern on its utterance: the bytes of score, start and end read off ali; and
    against the restatement's forward sweep"""
    U = len(utt)
    if pair_utt is None:
        pair_utt = np.repeat(np.arange(U), len(pats))
        pats, flags = pats * U, flags * U
    zs = np.split(z, np.cumsum(utt)[:-1])
    score, start, end, free = _device_spot(z, utt, pair_utt, pats, flags)
    # the same pairs as an alignment batch: one "utterance" per pair, its frames repeated
    za = np.concatenate([zs[u] for u in pair_utt] + [np.zeros((0, z.shape[1]), np.float32)])
    alis, ascore, afree = _device_align(za, [utt[u] for u in pair_utt], pats, flags)
    assert score.tobytes() == ascore.tobytes(), (name, np.nonzero(score != ascore)[0][:8])
    for p, u in enumerate(pair_utt):
        want = (-1, -1) if ascore[p] == -np.inf else span(alis[p])
        assert (int(start[p]), int(end[p])) == want, (name, p, u, len(pats[p]), start[p], end[p], want)
        assert (int(start[p]), int(end[p])) == wild_spot(zs[u], pats[p], flags[p])[1:], (name, p)
        assert afree[p].tobytes() == free[u].tobytes()
    f64 = np.array([wild_align(a, [], None)[2] for a in zs])
    f32 = np.array([wild_align(a, [], None, np.float32)[2] for a in zs])
    tol = np.maximum(4.0 * np.abs(f32 - f64).max(), 1e-6 * np.abs(f64))
    assert np.all(np.abs(free - f64) <= tol), (name, free, f64, tol)
    print("ctc_wild_edges: %-28s %3d pairs       score, start, end equal the alignment's   |free - float64| %.3e  bound %.3e"
          % (name, len(pair_utt), np.abs(free - f64).max(), tol.max()))
    return score, start, end, free


def test_spot_equals_align_for_every_pair(gpu):
    rng = np.random.default_rng(820)
    utt = [0, 1, 17, 64, 130]
    z = integer_logits(rng, sum(utt), 9)
    pats = [np.zeros(0, np.int32), np.array([3], np.int32), np.array([1, 1], np.int32), _labels(rng, 3), _labels(rng, 7),
            _labels(rng, 12, repeats=3), _labels(rng, 12)]
    for mode in ("ends", "random", "none"):
        flags = _flags(rng, mode, pats)
        score, start, end, _ = _spot_against_align("spot 5 x 7, flags " + mode, z, utt, pats, flags)
        score, start, end = score.reshape(5, 7), start.reshape(5, 7), end.reshape(5, 7)
        assert score[0, 0] == 0.0 and np.all(score[0, 1:] == -np.inf) and np.all(start[0, 1:] == -1)  # no frames
        assert score[1, 5] == -np.inf and (start[1, 5], end[1, 5]) == (-1, -1)  # 12 labels in one frame
        assert np.all(start[:, 0] == 0) and np.all(end[:, 0] == 0)  # the empty pattern
    # an utterance without a pair between others
    flags = _flags(rng, "ends", pats)
    _spot_against_align("spot, an utterance skipped", z, utt, [pats[4], pats[6], pats[3]], [flags[4], flags[6], flags[3]],
                        pair_utt=np.array([2, 2, 4]))
    # P == 0 writes free only
    score, start, end, free = _device_spot(z, utt, [], [], None)
    assert score.size == 0 and free[0] == 0.0 and np.all(np.isfinite(free)) and np.all(free[1:] < 0)
    assert free.tobytes() == _device_align(z, utt, [np.zeros(0, np.int32)] * 5, None)[2].tobytes()


@pytest.mark.parametrize("S", [64, 200, 511])
def test_spot_equals_align_at_the_other_register_tiles(gpu, S):
    """the longest pattern selects the tile of the whole launch: short patterns run in it beside the long one"""
    rng = np.random.default_rng(830 + S)
    long = _labels(rng, S, repeats=S // 7)
    utt = [_min_frames(long) + 29, _min_frames(long) - 1, 40]
    pats = [long, _labels(rng, 5), np.zeros(0, np.int32)]
    for mode in ("ends", "random"):
        score, _, _, _ = _spot_against_align("spot S=%d, flags %s" % (S, mode), integer_logits(rng, sum(utt), 9), utt, pats,
                                             _flags(rng, mode, pats))
        assert np.isfinite(score[0]) and score[3] == -np.inf and score[6] == -np.inf


@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
@pytest.mark.parametrize("O", [9, 36])
def test_engine_entries_on_the_engines_logits(gpu, dtype, O):
    """valid paths whose float64 score is the returned score, score <= free, score >= tfk_ctc_align's, free = the
    log-probability of the per-frame best path; tfk_ctc_spot gives every pair what tfk_ctc_align_wild gives it"""
    eng, utt, X, labels, lab = _engine_case(dtype, O, 840 + O)
    rng = np.random.default_rng(841 + O)
    zs = np.split(eng.posteriors(X, raw_logits=True), np.cumsum(utt)[:-1])
    refs = _split(labels, lab)
    plain = eng.ctc_align(X, utt, labels, lab)
    # free is the log-probability of tfk_ctc_greedy's frame path: that entry takes every frame's largest logit (the path whose
    # log-probability is sum_t (max_c z[t, c] - lse[t]), which `best` below evaluates in float64) and returns it collapsed
    greedy = eng.ctc_greedy(X, utt)[0]
    assert all(np.array_equal(g, w) for g, w in zip(greedy, best_path(np.concatenate(zs), utt)))
    worst = worst_free = bound = 0.0
    for mode in ("ends", "random"):
        flags = _flags(rng, mode, refs)
        alis, scores, free = eng.ctc_align_wild(X, utt, labels, lab, np.concatenate(flags))
        assert scores.dtype == free.dtype == np.float32 and scores.shape == free.shape == (len(utt),)
        _, s64, f64, tol = _restatement(zs, refs, flags)
        feasible = 0
        for u in range(len(utt)):
            best = float((zs[u].astype(np.float64).max(axis=1) - row_lse(zs[u].astype(np.float64))).sum())
            assert abs(float(free[u]) - best) <= tol[u], (u, free[u], best, tol[u])
            worst_free, bound = max(worst_free, abs(float(free[u]) - best)), max(bound, tol[u])
            if not np.isfinite(s64[u]):
                assert alis[u] is None and scores[u] == -np.inf, (u, utt[u], lab[u])
                continue
            feasible += 1
            assert alis[u].shape == (utt[u],)
            check_valid(alis[u], refs[u], O)
            mine = wild_path_score(zs[u], refs[u], flags[u], alis[u]) if utt[u] else 0.0
            worst = max(worst, abs(float(scores[u]) - mine))
            assert abs(float(scores[u]) - mine) <= tol[u], (u, scores[u], mine, tol[u])
            assert mine >= s64[u] - tol[u], (u, mine, s64[u], tol[u])
            assert float(scores[u]) <= float(free[u]) + tol[u] and float(scores[u]) >= float(plain[1][u]) - tol[u]
        assert feasible >= 4
    none = eng.ctc_align_wild(X, utt, labels, lab)  # no flags: tfk_ctc_align's result
    assert none[1].tobytes() == plain[1].tobytes()
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(none[0], plain[0]))
    # spotting: up to two patterns per utterance (the head and the tail of its reference), none for two of them
    pats = [[r[:3], r[-2:]] if i % 3 != 1 else [] for i, r in enumerate(refs)]
    flat = [p for ps in pats for p in ps]
    pflags = _flags(rng, "ends", flat)
    got = eng.ctc_spot(X, utt, [len(ps) for ps in pats], np.concatenate(flat), [p.size for p in flat], np.concatenate(pflags))
    assert got[3].tobytes() == free.tobytes() and [g.size for g in got[0]] == [len(ps) for ps in pats]
    for k in range(2):
        targets = [ps[k] if ps else np.zeros(0, np.int32) for ps in pats]
        wild = np.concatenate([np.ones(t.size + 1, np.uint8) if t.size < 2 else np.array([1] + [0] * (t.size - 1) + [1], np.uint8)
                               for t in targets])
        alis, scores, _ = eng.ctc_align_wild(X, utt, np.concatenate(targets), [t.size for t in targets], wild)
        for u, ps in enumerate(pats):
            if ps:
                assert got[0][u][k].tobytes() == scores[u].tobytes(), (u, k)
                assert (int(got[1][u][k]), int(got[2][u][k])) == span(alis[u]), (u, k)
    print("ctc_wild_edges: %-28s %3d utterances  |score - float64| %.3e  |free - float64| %.3e  bound <= %.3e"
          % ("engine %s O=%d" % (dtype, O), len(utt), worst, worst_free, bound))
    eng.close()


def test_raw_entries_equal_host_spliced_bit_for_bit(gpu):
    import torch
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(850)
    D, C = 4, 2
    eng, _ = make_pair(rng, max_frames=256, **dict(KW, input_dim=D * (2 * C + 1), output_dim=12))
    _sharpen(eng, rng, 4.0, 2.0)
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 5, 63, 17)]
    lens = [u.shape[0] for u in utts]
    labels, lab = _refs(np.random.default_rng(851), len(utts), 12, 0, 15)
    wild = np.concatenate(_flags(rng, "random", _split(labels, lab)))
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)
    spliced = np.concatenate([u.spliced() for u in utts])

    def same(a, b):
        return all(all((p is None and q is None) or np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x, y))
                   if isinstance(x, list) else x.tobytes() == y.tobytes() for x, y in zip(a, b))

    host = eng.ctc_align_wild(spliced, lens, labels, lab, wild)
    assert same(host, eng.ctc_align_wild_raw(raw, lens, C, labels, lab, wild, cmvn=cmvn_table(utts)))
    assert same(host, eng.ctc_align_wild_raw(torch.from_numpy(raw).cuda(), lens, C, labels, lab, wild, cmvn=cmvn_table(utts)))
    assert sum(a is not None for a in host[0]) >= 3 and any(a is not None and np.any(a >= 0) for a in host[0])
    counts = [1] * len(utts)  # spotting: every utterance's own reference as its pattern
    host = eng.ctc_spot(spliced, lens, counts, labels, lab, wild)
    assert same(host, eng.ctc_spot_raw(raw, lens, C, counts, labels, lab, wild, cmvn=cmvn_table(utts)))
    assert same(host, eng.ctc_spot_raw(torch.from_numpy(raw).cuda(), lens, C, counts, labels, lab, wild, cmvn=cmvn_table(utts)))
    assert sum(np.isfinite(s[0]) for s in host[0]) >= 3
    eng.close()


def test_limits_are_reported_and_leave_the_engine_usable(gpu):
    rng = np.random.default_rng(860)
    eng, _ = make_pair(rng, max_frames=1024, **KW)
    O = KW["output_dim"]
    utt = np.array([600, 15], np.int32)
    X = rng.standard_normal((615, KW["input_dim"])).astype(np.float32)
    labels, lab = _refs(rng, 2, O, 3, 6)
    flags = np.concatenate(_flags(rng, "ends", _split(labels, lab)))
    good = eng.ctc_align_wild(X, utt, labels, lab, flags)
    good_spot = eng.ctc_spot(X, utt, [1, 1], labels, lab, flags)
    ptr = lambda a, on=True: np.ascontiguousarray(a).ctypes.data_as(c_void_p) if on else c_void_p(None)
    keep = []  # (the arrays a call reads must outlive it)

    def arr(a, dtype):
        keep.append(np.ascontiguousarray(a, dtype))
        return keep[-1]

    def align(lab_vals=labels, lab_lens=lab, lens=utt, wild=flags, ali=True, score=True, free=True):
        out = np.empty(615, np.int32), np.empty(2, np.float32), np.empty(2, np.float32)
        return eng.lib.tfk_ctc_align_wild(eng._h, ptr(X), X.shape[1], 615, ptr(arr(lens, np.int32)), 2, ptr(arr(lab_vals, np.int32)),
                                          ptr(arr(lab_lens, np.int32)), ptr(arr(wild, np.uint8)), ptr(out[0], ali),
                                          ptr(out[1], score), ptr(out[2], free), 0)

    def spot(counts=(1, 1), lab_vals=labels, lab_lens=lab, lens=utt, wild=flags, score=True, start=True, free=True):
        out = np.empty(2, np.float32), np.empty(2, np.int32), np.empty(2, np.int32), np.empty(2, np.float32)
        return eng.lib.tfk_ctc_spot(eng._h, ptr(X), X.shape[1], 615, ptr(arr(lens, np.int32)), 2, ptr(arr(counts, np.int32)),
                                    ptr(arr(lab_vals, np.int32)), ptr(arr(lab_lens, np.int32)), ptr(arr(wild, np.uint8)),
                                    ptr(out[0], score), ptr(out[1], start), ptr(out[2]), ptr(out[3], free), 0)

    big = rng.integers(0, O - 1, size=512).astype(np.int32)
    long_labels, long_lens = np.concatenate([big, labels[lab[0]:]]), [512, lab[1]]
    long_flags = np.zeros(512 + lab[1] + 2, np.uint8)
    blank = np.where(np.arange(labels.size) == lab[0], O - 1, labels)
    two = flags.copy()
    two[lab[0] + 1 + 2] = 2  # utterance 1 / pair 1, gap 2
    cases = [
        ("512 labels", dict(lab_vals=long_labels, lab_lens=long_lens, wild=long_flags), b"511", b"511"),
        ("a label equal to the blank", dict(lab_vals=blank), b"utterance 1", b"pair 1"),
        ("a wild value of 2", dict(wild=two), b"utterance 1, gap 2", b"(pair 1), gap 2"),
        ("a negative label count", dict(lab_lens=[-1, lab[1]]), b"negative", b"negative"),
        ("a negative frame count", dict(lens=[616, -1]), b"negative", b"negative"),
        ("NULL score", dict(score=False), b"NULL", b"NULL"),
        ("NULL free", dict(free=False), b"NULL", b"NULL"),
    ]
    for name, kw, word, spot_word in cases:
        for fn, w in ((align, word), (spot, spot_word)):
            assert fn(**kw) != 0, name
            assert w in eng.lib.tfk_last_error(), (name, eng.lib.tfk_last_error())
            again = eng.ctc_align_wild(X, utt, labels, lab, flags)  # the next valid call succeeds, with the same result
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again[1:], good[1:])), name
            assert all(np.array_equal(a, b) for a, b in zip(again[0], good[0])), name
    for name, fn, kw, word in (("NULL ali", align, dict(ali=False), b"NULL"), ("NULL start", spot, dict(start=False), b"NULL"),
                               ("more than 2^20 pairs", spot, dict(counts=(1 << 20, 1)), b"1048576"),
                               ("a negative pattern count", spot, dict(counts=(1, -1)), b"utterance 1")):
        assert fn(**kw) != 0, name
        assert word in eng.lib.tfk_last_error(), (name, eng.lib.tfk_last_error())
        again = eng.ctc_spot(X, utt, [1, 1], labels, lab, flags)
        assert all(np.concatenate(a).tobytes() == np.concatenate(b).tobytes() for a, b in zip(again[:3], good_spot[:3])), name
        assert again[3].tobytes() == good_spot[3].tobytes()
    assert align() == 0 and spot() == 0
    for bad in (flags[:-1], flags.astype(np.int32)):  # the Python layer: one flag too few, another dtype
        with pytest.raises(ValueError):
            eng.ctc_align_wild(X, utt, labels, lab, bad)
        with pytest.raises(ValueError):
            eng.ctc_spot(X, utt, [1, 1], labels, lab, bad)
    eng.close()


def test_planted_keyword_end_to_end(gpu, tmp_path):
    """Decoder.ctc_spot on a trained toy CTC model: a stretch of every utterance's transcript, searched in that utterance,
    costs less against the free path than the same stretch with every label shifted, and is found where the forced
    alignment of the whole transcript puts it"""
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    for _ in range(E2E_STEPS):
        tr.update(xs, ys)
    tr.save_model(str(tmp_path / "model"))
    tr.close()
    dec = Decoder(dnn, F, maxlen)
    dec.restore(str(tmp_path / "model"))
    targets = [np.asarray(y).astype(np.int32) for y in ys]
    full, _ = dec.ctc_align(xs, targets)
    L, n = coder.num_labels, 4
    keys = [t[t.size // 2 - n // 2:t.size // 2 - n // 2 + n] for t in targets]
    pats = [(k + s) % L for k in keys for s in range(4)]  # pattern 4 u + s: utterance u's keyword shifted by s
    scores, starts, ends, free = dec.ctc_spot(xs, pats)
    assert scores.shape == (len(xs), len(pats)) and np.all(scores <= free[:, None] + 1e-4)
    for u, t in enumerate(targets):
        cost = scores[u, 4 * u:4 * u + 4] - free[u]
        print("utterance %d: keyword %s costs %.3f, shifted %s" % (u, keys[u].tolist(), cost[0], cost[1:].tolist()))
        assert np.isfinite(cost[0]) and np.all(cost[0] > cost[1:]), (u, cost)
        at = t.size // 2 - n // 2
        planted = np.nonzero((full[u] >= at) & (full[u] < at + n))[0]
        assert starts[u, 4 * u] < planted[-1] + 1 and ends[u, 4 * u] > planted[0], (u, starts[u, 4 * u], ends[u, 4 * u], planted)
    alis, ascores, afree = dec.ctc_align_wild(xs, [keys[u] for u in range(len(xs))])  # the same through the alignment
    assert ascores.tobytes() == np.array([scores[u, 4 * u] for u in range(len(xs))], np.float32).tobytes()
    assert afree.tobytes() == free.tobytes()
    assert [span(a) for a in alis] == [(int(starts[u, 4 * u]), int(ends[u, 4 * u])) for u in range(len(xs))]
    dec.close()
