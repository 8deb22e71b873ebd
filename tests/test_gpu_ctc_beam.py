"""CTC prefix beam search on the device (tfk_ctc_beam / tfk_ctc_beam_raw / tfk_ctc_beam_logits, csrc/ctc.hip) against the
float64 numpy restatement of tests/test_ctc_beam_host.py applied to the SAME logits (the engine's own, or chosen ones through
the stand-alone entry).

The device recursion runs in fp32, so scores are compared within `tol` = 4 x the largest |float32 run - float64 run| of the
RESTATEMENT's best score on the same inputs (computed in the test; the factor covers another legitimate fp32 evaluation
order), floored at 1e-6 x |score|.  Hypotheses: the device's best must be one of the restatement's hypotheses whose float64
score lies within 2 tol of its best (two scores each off by at most tol can swap only inside that band); that this band
holds a single hypothesis for at least 75 % of a test's utterances is asserted on the restatement alone, before the device
is consulted."""
import os
import socket
import sys
from ctypes import c_void_p

import numpy as np
import pytest

from test_ctc_beam_host import ctc_log_prob, enumeration_cases, peaky_logits, prefix_beam_search
from test_ctc_decode_host import levenshtein
from test_gpu_ctc_decode import _refs, _split, _toy_ctc
from util import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(input_dim=20, num_layers=2, num_units=32, output_dim=9, nonlin="tanh", batch_norm=True,
          init_learning_rate=1e-3, num_steps=50)


def _device_beam_logits(z, utt, W, P):
    """tfk_ctc_beam_logits on host logits: (hyps[u][n], scores [U, P])"""
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    z = np.ascontiguousarray(z, dtype=np.float32)
    T, O = z.shape
    U = len(utt)
    seg = np.concatenate([[0], np.cumsum(utt)]).astype(np.int32)
    d_z, d_seg = torch.from_numpy(z).cuda(), torch.from_numpy(seg).cuda()
    hyp = torch.full((P, max(T, 1)), -7, dtype=torch.int32, device="cuda")
    hyp_len = torch.full((P, U), -7, dtype=torch.int32, device="cuda")
    score = torch.zeros((P, U), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tfk_ctc_beam_logits(c_void_p(stream), c_void_p(d_z.data_ptr()), O, O, T, c_void_p(d_seg.data_ptr()), U, W, P,
                                       c_void_p(hyp.data_ptr()), c_void_p(hyp_len.data_ptr()), c_void_p(score.data_ptr())))
    torch.cuda.synchronize()
    hyp, hyp_len, score = hyp.cpu().numpy(), hyp_len.cpu().numpy(), score.cpu().numpy()
    for n in range(P):  # the rows past a hypothesis are -1
        for u in range(U):
            assert np.all(hyp[n, seg[u] + hyp_len[n, u]:seg[u + 1]] == -1)
    return [[hyp[n, seg[u]:seg[u] + hyp_len[n, u]].copy() for n in range(P)] for u in range(U)], score.T.copy()


def _restatement(z, utt, W, P=8):
    """float64 N-best of the restatement and the per-utterance tol from its own float32 run"""
    P = min(P, W)
    h64, s64 = prefix_beam_search(z, utt, W, P)
    _, s32 = prefix_beam_search(z, utt, W, 1, dtype=np.float32)
    diff = np.abs(s32[:, 0] - s64[:, 0])
    tol = np.maximum(4.0 * diff.max(), 1e-6 * np.abs(s64[:, 0]))
    return h64, s64, tol


def _check_best(name, z, utt, W, hyps, scores):
    """checks a, b, c of every utterance's best path; returns the largest |device - float64| and the smallest tol"""
    h64, s64, tol = _restatement(z, utt, W)
    band = [[n for n in range(s64.shape[1]) if s64[u, n] >= s64[u, 0] - 2 * tol[u]] for u in range(len(utt))]
    crowded = sum(len(b) > 1 for b in band)
    assert 4 * crowded <= len(utt), "%s: %d of %d utterances have rivals within 2 tol of the best" % (name, crowded, len(utt))
    seg = np.concatenate([[0], np.cumsum(utt)])
    worst = 0.0
    for u in range(len(utt)):
        got, sc = hyps[u][0], float(scores[u, 0])
        exact = ctc_log_prob(z[seg[u]:seg[u + 1]], got)
        err = abs(sc - s64[u, 0])
        print("%s utt %d: T %d labels %d device %.6f float64 %.6f exact %.6f |diff| %.2e tol %.2e band %d"
              % (name, u, utt[u], got.size, sc, s64[u, 0], exact, err, tol[u], len(band[u])))
        assert exact >= sc - tol[u], (name, u, exact, sc, tol[u])                                     # a
        assert err <= tol[u], (name, u, sc, s64[u, 0], tol[u])                                       # b
        assert any(np.array_equal(got, h64[u][n]) for n in band[u]), (name, u, got, h64[u][0])       # c
        worst = max(worst, err)
    print("%s: largest |device - float64| %.3e, smallest tol %.3e" % (name, worst, tol.min()))


def test_standalone_entry_equals_exhaustive_enumeration_cases(gpu):
    """the CPU tier's enumeration matrices (2 labels + blank, T = 6, W = 128 prunes nothing) as one batch of utterances"""
    cases = enumeration_cases()
    z = np.concatenate(cases).astype(np.float32)
    utt = [6] * len(cases)
    P = 8
    hyps, scores = _device_beam_logits(z, utt, 128, P)
    h64, s64, tol = _restatement(z, utt, 128, P)
    worst = 0.0
    for u in range(len(utt)):
        assert np.array_equal(hyps[u][0], h64[u][0]), (u, hyps[u][0], h64[u][0])
        clear = [n for n in range(P) if (n == 0 or s64[u, n - 1] - s64[u, n] > 2 * tol[u])
                 and (n == P - 1 or s64[u, n] - s64[u, n + 1] > 2 * tol[u])]
        assert 0 in clear and len(clear) >= 4
        for n in clear:
            assert np.array_equal(hyps[u][n], h64[u][n]), (u, n)
            # (the floor of tol is relative to the score compared: path n's own, not the best path's)
            tol_n = max(tol[u], 1e-6 * abs(s64[u, n]))
            assert abs(scores[u, n] - s64[u, n]) <= tol_n, (u, n, scores[u, n], s64[u, n], tol_n)
            worst = max(worst, abs(scores[u, n] - s64[u, n]))
    print("enumeration cases: largest |device - float64| %.3e, tol %.3e ... %.3e" % (worst, tol.min(), tol.max()))


def _sharpen(eng, rng, scale, blank_bias):
    """output layer with logits of standard deviation ~scale and a biased blank: hypotheses far shorter than the frames"""
    from tfkaldi_amd import _lib
    eng.set(_lib.WEIGHTS, eng.L, (rng.standard_normal((eng.H, eng.O)) * scale / np.sqrt(eng.H)).astype(np.float32))
    bias = np.zeros(eng.O, np.float32)
    bias[eng.O - 1] = blank_bias
    eng.set(_lib.BIASES, eng.L, bias)


@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
@pytest.mark.parametrize("O", [9, 36])
def test_engine_entry_equals_restatement_on_the_engines_logits(gpu, dtype, O):
    rng = np.random.default_rng(100 + O)
    eng, _ = make_pair(rng, max_frames=512, compute_dtype=dtype, **dict(KW, output_dim=O))
    _sharpen(eng, rng, 6.0, 3.0)
    utt = [30, 0, 1, 77, 140, 2, 0, 65]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    labels, lab = _refs(rng, len(utt), O)
    z = eng.posteriors(X, raw_logits=True)
    for W in (1, 10, 100):
        P = min(3, W)
        hyps, scores, edits = eng.ctc_beam(X, utt, beam_width=W, top_paths=P, labels=labels, label_lens=lab)
        assert scores.shape == (len(utt), P) and scores.dtype == np.float32 and edits.dtype == np.int32
        assert all(len(h) == P and all(p.dtype == np.int32 for p in h) for h in hyps)
        _check_best("%s O=%d W=%d" % (dtype, O, W), z, utt, W, hyps, scores)
        assert edits.tolist() == [levenshtein(h[0], r) for h, r in zip(hyps, _split(labels, lab))]
        for u in (1, 6):  # zero-frame utterances: the empty hypothesis with score 0, then padding
            assert all(p.size == 0 for p in hyps[u]) and scores[u].tolist() == [0.0] + [-np.inf] * (P - 1)
        assert np.all(scores[:, :-1] >= scores[:, 1:])  # best first
        alone = eng.ctc_beam(X, utt, beam_width=W, top_paths=P)
        assert alone[2] is None and np.array_equal(alone[1], scores)
    assert sum(h[0].size for h in hyps) > 20  # a non-trivial decode
    eng.close()


def test_standalone_entry_at_cfg5_size_on_peaky_logits(gpu):
    """[12800, 36] host-made logits (16 x 800 frames, ~100 labels each, the blank dominant elsewhere), W = 100: the
    restatement's 2-tol band condition for this seed is what tests/test_ctc_beam_host.py::
    test_peaky_cfg5_logits_have_clear_winners asserts on the CPU, on the same 16 utterances"""
    rng = np.random.default_rng(55)
    z = peaky_logits(rng, 16 * 800, 36, 16 * 100)
    utt = [800] * 16
    hyps, scores = _device_beam_logits(z, utt, 100, 3)
    _check_best("cfg5 peaky logits", z, utt, 100, hyps, scores)
    again = _device_beam_logits(z, utt, 100, 3)
    assert np.array_equal(again[1], scores) and all(np.array_equal(a, b) for x, y in zip(again[0], hyps) for a, b in zip(x, y))


def test_engine_entry_at_cfg5_size(gpu):
    """BASELINE configs[4]'s micro-batch: 16 utterances x 800 frames of a 4x512 DNN, 35 characters + blank, the output layer
    scaled and the blank biased so that hypotheses are ~100 labels, W = 100"""
    rng = np.random.default_rng(5)
    kw = dict(input_dim=440, num_layers=4, num_units=512, output_dim=36, nonlin="relu", batch_norm=True,
              init_learning_rate=1e-3, num_steps=50, max_frames=12800)
    eng, _ = make_pair(rng, **kw)
    _sharpen(eng, rng, 8.0, 7.0)
    utt = [800] * 16
    X = rng.standard_normal((12800, 440)).astype(np.float32)
    labels, lab = _refs(rng, 16, 36, 90, 110)
    z = eng.posteriors(X, raw_logits=True)
    hyps, scores, edits = eng.ctc_beam(X, utt, beam_width=100, top_paths=3, labels=labels, label_lens=lab)
    sizes = [h[0].size for h in hyps]
    print("cfg5 engine: hypothesis lengths %d ... %d" % (min(sizes), max(sizes)))
    assert 40 <= np.mean(sizes) <= 250
    _check_best("cfg5 engine", z, utt, 100, hyps, scores)
    assert edits.tolist() == [levenshtein(h[0], r) for h, r in zip(hyps, _split(labels, lab))]
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
    labels, lab = _refs(rng, len(utts), 12)
    raw = np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)

    def same(a, b):
        return (all(np.array_equal(p, q) for x, y in zip(a[0], b[0]) for p, q in zip(x, y))
                and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]))

    host = eng.ctc_beam(np.concatenate([u.spliced() for u in utts]), lens, beam_width=20, top_paths=4, labels=labels,
                        label_lens=lab)
    dev = eng.ctc_beam_raw(raw, lens, C, cmvn=cmvn_table(utts), beam_width=20, top_paths=4, labels=labels, label_lens=lab)
    cuda = eng.ctc_beam_raw(torch.from_numpy(raw).cuda(), lens, C, cmvn=cmvn_table(utts), beam_width=20, top_paths=4,
                            labels=labels, label_lens=lab)
    assert same(host, dev) and same(host, cuda)
    assert same(host, eng.ctc_beam(np.concatenate([u.spliced() for u in utts]), lens, beam_width=20, top_paths=4,
                                   labels=labels, label_lens=lab))  # two identical calls are bit-identical
    assert host[2].tolist() == [levenshtein(h[0], r) for h, r in zip(host[0], _split(labels, lab))]
    assert sum(h[0].size for h in host[0]) > 5
    eng.close()


def test_fewer_survivors_than_top_paths_pads(gpu):
    """one frame, 3 labels + blank: 4 prefixes exist, so paths 4 ... 7 of W = 8 are empty with score -inf"""
    z = np.array([[2.0, 1.0, 0.0, 0.5]], np.float32)
    hyps, scores = _device_beam_logits(z, [1, 0], 8, 8)
    lp = z[0] - np.log(np.exp(z[0].astype(np.float64)).sum())
    assert [h.tolist() for h in hyps[0]] == [[0], [1], [], [2]] + [[]] * 4
    assert np.allclose(scores[0, :4], [lp[0], lp[1], lp[3], lp[2]], rtol=0, atol=1e-6)
    assert np.all(scores[0, 4:] == -np.inf)
    assert all(h.size == 0 for h in hyps[1]) and scores[1].tolist() == [0.0] + [-np.inf] * 7


def test_limits_are_reported_and_leave_the_engine_usable(gpu):
    import torch
    from tfkaldi_amd import _lib
    from tfkaldi_amd._lib import EngineError
    rng = np.random.default_rng(13)
    eng, _ = make_pair(rng, max_frames=256, **KW)
    utt = [20, 15]
    X = rng.standard_normal((35, KW["input_dim"])).astype(np.float32)
    good = eng.ctc_beam(X, utt, beam_width=16, top_paths=2)
    for kw, word in ((dict(beam_width=129), "beam_width"), (dict(beam_width=0, top_paths=0), "beam_width")):
        with pytest.raises((EngineError, ValueError), match=word):
            eng.ctc_beam(X, utt, **kw)
    h, n, s = np.empty((3, 35), np.int32), np.empty((3, 2), np.int32), np.empty((3, 2), np.float32)
    lens = np.array(utt, np.int32)
    ptr = lambda a: a.ctypes.data_as(c_void_p)
    call = lambda W, P, flags=0: eng.lib.tfk_ctc_beam(eng._h, ptr(X), X.shape[1], 35, ptr(lens), 2, W, P, c_void_p(None),
                                                      c_void_p(None), ptr(h), ptr(n), ptr(s), c_void_p(None), flags)
    for W, P, flags, word in ((129, 1, 0, b"128"), (4, 5, 0, b"top_paths"), (0, 1, 0, b"beam_width"),
                              (4, 1, _lib.RAW_DEVICE, b"flags")):
        assert call(W, P, flags) != 0
        assert word in eng.lib.tfk_last_error(), (W, P, eng.lib.tfk_last_error())
        again = eng.ctc_beam(X, utt, beam_width=16, top_paths=2)
        assert again[1].tobytes() == good[1].tobytes()
    assert call(3, 3) == 0
    eng.close()
    wide, _ = make_pair(rng, max_frames=256, **dict(KW, output_dim=65))  # more classes than the kernel's label mask holds
    with pytest.raises(EngineError, match="output_dim"):
        wide.ctc_beam(X, utt, beam_width=4)
    assert len(wide.ctc_greedy(X, utt)[0]) == 2  # the engine works afterwards
    wide.close()
    lib = _lib.load()
    z = torch.zeros((4, 70), dtype=torch.float32, device="cuda")
    assert lib.tfk_ctc_beam_logits(c_void_p(0), c_void_p(z.data_ptr()), 70, 70, 4, c_void_p(z.data_ptr()), 1, 4, 1,
                                   c_void_p(z.data_ptr()), c_void_p(z.data_ptr()), c_void_p(z.data_ptr())) != 0
    assert b"64" in lib.tfk_last_error()


def test_decoder_and_trainer_end_to_end(gpu, tmp_path):
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    for _ in range(60):
        tr.update(xs, ys)
    greedy = tr.label_errors(xs, ys)
    beam = tr.label_errors(xs, ys, beam_width=100)
    assert greedy == tr.label_errors(xs, ys, beam_width=None)
    assert type(beam[0]) is int and beam[1] == greedy[1] == sum(len(y) for y in ys)
    hyps, scores, _ = tr.engine.ctc_beam(np.concatenate(xs), [len(x) for x in xs], beam_width=100, top_paths=2)
    assert beam[0] == sum(levenshtein(h[0], np.asarray(y).astype(np.int64)) for h, y in zip(hyps, ys))
    print("toy model after 60 updates: label errors greedy %d, beam %d of %d" % (greedy[0], beam[0], beam[1]))
    tr.save_model(str(tmp_path / "model"))
    tr.close()
    dec = Decoder(dnn, F, maxlen)
    dec.restore(str(tmp_path / "model"))
    got, got_scores = dec.ctc_beam_search(xs, beam_width=100, top_paths=2)
    assert got_scores.tobytes() == scores.tobytes()
    assert all(np.array_equal(a, b) for x, y in zip(got, hyps) for a, b in zip(x, y))
    assert all(isinstance(coder.decode(h[0]), str) for h in got)
    assert dec.ctc_beam_search([])[0] == []
    dec.close()


def _dp_data(num_mb, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(num_mb):
        utt = [30 + 3 * i, 17 + i, 0 if i == 1 else 9]
        X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
        labels, lab = _refs(rng, 3, KW["output_dim"], 0, 8)
        out.append((X, np.array(utt, np.int32), labels, lab))
    return out


def _dp_worker(rank, world, port, num_mb, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), TFK_SHARE_DEVICE="1", TFK_DIST_BACKEND="gloo")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    from tfkaldi_amd.dataparallel import CtcMicroBatch, DataParallel, init_from_env
    from util import make_pair as pair
    init_from_env()
    dp = DataParallel()
    assert dp.enabled
    eng, _ = pair(np.random.default_rng(5), max_frames=256, torch_state=True, **KW)
    got = dp.label_errors(eng, [CtcMicroBatch(*mb) for mb in _dp_data(num_mb, 3)], beam_width=100)
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(got, dtype=np.int64))
    eng.close()
    dist.destroy_process_group()


def test_beam_label_errors_two_ranks_equal_single_process(gpu, tmp_path):
    import torch.multiprocessing as mp
    from tfkaldi_amd.dataparallel import CtcMicroBatch, DataParallel
    world, num_mb = 2, 3
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_dp_worker, args=(world, port, num_mb, str(tmp_path)), nprocs=world, join=True)
    eng, _ = make_pair(np.random.default_rng(5), max_frames=256, **KW)
    want = DataParallel().label_errors(eng, [CtcMicroBatch(*mb) for mb in _dp_data(num_mb, 3)], beam_width=100)
    eng.close()
    assert want[0] > 0 and want[1] > 0
    for rank in range(world):
        assert tuple(np.load(os.path.join(str(tmp_path), "rank%d.npy" % rank)).tolist()) == want
