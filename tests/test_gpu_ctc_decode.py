"""Best-path CTC decoding and label errors on the device (tfk_ctc_greedy / tfk_ctc_greedy_raw / tfk_label_edit_distance,
csrc/ctc.hip) against the numpy restatement of tf.nn.ctc_greedy_decoder(merge_repeated=True) + tf.edit_distance
(tests/test_ctc_decode_host.py) applied to the SAME engine's logits: the forward is deterministic, so the two agree exactly."""
import os
import socket
import sys
from ctypes import c_void_p

import numpy as np
import pytest

from test_ctc_decode_host import best_path, levenshtein
from util import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(input_dim=20, num_layers=2, num_units=32, output_dim=9, nonlin="tanh", batch_norm=True,
          init_learning_rate=1e-3, num_steps=50)


def _refs(rng, U, O, lo=0, hi=40):
    lab = rng.integers(lo, hi + 1, size=U).astype(np.int32)
    return rng.integers(0, O - 1, size=int(lab.sum())).astype(np.int32), lab


def _split(labels, lens):
    return np.split(np.asarray(labels), np.cumsum(lens)[:-1])


def _check_against_logits(eng, X, utt, labels, lab):
    hyps, edits = eng.ctc_greedy(X, utt, labels, lab)
    want = best_path(eng.posteriors(X, raw_logits=True), utt)
    assert len(hyps) == len(want)
    for u, (h, w) in enumerate(zip(hyps, want)):
        assert h.dtype == np.int32 and np.array_equal(h, w), (u, h[:20], w[:20])
    assert edits.dtype == np.int32
    assert edits.tolist() == [levenshtein(h, r) for h, r in zip(want, _split(labels, lab))]
    alone, none = eng.ctc_greedy(X, utt)  # without references: the same hypotheses
    assert none is None and all(np.array_equal(a, h) for a, h in zip(alone, hyps))
    return hyps


@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
@pytest.mark.parametrize("O", [9, 36, 2000])
def test_greedy_equals_numpy_on_the_engines_logits(gpu, dtype, O):
    rng = np.random.default_rng(O)
    eng, _ = make_pair(rng, max_frames=512, compute_dtype=dtype, **dict(KW, output_dim=O))
    utt = [30, 0, 1, 77, 140, 2, 0, 65]  # zero- and one-frame utterances among them
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    labels, lab = _refs(rng, len(utt), O)
    hyps = _check_against_logits(eng, X, utt, labels, lab)
    assert hyps[1].size == 0 and hyps[6].size == 0 and hyps[2].size <= 1
    assert sum(h.size for h in hyps) > 20  # a non-trivial decode
    eng.close()


def test_greedy_at_cfg5_size(gpu):
    """BASELINE configs[4]'s micro-batch: 16 utterances x ~800 frames of a 4x512 DNN, 35 characters + blank, ~100 labels"""
    rng = np.random.default_rng(5)
    kw = dict(input_dim=440, num_layers=4, num_units=512, output_dim=36, nonlin="relu", batch_norm=True,
              init_learning_rate=1e-3, num_steps=50, max_frames=12800)
    eng, _ = make_pair(rng, **kw)
    utt = [800] * 16
    X = rng.standard_normal((12800, 440)).astype(np.float32)
    labels, lab = _refs(rng, 16, 36, 90, 110)
    _check_against_logits(eng, X, utt, labels, lab)
    eng.close()


def test_raw_entry_equals_host_spliced(gpu):
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(8)
    D, C = 4, 2
    eng, _ = make_pair(rng, max_frames=256, **dict(KW, input_dim=D * (2 * C + 1), output_dim=12))
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 5, 63, 17)]
    lens = [u.shape[0] for u in utts]
    labels, lab = _refs(rng, len(utts), 12)
    host = eng.ctc_greedy(np.concatenate([u.spliced() for u in utts]), lens, labels, lab)
    dev = eng.ctc_greedy_raw(np.concatenate([np.asarray(u) for u in utts]), lens, C, cmvn=cmvn_table(utts),
                             labels=labels, label_lens=lab)
    assert all(np.array_equal(a, b) for a, b in zip(host[0], dev[0])) and np.array_equal(host[1], dev[1])
    assert sum(h.size for h in host[0]) > 5
    eng.close()


def test_refused_cmvn_table_releases_the_device_tensor(gpu):
    """a device tensor with a wrong-shaped cmvn table: ValueError, no reference to the tensor stays parked in the engine, and
    the next valid call gives the bytes it gave before"""
    import torch
    from tfkaldi_amd.processing.feature_reader import Unspliced, cmvn_table
    rng = np.random.default_rng(8)
    D, C = 4, 2
    eng, _ = make_pair(rng, max_frames=256, **dict(KW, input_dim=D * (2 * C + 1), output_dim=12))
    utts = [Unspliced(rng.standard_normal((n, D)) * 2 + 1, C,
                      np.stack([rng.standard_normal(D), 0.5 + rng.random(D)]).astype(np.float32)) for n in (40, 5, 63, 17)]
    lens = [u.shape[0] for u in utts]
    labels, lab = _refs(rng, len(utts), 12)
    table = cmvn_table(utts)
    raw = torch.from_numpy(np.concatenate([np.asarray(u) for u in utts]).astype(np.float32)).cuda()
    call = lambda cmvn: eng.ctc_greedy_raw(raw, lens, C, cmvn=cmvn, labels=labels, label_lens=lab)
    before = call(table)
    assert sum(h.size for h in before[0]) > 5
    for bad in (table[:3], table[:, :1], table[:, :, :D - 1]):
        with pytest.raises(ValueError, match="cmvn table"):
            call(bad)
        assert eng._raw_pending is None
    after = call(table)
    assert len(after[0]) == len(before[0])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(after[0], before[0])) and after[1].tobytes() == before[1].tobytes()
    eng.close()


def test_known_answers_from_a_zero_output_layer(gpu):
    """right after initialize() the output layer is zero: every logit is exactly 0, class 0 wins every frame's tie"""
    from tfkaldi_amd import _lib
    rng = np.random.default_rng(9)
    eng, _ = make_pair(rng, output_too=False, max_frames=256, **KW)
    O = KW["output_dim"]
    utt = [12, 0, 1, 30, 5]
    X = rng.standard_normal((sum(utt), KW["input_dim"])).astype(np.float32)
    lab = np.array([4, 3, 0, 7, 2], np.int32)
    labels = rng.integers(1, O - 1, size=int(lab.sum())).astype(np.int32)
    labels[4] = 0  # utterance 1's reference holds a 0 (it has no frames: distance = its length)
    labels[10] = 0  # utterance 3's reference holds a 0
    hyps, edits = eng.ctc_greedy(X, utt, labels, lab)
    assert [h.tolist() for h in hyps] == [[0] if n else [] for n in utt]
    refs = _split(labels, lab)
    want = [(len(r) - (0 in r.tolist()) if len(r) else 1) if n else len(r) for n, r in zip(utt, refs)]
    assert edits.tolist() == want
    bias = np.zeros(O, np.float32)
    bias[O - 1] = 1.0  # the blank wins every frame: empty hypotheses
    eng.set(_lib.BIASES, eng.L, bias)
    hyps, edits = eng.ctc_greedy(X, utt, labels, lab)
    assert all(h.size == 0 for h in hyps) and edits.tolist() == lab.tolist()
    eng.close()


def test_engine_edit_distances_for_long_references(gpu):
    rng = np.random.default_rng(10)
    eng, _ = make_pair(rng, max_frames=4096, **dict(KW, output_dim=36))
    utt = [600, 300, 900, 50, 700, 400]
    X = (rng.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
    lab = np.array([511, 0, 257, 64, 129, 300], np.int32)  # every register tile, the limit, an empty reference
    labels = rng.integers(0, 35, size=int(lab.sum())).astype(np.int32)
    _check_against_logits(eng, X, utt, labels, lab)
    eng.close()


def _device_edit_distance(pairs):
    import torch
    from tfkaldi_amd import _lib
    lib = _lib.load()
    hyp_off = np.concatenate([[0], np.cumsum([len(h) for h, _ in pairs])]).astype(np.int32)
    ref_off = np.concatenate([[0], np.cumsum([len(r) for _, r in pairs])]).astype(np.int32)
    flat = lambda seqs: np.concatenate([np.asarray(s, np.int32) for s in seqs] + [np.zeros(1, np.int32)])
    t = {k: torch.from_numpy(v).cuda() for k, v in dict(hyp=flat([h for h, _ in pairs]), ref=flat([r for _, r in pairs]),
                                                       hyp_off=hyp_off, ref_off=ref_off).items()}
    dist = torch.full((len(pairs),), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.tfk_label_edit_distance(c_void_p(stream), c_void_p(t["hyp"].data_ptr()), c_void_p(t["hyp_off"].data_ptr()),
                                           c_void_p(t["ref"].data_ptr()), c_void_p(t["ref_off"].data_ptr()), len(pairs),
                                           c_void_p(dist.data_ptr())))
    return dist.cpu().numpy().tolist()


def test_label_edit_distance_adversarial_pairs(gpu):
    rng = np.random.default_rng(12)
    seq = lambda n, a=30: rng.integers(0, a, size=n).tolist()
    s300, s511 = seq(300), seq(511)
    pairs = [
        (s300, s300),                               # identical
        (seq(200, 5), [x + 100 for x in seq(180, 5)]),  # disjoint alphabets
        (s511, s511[::-1]),                         # reversed
        ([], s511), (s300, []), ([], []),           # one side empty
        (seq(2000), seq(511)),                      # a 2000-label hypothesis against the longest reference
        ([7] * 700, [7] * 64), ([7] * 64, [7] * 500), ([3] * 129, [4] * 129),  # long runs of one symbol
        ([1], [1]), ([1], [2]), (seq(64), seq(65)), (seq(65), seq(64)), (seq(1), seq(511)),
    ]
    pairs += [(seq(int(rng.integers(0, 900)), 6), seq(int(rng.integers(0, 512)), 6)) for _ in range(40)]
    got = _device_edit_distance(pairs)
    assert got == [levenshtein(h, r) for h, r in pairs]
    # a reference beyond the limit (or a negative length) is marked, not computed
    bad = _device_edit_distance([(seq(10), seq(512)), ([1, 2, 3], [1, 3])])
    assert bad == [-1, 1]


def test_errors_leave_the_engine_usable(gpu):
    from tfkaldi_amd import _lib
    rng = np.random.default_rng(13)
    eng, _ = make_pair(rng, max_frames=256, **KW)
    O = KW["output_dim"]
    utt = np.array([20, 15], np.int32)
    X = rng.standard_normal((35, KW["input_dim"])).astype(np.float32)
    labels, lab = _refs(rng, 2, O, 3, 6)
    good = eng.ctc_greedy(X, utt, labels, lab)

    def raw_call(hyp=True, hyp_len=True, edits=True, refs=True, flags=0, T=35, lab_vals=labels, lab_lens=lab):
        h = np.empty(T, np.int32)
        n = np.empty(2, np.int32)
        d = np.empty(2, np.int32)
        lv = np.ascontiguousarray(lab_vals, np.int32)
        ll = np.ascontiguousarray(lab_lens, np.int32)
        ptr = lambda a, on: a.ctypes.data_as(c_void_p) if on else c_void_p(None)
        return eng.lib.tfk_ctc_greedy(eng._h, X.ctypes.data_as(c_void_p), X.shape[1], T, utt.ctypes.data_as(c_void_p), 2,
                                      ptr(lv, refs), ptr(ll, refs), ptr(h, hyp), ptr(n, hyp_len), ptr(d, edits), flags)

    big = rng.integers(0, O - 1, size=512).astype(np.int32)
    cases = {
        "label >= O - 1": dict(lab_vals=np.where(np.arange(labels.size) == 1, O - 1, labels)),
        "more than 511 labels": dict(lab_vals=np.concatenate([big, labels[:lab[1]]]), lab_lens=[512, lab[1]]),
        "utt_len does not sum to T": dict(T=34),
        "NULL hyp": dict(hyp=False), "NULL hyp_len": dict(hyp_len=False),
        "edits without references": dict(refs=False),
        "unknown flag": dict(flags=_lib.DEVICE_PTRS), "raw-only flag": dict(flags=_lib.RAW_DEVICE),
    }
    for name, kw in cases.items():
        assert raw_call(**kw) != 0, name
        assert eng.lib.tfk_last_error(), name
        again = eng.ctc_greedy(X, utt, labels, lab)  # the next valid call succeeds, with the same result
        assert all(np.array_equal(a, b) for a, b in zip(again[0], good[0])) and np.array_equal(again[1], good[1]), name
    assert raw_call() == 0
    eng.close()


# the forward-only calls that share the engine's pass plumbing; refs None: the call without references (forced alignment has
# no such form, posteriors takes none)
FORWARD_ONLY = {
    "posteriors": lambda eng, X, utt, refs: eng.posteriors(X, raw_logits=True),
    "ctc_greedy": lambda eng, X, utt, refs: eng.ctc_greedy(X, utt, *(refs or ())),
    "ctc_beam": lambda eng, X, utt, refs: eng.ctc_beam(X, utt, 8, 2, *(refs or ())),
    "ctc_align": lambda eng, X, utt, refs: eng.ctc_align(X, utt, *refs) if refs else None,
}


@pytest.mark.parametrize("call", sorted(FORWARD_ONLY))
def test_decoding_between_steps_has_no_side_effects(gpu, call):
    """a training trace with forward-only calls between (and inside) the steps is bit-identical to one without (no dropout)"""
    decode = FORWARD_ONLY[call]

    def trace(on):
        rng = np.random.default_rng(21)
        eng, _ = make_pair(rng, max_frames=256, **KW)
        data = np.random.default_rng(22)
        losses = []
        for step in range(4):
            utt = [25 + step, 18]
            X = (data.standard_normal((sum(utt), KW["input_dim"])) * 1.5).astype(np.float32)
            labels, lab = _refs(data, 2, KW["output_dim"], 2, 6)  # (2..6 labels: every utterance is long enough for them)
            if on:
                decode(eng, X[::-1].copy(), utt[::-1], (labels, lab[::-1]))
            eng.accumulate_ctc(X[:utt[0]], [utt[0]], labels[:lab[0]], [lab[0]])
            if on:
                decode(eng, X, utt, (labels, lab) if call == "ctc_align" else None)
            eng.accumulate_ctc(X[utt[0]:], [utt[1]], labels[lab[0]:], [lab[1]], last=True)
            losses.append(eng.apply())
            if on:
                decode(eng, X, utt, (labels, lab))
        from tfkaldi_amd import _lib
        sums = [eng.param_checksum(w) for w in (0, 2)]
        stats = [eng.get(kind, l).tobytes() for l in range(eng.L) for kind in (_lib.BN_MOVING_MEAN, _lib.BN_MOVING_VAR)]
        state = (eng.global_step, eng.scalar(_lib.ADAM_STEPS), eng.get(_lib.WEIGHTS, 0, _lib.SLOT_ADAM_V).tobytes())
        eng.close()
        return losses, sums, stats, state
    assert trace(False) == trace(True)


# Measured on the GPU (LER of the training batch every 25 updates): 0.81 after 200, 0.33 after 275, 0.26 after 300, 0.02
# after 350, 0 from 375 on -- 400 leaves 100 updates of margin past the 0.3 crossing
E2E_STEPS = 400


def _toy_ctc(tmp_path, numutt=2, lengths=(90, 70, 120, 80, 100, 60, 75, 110)):
    """the toy setup of test_gpu_ctc.py::test_ctc_trainer_end_to_end: TextBatchDispenser + TextCoder character targets"""
    from tfkaldi_amd import synthetic
    from tfkaldi_amd.neuralNetworks.classifiers import activation as act
    from tfkaldi_amd.neuralNetworks.classifiers.dnn import DNN
    from tfkaldi_amd.processing import batchdispenser, feature_reader, target_coder, target_normalizers
    D, C, U = 8, 2, 4
    lengths = list(lengths)
    paths = synthetic.write_corpus(str(tmp_path), len(lengths), 10, feat_dim=D, lengths=lengths, num_speakers=2)
    text = synthetic.write_text_targets(str(tmp_path), len(lengths))
    reader = feature_reader.FeatureReader(paths["feats_scp"], paths["cmvn_scp"], paths["utt2spk"], C, max(lengths))
    coder = target_coder.TextCoder(target_normalizers.aurora4_normalizer)
    disp = batchdispenser.TextBatchDispenser(reader, coder, U, text)
    O = coder.num_labels + 1
    dnn = DNN(O, 2, 48, act.TfActivation(act.Batchnorm(None), "relu"), False)
    return dnn, disp, coder, D * (2 * C + 1), max(lengths)


def test_ctc_trainer_decode_end_to_end(gpu, tmp_path):
    from tfkaldi_amd.neuralNetworks.decoder import Decoder
    from tfkaldi_amd.neuralNetworks.trainer import CTCTrainer
    dnn, disp, coder, F, maxlen = _toy_ctc(tmp_path)
    tr = CTCTrainer(dnn, F, maxlen, disp.max_target_length, 3e-3, 1.0, 1000, 2, seed=11)
    tr.initialize()
    xs, ys = disp.get_batch()
    n_ref = sum(len(y) for y in ys)
    before = tr.label_errors(xs, ys)
    assert before[1] == n_ref and before[0] > 0
    for _ in range(E2E_STEPS):
        tr.update(xs, ys)
    edits, labels = tr.label_errors(xs, ys)
    assert type(edits) is int and type(labels) is int and labels == n_ref
    hyps, _ = tr.engine.ctc_greedy(np.concatenate(xs), [len(x) for x in xs])
    assert edits == sum(levenshtein(h, np.asarray(y).astype(np.int64)) for h, y in zip(hyps, ys))
    assert edits / labels < 0.3, (edits, labels, before)
    assert tr.label_errors(None, ys) is None and tr.label_errors(xs, None) is None
    text = [coder.decode(h) for h in hyps]
    assert all(isinstance(t, str) for t in text)
    tr.save_model(str(tmp_path / "model"))
    tr.close()
    dec = Decoder(dnn, F, maxlen)
    dec.restore(str(tmp_path / "model"))
    got = dec.ctc_best_path(xs)
    assert len(got) == len(hyps) and all(np.array_equal(a, b) for a, b in zip(got, hyps))
    assert dec.ctc_best_path([]) == []
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
    got = dp.label_errors(eng, [CtcMicroBatch(*mb) for mb in _dp_data(num_mb, 3)])
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(got, dtype=np.int64))
    eng.close()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("num_mb", [3, 1])  # uneven blocks, an idle rank
def test_label_errors_two_ranks_equal_single_process(gpu, tmp_path, num_mb):
    import torch.multiprocessing as mp
    from tfkaldi_amd.dataparallel import CtcMicroBatch, DataParallel
    world = 2
    mp.spawn(_dp_worker, args=(world, _free_port(), num_mb, str(tmp_path)), nprocs=world, join=True)
    eng, _ = make_pair(np.random.default_rng(5), max_frames=256, **KW)
    want = DataParallel().label_errors(eng, [CtcMicroBatch(*mb) for mb in _dp_data(num_mb, 3)])
    eng.close()
    assert want[0] > 0 and want[1] > 0
    for rank in range(world):
        assert tuple(np.load(os.path.join(str(tmp_path), "rank%d.npy" % rank)).tolist()) == want
