"""The CTC loss kernels (ctc_gather, ctc_alpha_beta_kernel<R>, ctc_grad, ctc_loss_reduce in tfkaldi_amd/csrc/ctc.hip) at
their own edges: every register tile R = 2 / 4 / 8 / 16 with the last states in lane 63 or straddling two lanes, frame
counts around the 8-frame prefetch ring, utterances without frames, peaky logits, a shrinking scratch stride, the label
limit and the other two arithmetics.

How the CTC kernels are isolated from the network: the net of cases a-f has neither batch norm nor dropout, so the
evaluation and the training forward pass compute the same logits.  Per case eval_accumulate_ctc runs first -- it leaves
the logits in place, DBG_LOGITS then holds the device's own fp32 logits `zdev` -- and accumulate_ctc second, after which
DBG_LOGITS holds dLogits.  The reference is the vectorised float64 oracle on `zdev` (oracle/ctc_oracle.py, pinned against
the scalar oracle and torch in tests/test_ctc_oracle.py), so the comparison sees the round-off of the CTC kernels alone.
The guard of that equivalence: the training pass's BATCH_LOSS equals the evaluation pass's to rtol 1e-6.  The loss of
the evaluation pass is compared with the oracle BEFORE the training pass is launched.

Tolerances are the project's own (tests/test_gpu_ctc.py): loss rtol 2e-5 per batch, 1e-6 for a single utterance; dLogits
rtol 1e-4 + atol 2e-5 below 200 frames per batch, 2e-4 from there on.  The reference's own uncertainty -- the oracle on
logits moved by one fp32 ulp, random signs, 3 draws -- is computed per case and printed next to the device's error (one
"ctc-edges" line per case under `pytest -s`, headed by the library's build id)."""
import numpy as np
import pytest

from oracle.ctc_oracle import ctc_batch, log_softmax
from test_gpu_ctc import KW
from test_gpu_ctc_beam import _sharpen
from util import assert_close, engine_grads, make_pair

pytestmark = pytest.mark.gpu

NET = dict(input_dim=20, num_layers=2, num_units=32, nonlin="tanh", batch_norm=False, init_learning_rate=1e-3,
           num_steps=50, max_frames=2048)
PEAKY = (12.0, 3.0)  # logit scale and blank bias of a trained, peaky model (as test_gpu_ctc_beam._sharpen is used)


def _tile(max_labels):
    """states per lane the loss kernel picks for its longest label sequence (regs_for in ctc.hip)"""
    r = 2
    while 64 * r < 2 * max_labels + 1:
        r *= 2
    return r


def _make(O, sharpen=None, seed=7, **over):
    rng = np.random.default_rng(seed + O)
    eng, oracle = make_pair(rng, **dict(NET, output_dim=O, **over))
    if sharpen:
        _sharpen(eng, rng, *sharpen)
    return eng, oracle


@pytest.fixture(scope="module")
def nets(gpu):
    """engines by (O, sharpen), made on first use, shared by the cases of this file and closed at its end"""
    from tfkaldi_amd.build import library_id
    print("\nctc-edges build id %s" % library_id())
    made = {}

    def get(O, sharpen=None):
        if (O, sharpen) not in made:
            made[(O, sharpen)] = _make(O, sharpen)[0]
        return made[(O, sharpen)]
    yield get
    for eng in made.values():
        eng.close()


def _labels(rng, S, O, repeat=0.0, distinct=False):
    if distinct:
        return rng.permutation(O - 1)[:S].astype(np.int32)
    lab = rng.integers(0, O - 1, size=S)
    for i in range(1, S):
        if rng.random() < repeat:
            lab[i] = lab[i - 1]
    return lab.astype(np.int32)


def _min_frames(lab):
    """frames the shortest alignment needs: one per label and a blank between equal neighbours"""
    lab = np.asarray(lab)
    return len(lab) + int((lab[1:] == lab[:-1]).sum())


def _frames(rng, T):
    return (rng.standard_normal((T, NET["input_dim"])) * 1.5).astype(np.float32)


def _reset(eng):
    eng.eval_finish()  # reads the scalars back: batch_loss / num_frames start from zero again


def _sensitivity(zdev, utt, labels, lab, loss, grad):
    """what one fp32 ulp of the logits is worth in the reference (the oracle alone, no device figure in it)"""
    rng = np.random.default_rng(0)
    d_loss = d_grad = 0.0
    for _ in range(3):
        toward = np.where(rng.integers(0, 2, size=zdev.shape) > 0, np.inf, -np.inf).astype(np.float32)
        l, g, _ = ctc_batch(np.nextafter(zdev, toward).astype(np.float64), utt, labels, lab, fast=True)
        if np.isfinite(loss) and loss != 0:
            d_loss = max(d_loss, abs(l - loss) / abs(loss))
        d_grad = max(d_grad, float(np.abs(g - grad).max()) if g.size else 0.0)
    return d_loss, d_grad


def _loss_close(name, got, want, rtol):
    if np.isfinite(want):
        assert_close(name, got, want, rtol, 0)
    else:
        assert got == want, (name, got, want)


def _rel(got, want):
    if not np.isfinite(want):
        return 0.0 if got == want else np.inf
    return abs(got - want) / max(abs(want), 1e-30)


def _eval_pass(eng, X, utt, labels, lab):
    """(the device's logits, the loss sum of the evaluation pass)"""
    from tfkaldi_amd import _lib
    _reset(eng)
    eng.eval_accumulate_ctc(X, utt, labels, lab)
    zdev = eng.debug_fetch(_lib.DBG_LOGITS, 0, X.shape[0])
    loss = eng.scalar(_lib.BATCH_LOSS)
    _reset(eng)
    return zdev, loss


def _train_pass(eng, X, utt, labels, lab):
    """(loss sum, label count, dLogits) of one training pass"""
    from tfkaldi_amd import _lib
    _reset(eng)
    eng.accumulate_ctc(X, utt, labels, lab)
    loss, count = eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES)
    dlog = eng.debug_fetch(_lib.DBG_LOGITS, 0, X.shape[0])
    _reset(eng)
    return loss, count, dlog


def _report(name, utt, lab, sens, errs):
    print("ctc-edges %-26s R %2d  U %2d  T %4d (longest %4d)  S max %3d | reference +-1 ulp: loss %.1e dlogits %.1e | "
          "device: eval loss %.1e loss %.1e dlogits %.1e" % ((name, _tile(max(lab)), len(utt), int(np.sum(utt)),
                                                              max(utt), max(lab)) + tuple(sens) + tuple(errs)))


def _check(name, eng, X, utt, labels, lab, reference=None):
    """One batch through the evaluation and the training pass against the oracle on the device's logits (or against
    reference(zdev) -> (loss, grad)); returns (zdev, loss, dlogits, reference loss, reference gradient)."""
    T = X.shape[0]
    atol = 2e-5 if T < 200 else 2e-4
    loss_rtol = 1e-6 if len(utt) == 1 else 2e-5
    zdev, eval_loss = _eval_pass(eng, X, utt, labels, lab)
    z64 = zdev.astype(np.float64)
    want_loss, want_grad, n_labels = ctc_batch(z64, utt, labels, lab, fast=True)
    sens = _sensitivity(zdev, utt, labels, lab, want_loss, want_grad)
    if reference is not None:
        want_loss, want_grad = reference(z64)
    if _rel(eval_loss, want_loss) > loss_rtol:  # (print the figures before the assertion stops the case)
        _report(name, utt, lab, sens, (_rel(eval_loss, want_loss), np.nan, np.nan))
    _loss_close(name + ": eval loss", eval_loss, want_loss, loss_rtol)
    loss, count, dlog = _train_pass(eng, X, utt, labels, lab)
    _report(name, utt, lab, sens, (_rel(eval_loss, want_loss), _rel(loss, want_loss), np.abs(dlog - want_grad).max()))
    _loss_close(name + ": training loss against the evaluation pass's", loss, eval_loss, 1e-6)
    _loss_close(name + ": loss", loss, want_loss, loss_rtol)
    assert count == n_labels == sum(lab)
    assert_close(name + ": dlogits", dlog, want_grad, rtol=1e-4, atol=atol)
    return zdev, loss, dlog, want_loss, want_grad


# ---- a. every register tile, the last states in lane 63 / straddling two lanes ----

@pytest.mark.parametrize("sharpen", [None, PEAKY], ids=["gentle", "peaky"])
@pytest.mark.parametrize("S", [63, 64, 127, 128, 255, 256, 511])
def test_every_register_tile(nets, S, sharpen):
    """three utterances: S labels over 2S + 40 frames; S labels, a quarter of them repeating their neighbour, over 3
    frames more than the shortest alignment needs; 5 labels over 20 frames, whose wave is almost idle.

    The row-sum assertion guards ctc_grad's normalisation itself, not the alpha / beta sweeps: ctc_grad divides the
    state posteriors of a frame by their sum (where that sum is within 1e-2 of one), so a row of dLogits sums to zero as
    far as the softmax row sums to one (36 classes: ~3e-7).  The sweeps are held by the loss and the dLogits
    comparisons; an offset or a log Z that is wrong leaves the band and shows in dLogits at its full size."""
    O = 36
    rng = np.random.default_rng(1000 + S)
    first, second, third = _labels(rng, S, O), _labels(rng, S, O, repeat=0.25), _labels(rng, 5, O)
    utt, lab = [2 * S + 40, _min_frames(second) + 3, 20], [S, S, 5]
    labels = np.concatenate([first, second, third])
    X = _frames(rng, sum(utt))
    eng = nets(O, sharpen)
    _, loss, dlog, want_loss, _ = _check("a tile S=%d %s" % (S, "peaky" if sharpen else "gentle"), eng, X, utt, labels, lab)
    assert np.isfinite(want_loss)
    assert np.abs(dlog.astype(np.float64).sum(axis=1)).max() < 1e-5  # softmax minus a distribution over the classes
    again = _train_pass(eng, X, utt, labels, lab)
    assert again[0] == loss and (again[2] == dlog).all()


def test_peaky_scale_30_repeat_heavy(nets):
    """9 classes, labels drawn from two of them (blanks are mandatory between most), logits of scale 30: most states
    sit at the kernel's finite minus infinity"""
    O = 9
    rng = np.random.default_rng(30)
    a, b = rng.integers(0, 2, size=20).astype(np.int32), rng.integers(0, 2, size=20).astype(np.int32)
    utt, lab = [_min_frames(a) + 5, 60], [20, 20]
    X = _frames(rng, sum(utt))
    _, _, dlog, want_loss, _ = _check("a scale 30 O=9", nets(O, (30.0, 3.0)), X, utt, np.concatenate([a, b]), lab)
    assert np.isfinite(want_loss)
    assert np.abs(dlog.astype(np.float64).sum(axis=1)).max() < 1e-5


# ---- b. exactly feasible: one alignment, the answer is known without the oracle ----

@pytest.mark.parametrize("sharpen", [None, PEAKY], ids=["gentle", "peaky"])
@pytest.mark.parametrize("S", [1, 63, 127, 255, 511])
def test_exactly_feasible_known_answer(nets, S, sharpen):
    """T = S + (number of equal neighbours): the only alignment emits every label once, with one blank between equal
    neighbours.  loss = -sum_t log softmax(z_t)[path_t], gradient = softmax - one-hot(path), formed directly in float64"""
    O = 36
    rng = np.random.default_rng(2000 + S)
    lab = _labels(rng, S, O, repeat=0.25)
    path = [int(lab[0])]
    for prev, cur in zip(lab[:-1], lab[1:]):
        path += [O - 1, int(cur)] if prev == cur else [int(cur)]
    T = len(path)
    assert T == _min_frames(lab)

    def known(z):
        lp = log_softmax(z)
        grad = np.exp(lp)
        grad[np.arange(T), path] -= 1.0
        return -lp[np.arange(T), path].sum(), grad
    _check("b exact S=%d %s" % (S, "peaky" if sharpen else "gentle"), nets(O, sharpen), _frames(rng, T), [T], lab, [S],
           reference=known)


# ---- c. frame counts around the prefetch ring (PFD = 8) ----

@pytest.mark.parametrize("sharpen", [None, PEAKY], ids=["gentle", "peaky"])
def test_frame_counts_around_the_prefetch_ring(nets, sharpen):
    O = 36
    rng = np.random.default_rng(3000)
    utt, lab, seqs = [], [], []
    for Tn in (1, 2, 3, 7, 8, 9, 10, 15, 16, 17, 18, 64, 65):
        for S in (0, 1, min(Tn, 4)):
            utt.append(Tn)
            lab.append(S)
            seqs.append(_labels(rng, S, O, distinct=True))  # distinct labels: feasible from T = S on
    X = _frames(rng, sum(utt))
    eng = nets(O, sharpen)
    tag = "peaky" if sharpen else "gentle"
    _, _, dlog, want_loss, _ = _check("c frames %s" % tag, eng, X, utt, np.concatenate(seqs), lab)
    assert np.isfinite(want_loss)
    # the same batch with the (Tn = 3, S = 3) utterance one frame short: its first two labels made equal
    short = next(i for i in range(len(utt)) if utt[i] == 3 and lab[i] == 3)
    seqs[short] = seqs[short].copy()
    seqs[short][1] = seqs[short][0]
    r0 = sum(utt[:short])
    _, loss2, dlog2, want2, _ = _check("c one short %s" % tag, eng, X, utt, np.concatenate(seqs), lab)
    assert want2 == np.inf and loss2 == np.inf
    assert not dlog2[r0:r0 + 3].any()
    keep = np.ones(len(X), dtype=bool)
    keep[r0:r0 + 3] = False
    assert (dlog2[keep] == dlog[keep]).all()


# ---- d. utterances without frames, more than one wave of utterances ----

def test_zero_frame_utterances(nets):
    from tfkaldi_amd import _lib
    O = 36
    rng = np.random.default_rng(4000)
    U, empty = 70, (0, 30, 31, 69)  # at the start, two in a row in the middle, at the end
    utt = [0 if u in empty else int(rng.integers(1, 5)) for u in range(U)]
    lab = [0 if u in empty else int(rng.integers(0, min(utt[u], 3) + 1)) for u in range(U)]
    assert sum(utt) < 200
    seqs = [_labels(rng, n, O, distinct=True) for n in lab]
    X = _frames(rng, sum(utt))
    eng = nets(O, None)
    _, _, dlog, want_loss, _ = _check("d zero-frame", eng, X, utt, np.concatenate(seqs), lab)
    assert np.isfinite(want_loss)
    # one of them with two labels: impossible, the batch loss is inf; every other utterance as before
    lab[31] = 2
    seqs[31] = _labels(rng, 2, O, distinct=True)
    _, loss2, dlog2, want2, _ = _check("d zero-frame S=2", eng, X, utt, np.concatenate(seqs), lab)
    assert want2 == np.inf and loss2 == np.inf
    assert (dlog2 == dlog).all()
    # and through the evaluation entry, where the average divides by the label count
    eng.eval_accumulate_ctc(X, utt, np.concatenate(seqs), lab)
    assert eng.scalar(_lib.NUM_FRAMES) == sum(lab)
    assert eng.eval_finish() == np.inf


# ---- e. the scratch stride shrinks and grows again on one engine ----

def test_scratch_stride_sequence(gpu):
    """max S = 5, 511, 5, 200 in this order: the stride of lp / alpha / beta is 128, 1024, 128, 512 floats while the
    buffers only ever grow.  One engine: the sequence through the evaluation entry, then through the training entry,
    which so starts on scratch that has already grown to its largest."""
    O = 36
    rng = np.random.default_rng(5000)
    batches = []
    for S in (5, 511, 5, 200):
        if S == 5 and batches:
            batches.append(batches[0])
            continue
        lab = [S, 3]
        labels = np.concatenate([_labels(rng, S, O), _labels(rng, 3, O)])
        utt = [2 * S + 9, 11]
        batches.append((_frames(rng, sum(utt)), utt, labels, lab))
    eng, _ = _make(O)
    refs = []
    for k, (X, utt, labels, lab) in enumerate(batches):
        zdev, loss = _eval_pass(eng, X, utt, labels, lab)
        want_loss, want_grad, _ = ctc_batch(zdev.astype(np.float64), utt, labels, lab, fast=True)
        print("ctc-edges e eval step %d S=%d: loss %.1e" % (k, max(lab), _rel(loss, want_loss)))
        _loss_close("e eval step %d" % k, loss, want_loss, 2e-5)
        refs.append((zdev, loss, want_loss, want_grad))
    assert refs[2][1] == refs[0][1] and (refs[2][0] == refs[0][0]).all()
    got = []
    for k, (X, utt, labels, lab) in enumerate(batches):
        zdev, eval_loss, want_loss, want_grad = refs[k]
        loss, count, dlog = _train_pass(eng, X, utt, labels, lab)
        sens = _sensitivity(zdev, utt, labels, lab, want_loss, want_grad)
        _report("e stride step %d" % k, utt, lab, sens, (_rel(eval_loss, want_loss), _rel(loss, want_loss),
                                                          np.abs(dlog - want_grad).max()))
        _loss_close("e step %d: training loss against the evaluation pass's" % k, loss, eval_loss, 1e-6)
        _loss_close("e step %d: loss" % k, loss, want_loss, 2e-5)
        assert count == sum(lab)
        assert_close("e step %d: dlogits" % k, dlog, want_grad, rtol=1e-4, atol=2e-5 if len(X) < 200 else 2e-4)
        got.append((loss, dlog))
    assert got[2][0] == got[0][0] and (got[2][1] == got[0][1]).all()
    eng.close()


# ---- f. the label limit ----

def test_label_limit(gpu):
    from tfkaldi_amd import _lib
    O = 36
    rng = np.random.default_rng(6000)
    eng, _ = _make(O)
    utt, lab = [40, 25], [9, 6]
    labels = np.concatenate([_labels(rng, n, O) for n in lab])
    X = _frames(rng, sum(utt))
    _, loss, dlog, _, _ = _check("f before the limit", eng, X, utt, labels, lab)
    eng.accumulate_ctc(X, utt, labels, lab)
    before = engine_grads(eng), eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES)
    assert before[1] == loss and before[2] == sum(lab)
    with pytest.raises(_lib.EngineError, match=r"512 labels.*limit 511"):
        eng.accumulate_ctc(_frames(rng, 600 + 25), [600, 25], np.concatenate([_labels(rng, 512, O, distinct=False),
                                                                               _labels(rng, 6, O)]), [512, 6])
    with pytest.raises(_lib.EngineError, match=r"limit 511"):
        eng.eval_accumulate_ctc(_frames(rng, 600), [600], _labels(rng, 512, O), [512])
    after = engine_grads(eng), eng.scalar(_lib.BATCH_LOSS), eng.scalar(_lib.NUM_FRAMES)
    assert after[1:] == before[1:]
    for k in before[0]:
        assert (after[0][k] == before[0][k]).all(), k
    _, loss2, dlog2, _, _ = _check("f after the limit", eng, X, utt, labels, lab)
    assert loss2 == loss and (dlog2 == dlog).all()
    eng.close()


# ---- g. the other arithmetics, the whole chain ----

def _rel_fro(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-30))


@pytest.mark.parametrize("case", ["medium", "peaky128"])
@pytest.mark.parametrize("dtype", ["float32_mfma", "bfloat16"])
def test_other_arithmetics_full_chain(gpu, dtype, case):
    """test_gpu_ctc.py's net (batch norm, tanh) on the exact fp32 matrix instructions and in mixed precision: loss, dLogits
    and every parameter gradient against make_pair's oracle of that arithmetic.  In bf16 mode the output layer's dW is
    computed from the bf16 twin of dLogits that ctc_grad writes: its gradient is the check on the twin.
    fp32: the tolerances of test_gpu_ctc.py; bf16: those of test_gpu_bf16_mode.py (relative Frobenius error <= 2e-3, loss
    rtol 5e-4)."""
    from tfkaldi_amd import _lib
    rng = np.random.default_rng(41)
    eng, oracle = make_pair(rng, max_frames=512, compute_dtype=dtype, **KW)
    O = KW["output_dim"]
    if case == "medium":  # 141 states: 4 per lane, as test_gpu_ctc.py's case of that name
        utt, lab = [210, 150], [70, 66]
    else:
        utt, lab = [2 * 128 + 40], [128]
        _sharpen(eng, rng, *PEAKY)
        oracle.W[oracle.L] = eng.get(_lib.WEIGHTS, eng.L).astype(np.float64)
        oracle.b[oracle.L] = eng.get(_lib.BIASES, eng.L).astype(np.float64)
    labels = np.concatenate([_labels(rng, n, O) for n in lab])
    T = sum(utt)
    X = _frames(rng, T)
    eng.accumulate_ctc(X, utt, labels, lab)
    loss, dlog, n_labels = ctc_batch(oracle.forward_logits(X), utt, labels, lab, fast=True)
    oracle.backward_from_dlogits(dlog, loss, n_labels)
    assert np.isfinite(loss)
    got_loss, got_dlog, got = eng.scalar(_lib.BATCH_LOSS), eng.debug_fetch(_lib.DBG_LOGITS, 0, T), engine_grads(eng)
    keys = [k for k in oracle.G if not (k.startswith("b") and not k.startswith("beta") and k != "b%d" % oracle.L)]
    print("ctc-edges g %-12s %-9s R %2d  T %4d  S max %3d | device: loss %.1e dlogits max %.1e fro %.1e | gradients fro %s"
          % (dtype, case, _tile(max(lab)), T, max(lab), _rel(got_loss, loss), np.abs(got_dlog - dlog).max(),
             _rel_fro(got_dlog, dlog), " ".join("%s %.1e" % (k, _rel_fro(got[k], oracle.G[k])) for k in keys)))
    assert eng.scalar(_lib.NUM_FRAMES) == sum(lab)
    if dtype == "bfloat16":
        np.testing.assert_allclose(got_loss, loss, rtol=5e-4)
        assert _rel_fro(got_dlog, dlog) <= 2e-3
        for k in keys:  # (bias under batch norm: true gradient 0, both sides hold round-off)
            assert _rel_fro(got[k], oracle.G[k]) <= 2e-3, (k, _rel_fro(got[k], oracle.G[k]))
    else:
        assert_close("batch_loss", got_loss, loss, 2e-5, 0)
        assert_close("dlogits", got_dlog, dlog, rtol=1e-4, atol=2e-4)
        for k in keys:
            want = oracle.G[k]
            assert_close("G[%s]" % k, got[k], want, rtol=1e-3, atol=2e-4 * max(np.abs(want).max(), 1e-3))
    eng.close()
