"""The forward-only pass -- what Nnet.decode writes for Kaldi, Decoder posteriors and Trainer.evaluate's validation loss -- at its
own edges, from the splice to the posteriors, in the style of tests/test_gpu_dnn_edges.py: float64 references evaluated on the
DEVICE's own fp32 input of the kernel under test.  One "decode-edges" line per case under `pytest -s`, headed by the library's
build id (recorded in profiles/decode_pass_edges.txt).

A. softmax_rows_kernel<NV> (kernels.hip), posteriors and log(posterior / prior): every register width full and one float4 past
   it, tails of 1 / 2 / 3 live columns, the generic kernel; the net of section A of the DNN edges file as initialised and PEAKED
   (every row's logits spread over more than 110, so that expf underflows on part of every row).  posteriors(raw_logits=True)
   gives the device's logits zdev (guard: a second call returns them bit for bit); both outputs of the same frames are compared
   with float64 on zdev.  The frames are the 19 of 304 candidates whose logit spreads are closest together: the peaked regime
   scales the output layer until the NARROWEST row spans 140, and a row of three logits that spans ten times as much would put
   lse near 600, where one fp32 ulp (6e-5) is already outside the earlier rule the bound below must respect.
   Posteriors: rtol 2e-5 + 2^-146 (8 spacings of the fp32 denormals -- the device keeps denormal results, see the table; the
   earlier atol 1e-9 hid every posterior below 5e-5); finite, >= 0, exactly +0 where expf underflows (z - max < -104.5).
   log(post / prior): the bound derived in tests/test_decode_edges_model.py from the kernel's operations,
   2^-23 (|z - lse| + |lse| + |log prior| + |want|) + 2^-24 (2 + 3 log O + additions of the row sum), never looser than the
   earlier 2e-5 + 2e-5 |want|; finite wherever the prior is positive, underflowed columns included; the float32 numpy
   restatement of the kernel's formula on the same zdev stays within half the bound (its worst error is printed beside the
   device's).  Priors: a normalised random one, and three with 1e-30, the smallest normal fp32 and exactly 1.0 rotated through
   column 0, column O - 1 and every slot of the last live float4; a zero prior gives +inf.
   Output layout through the C ABI with TFK_DEVICE_PTRS: 16-byte aligned rows (vector stores), an odd leading dimension and an
   `out` one float off alignment (element stores) agree bit for bit and leave a sentinel around them untouched; so does a host
   `out` with ldo = O + 3, pageable and pinned.
B. splice_kernel with device CMVN, bit for bit against host_splice of numpy's fp32 (x - mean) / std: raw dimensions that are no
   multiple of 4, padding columns of the staged input, context 0, the workload's own 40 x 11; a single one-frame utterance,
   empty utterances first, last and adjacent (their CMVN rows are NaN: reading one shows), 257 utterances of 1 or 2 frames;
   ldraw > D on the host and a column slice of a wider CUDA tensor; the evaluation entries (plain and stacked) and one training
   pass, plain and stacked (the stacked TRAINING pass is the one that scatters rows through out_seg).
C. Evaluation-mode hidden layers, TFK_FUSE_EVAL = 0 and 1 from the same parameters, three arithmetics: a moving variance of 0
   (rstd = 31.6, on a column wide enough to saturate sigmoid and tanh and to overflow expf) and of 1e8, |moving mean| = 30 on
   every other column, T = 1 .. 257, H = 130 and 33.  Unfused: DBG_BN_MEAN is the moving mean bit for bit, DBG_BN_RSTD within
   2 ulp of float64, DBG_HIDDEN against the float64 chain on DBG_PREACT at rtol 1e-4 + atol 2e-5.  Fused: within 2 ulp of the
   unfused output.  Saturated values exact on both paths: sigmoid 1 above u = 20 and +0 below -104 (expf(-u) = Inf), tanh +-1
   beyond |u| = 20.  (The padding columns [H, ldH) of a layer output are not reachable through tfk_debug_fetch, which copies H
   columns; what they could spoil -- the next layer's pre-activation, whose operand twins are read over the padded width -- is
   compared here layer by layer.)  The L2-norm chain, never fused, at the s > 1 kink against float64 on zdev.
D. loss_reduce_kernel over several evaluation micro-batches: T = 1 / 255 / 256 / 257 / 1025 alone and three passes before one
   eval_finish, against the float64 log-sum-exp on DBG_LOGITS, rtol 2e-5; the frame and micro-batch counts exact after every
   pass (read from the scalar bucket of a torch-state engine's reduce region: no scalar selector exposes the latter);
   keep_prob 0.7 drops nothing in evaluation.
E. The forward-only entries in the middle of a two-micro-batch training step leave parameters, Adam moments, moving averages,
   gradient sums and the step's loss / frame sums bit-identical, and the step finishes as on an engine that never evaluated."""
import ctypes
import os

import numpy as np
import pytest

from oracle.dnn_oracle import _nonlin
from test_bn_stats_model import BN_EPS, offset_layer
from test_decode_edges_model import (POST_ATOL, POST_RTOL, edge_prior, log_prior_reference, lse64, random_prior, rows_f32,
                                     softmax64, worst_ratio)
from test_gpu_device_splice import host_splice
from test_gpu_dnn_edges import NET_A, T_A, XENT_CASES, _engine, _forced_labels, _oracle, _rel, _width
from util import assert_close, batch, copy_oracle_to_engine, engine_grads, engine_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nets(gpu):
    """engines by (arithmetic, shape, TFK_FUSE_EVAL, tag), made on first use, shared by the cases of this file and closed at its
    end; every case loads its own parameters"""
    from tfkaldi_amd.build import library_id
    print("\ndecode-edges build id %s" % library_id())
    made = {}

    def get(dtype, fuse=None, tag=0, **kw):
        key = (dtype, fuse, tag) + tuple(sorted(kw.items()))
        if key not in made:
            old = os.environ.get("TFK_FUSE_EVAL")
            if fuse is not None:
                os.environ["TFK_FUSE_EVAL"] = fuse  # (read when the engine is created)
            try:
                made[key] = _engine(kw, dtype)
            finally:
                if fuse is not None:
                    if old is None:
                        del os.environ["TFK_FUSE_EVAL"]
                    else:
                        os.environ["TFK_FUSE_EVAL"] = old
        return made[key]
    yield get
    for eng in made.values():
        eng.close()


# ================= A. softmax_rows_kernel =================

def _similar_rows(z, n):
    """indices of the n rows of z whose spreads (max - min) are closest together"""
    spread = z.max(axis=1) - z.min(axis=1)
    order = np.argsort(spread)
    ratio = spread[order[n - 1:]] / spread[order[:len(order) - n + 1]]
    i = int(np.argmin(ratio))
    return np.sort(order[i:i + n])


def _softmax_setup(nets, dtype, O, regime):
    """(engine, frames, device logits) of a case of section A"""
    kw = dict(NET_A, output_dim=O)
    eng = nets(dtype, **kw)
    rng = np.random.default_rng(100 + O)
    oracle = _oracle(kw, dtype, rng)
    copy_oracle_to_engine(oracle, eng)
    cand = batch(rng, 16 * T_A, kw["input_dim"], O)[0]
    X = cand[_similar_rows(eng.posteriors(cand, raw_logits=True), T_A)]
    if regime == "peaked":
        z0 = eng.posteriors(X, raw_logits=True)
        factor = np.float32(140.0 / (z0.max(axis=1) - z0.min(axis=1)).min())
        for p in (oracle.W, oracle.b):
            p[oracle.L] = (p[oracle.L].astype(np.float32) * factor).astype(np.float64)
        copy_oracle_to_engine(oracle, eng)
    zdev = eng.posteriors(X, raw_logits=True).copy()
    assert (eng.posteriors(X, raw_logits=True) == zdev).all(), "the logits of two passes over the same frames"
    return eng, rng, X, zdev


@pytest.mark.parametrize("regime", ["initial", "peaked"])
@pytest.mark.parametrize("dtype,O", XENT_CASES, ids=["%s-%d" % c for c in XENT_CASES])
def test_softmax_rows_every_width(nets, dtype, O, regime):
    eng, rng, X, zdev = _softmax_setup(nets, dtype, O, regime)
    spread = zdev.max(axis=1) - zdev.min(axis=1)
    under = (zdev - zdev.max(axis=1, keepdims=True)) < -104.5  # expf is 0 below -103.98, half the smallest denormal
    if regime == "peaked":
        assert spread.min() > 110 and under.any(axis=1).all(), spread.min()
    # posteriors
    post, want = eng.posteriors(X).copy(), softmax64(zdev)
    tol = POST_RTOL * want + POST_ATOL
    r_post = float((np.abs(post - want) / tol).max())
    m_post = float((np.abs(rows_f32(zdev) - want) / tol).max())
    denormal = (post > 0) & (post < np.finfo(np.float32).tiny)
    # log(posterior / prior)
    priors = [("random", random_prior(rng, O))] + [("edges%d" % k, edge_prior(rng, O, k)) for k in range(3)]
    lines, outs = [], []
    for name, prior in priors:
        eng.set_prior(prior)
        ll = eng.posteriors(X, log_div_prior=True).copy()
        want_ll, bound = log_prior_reference(zdev, prior)
        assert (bound <= 2e-5 + 2e-5 * np.abs(want_ll)).all()
        outs.append((name, ll, want_ll, bound, worst_ratio(ll, want_ll, bound), worst_ratio(rows_f32(zdev, prior), want_ll, bound)))
        lines.append("%s %.2f (f32 model %.2f)" % (name, outs[-1][4], outs[-1][5]))
    nv, tail = _width(O)
    print("decode-edges A rows %-12s O %4d NV %d tail %d %-7s spread %5.1f..%5.1f underflow %5d denormal %4d | posteriors / tol "
          "%.2f (f32 model %.2f) | log(post / prior) / bound: %s" % (dtype, O, nv, tail, regime, spread.min(), spread.max(),
                                                                   int(under.sum()), int(denormal.sum()), r_post, m_post,
                                                                   "  ".join(lines)))
    assert np.isfinite(post).all() and (post >= 0).all()
    assert (post[under] == 0).all() and not np.signbit(post[under]).any()
    assert r_post <= 1, r_post
    assert np.abs(post.sum(axis=1) - 1).max() < 1e-5
    for name, ll, want_ll, bound, r_dev, r_model in outs:
        assert np.isfinite(ll).all(), name  # (underflowed columns included: the promise in the kernel's comment)
        assert r_model <= 0.5, (name, r_model)
        assert r_dev <= 1, (name, r_dev)


def test_softmax_rows_zero_prior_is_plus_infinity(nets):
    O = 1025
    eng, rng, X, zdev = _softmax_setup(nets, "float32", O, "initial")
    prior = random_prior(rng, O)
    zero = [0, 1023, O - 1]
    prior[zero] = 0.0
    eng.set_prior(prior)
    ll = eng.posteriors(X, log_div_prior=True)
    rest = np.setdiff1d(np.arange(O), zero)
    assert np.isposinf(ll[:, zero]).all() and np.isfinite(ll[:, rest]).all()


SENTINEL = np.float32(-7.25)


@pytest.mark.parametrize("O", [1025, 4094])
def test_softmax_rows_output_layouts(nets, O):
    """tfk_posteriors into caller-owned rows: vector stores, element stores (odd ldo, misaligned out), host rows with ldo > O"""
    import torch
    from tfkaldi_amd import _lib
    eng, rng, X, zdev = _softmax_setup(nets, "float32", O, "initial")
    eng.set_prior(random_prior(rng, O))
    T, F = X.shape
    Xd = torch.from_numpy(X).cuda()
    ld4 = (O + 3) // 4 * 4 + 4
    layouts = [("aligned", ld4, 0), ("odd ldo", O + 1, 0), ("out + 1 float", ld4, 1)]
    assert ld4 % 4 == 0 and (O + 1) % 4 != 0
    for flag, mode in ((0, "posteriors"), (_lib.LOG_DIV_PRIOR, "log(post / prior)")):
        want = eng.posteriors(X, log_div_prior=bool(flag)).copy()
        for name, ldo, off in layouts:
            buf = torch.full((off + T * ldo + 8,), float(SENTINEL), dtype=torch.float32, device="cuda")
            assert buf.data_ptr() % 16 == 0
            torch.cuda.synchronize()
            _lib.check(eng.lib.tfk_posteriors(eng._h, ctypes.c_void_p(Xd.data_ptr()), F, T,
                                              ctypes.c_void_p(buf.data_ptr() + 4 * off), ldo, flag | _lib.DEVICE_PTRS))
            eng.synchronize()
            flat = buf.cpu().numpy()
            rows = flat[off:off + T * ldo].reshape(T, ldo)
            assert (rows[:, :O] == want).all(), (mode, name)
            assert (rows[:, O:] == SENTINEL).all() and (flat[:off] == SENTINEL).all() and (flat[off + T * ldo:] == SENTINEL).all(), \
                (mode, name)
        for name in ("pageable", "pinned"):
            out = np.full((T, O + 3), SENTINEL, dtype=np.float32)
            if name == "pinned":
                keep = torch.from_numpy(out).pin_memory()
                out = keep.numpy()
            _lib.check(eng.lib.tfk_posteriors(eng._h, X.ctypes.data_as(ctypes.c_void_p), F, T, out.ctypes.data_as(ctypes.c_void_p),
                                              O + 3, flag))
            assert (out[:, :O] == want).all() and (out[:, O:] == SENTINEL).all(), (mode, name)
    print("decode-edges A layouts O %d | aligned / odd ldo / misaligned out / host ldo = O + 3 (pageable, pinned): bit-identical, "
          "sentinels untouched" % O)


# ================= B. splice and CMVN on the device =================

GEOMETRIES = [(1, 0), (3, 1), (13, 1), (13, 0), (5, 3), (40, 5)]
LISTS = ["one-frame", "empties", "many"]


def _utterance_list(rng, which, c):
    """(frames per utterance, utterances per micro-batch of the stacked calls)"""
    if which == "one-frame":
        return [1], [1]
    if which == "empties":  # a segment that starts and ends with an empty utterance; empty ones first, last and adjacent
        return [0, 3, 0, 0, 1, c, c + 1, 2 * c + 1, 0], [3, 3, 3]
    return list(rng.integers(1, 3, size=257)), [100, 100, 57]


@pytest.mark.parametrize("which", LISTS)
@pytest.mark.parametrize("D,c", GEOMETRIES, ids=["D%d-c%d" % g for g in GEOMETRIES])
def test_splice_and_cmvn_bit_identical(nets, D, c, which):
    import torch
    from tfkaldi_amd import _lib
    F = D * (2 * c + 1)
    kw = dict(input_dim=F, num_layers=2, num_units=32, output_dim=11, nonlin="relu", batch_norm=True, init_learning_rate=1e-3,
              num_steps=10, max_frames=512)
    a, b = nets("float32", **kw), nets("float32", tag=1, **kw)  # a: host-spliced frames, b: raw frames
    rng = np.random.default_rng(1000 * D + 10 * c + LISTS.index(which))
    oracle = _oracle(kw, "float32", rng)
    for e in (a, b):
        copy_oracle_to_engine(oracle, e)
    lens, seg_utts = _utterance_list(rng, which, c)
    U, T = len(lens), int(np.sum(lens))
    # frames of unit scale as they are, and -- for the CMVN table -- as features come: per-utterance scales of 0.5 .. 30 around
    # offsets of +-50 (the net then sees inputs of unit scale either way: a one-frame loss near 0 between logits near 100 would
    # put the comparison with float64 below the fp32 ulp of the logits)
    unit = [rng.standard_normal((n, D)).astype(np.float32) for n in lens]
    scale, offset = rng.uniform(0.5, 30.0, size=(len(lens), D)), rng.uniform(-50, 50, size=(len(lens), D))
    y = rng.integers(0, kw["output_dim"], size=T).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(seg_utts)])
    seg_rows = [int(np.sum(lens[first[i]:first[i + 1]])) for i in range(len(seg_utts))]
    assert all(r > 0 for r in seg_rows) and sum(seg_rows) == T
    cuts = np.concatenate([[0], np.cumsum(lens)])
    checked = []
    for with_cmvn in (False, True):
        table = None
        utts = normalised = unit
        if with_cmvn:
            utts = [(u * sc + off).astype(np.float32) for u, sc, off in zip(unit, scale, offset)]
            table = np.stack([np.stack([off + rng.standard_normal(D), sc * rng.uniform(0.8, 1.25, size=D)])
                              for sc, off in zip(scale, offset)]).astype(np.float32)
            normalised = [(u - t[0]) / t[1] for u, t in zip(utts, table)]  # numpy fp32 subtract and divide
            assert all(n.dtype == np.float32 for n in normalised)
            table[np.asarray(lens) == 0] = np.nan  # the rows of an empty utterance must not be read
        raw = np.concatenate(utts)
        X = np.concatenate([host_splice(n, c) for n in normalised])
        assert X.shape == (T, F) and np.isfinite(X).all()

        differ = []

        def same(name, got, want):  # (collected: one line names everything that differs)
            assert got.shape == want.shape, name
            if not (got == want).all():
                differ.append("%s: %d of %d elements, largest |got| %.3g |want| %.3g" % (
                    name, int((got != want).sum()), got.size, np.abs(got).max(), np.abs(want).max()))

        # decoding: hidden layer 0, logits, posteriors
        want_post = a.posteriors(X).copy()
        want_hid = a.debug_fetch(_lib.DBG_HIDDEN, 0, T)
        want_z = a.posteriors(X, raw_logits=True).copy()
        same("posteriors", b.posteriors_raw(raw, lens, c, cmvn=table), want_post)
        same("hidden 0", b.debug_fetch(_lib.DBG_HIDDEN, 0, T), want_hid)
        same("logits", b.posteriors_raw(raw, lens, c, raw_logits=True, cmvn=table), want_z)
        # a host matrix with ldraw = D + 3 through the C ABI, a CUDA column slice of a wider tensor
        wide = np.full((T, D + 3), np.nan, dtype=np.float32)
        wide[:, :D] = raw
        out = np.empty((T, b.O), dtype=np.float32)
        lens32 = np.asarray(lens, dtype=np.int32)
        _lib.check(b.lib.tfk_posteriors_raw(b._h, wide.ctypes.data_as(ctypes.c_void_p), D + 3, T, lens32.ctypes.data_as(ctypes.c_void_p),
                                            U, c, None if table is None else table.ctypes.data_as(ctypes.c_void_p),
                                            out.ctypes.data_as(ctypes.c_void_p), b.O, 0))
        same("posteriors, ldraw = D + 3", out, want_post)
        wide_d = torch.full((T, D + 5), float("nan"), dtype=torch.float32, device="cuda")
        wide_d[:, 2:2 + D] = torch.from_numpy(raw).cuda()
        same("posteriors, CUDA column slice", b.posteriors_raw(wide_d[:, 2:2 + D], lens, c, cmvn=table), want_post)
        # validation loss: plain and stacked raw entries
        a.zero_accumulators()
        a.eval_accumulate(X, y)
        loss_a = a.eval_finish()
        b.zero_accumulators()
        b.eval_accumulate_raw(raw, y, lens, c, cmvn=table)
        assert b.scalar(_lib.NUM_FRAMES) == T
        assert b.eval_finish() == loss_a
        b.zero_accumulators()
        b.eval_accumulate_stacked_raw(raw, y, lens, c, seg_utts, cmvn=table)
        assert b.scalar(_lib.NUM_FRAMES) == T
        loss_stacked = b.eval_finish()
        b.zero_accumulators()
        for i in range(len(seg_utts)):
            u0, u1 = first[i], first[i + 1]
            b.eval_accumulate_raw(raw[cuts[u0]:cuts[u1]], y[cuts[u0]:cuts[u1]], lens[u0:u1], c,
                                  cmvn=None if table is None else table[u0:u1])
        assert b.scalar(_lib.NUM_FRAMES) == T
        loss_segments = b.eval_finish()
        oracle.eval_accumulate(X, y)
        loss64 = oracle.eval_finish()
        assert abs(loss_stacked - loss_segments) <= 2e-6 * abs(loss_segments), (loss_stacked, loss_segments)
        assert_close("validation loss", loss_stacked, loss64, 2e-5, 0)
        # one training pass, plain and stacked (out_seg)
        a.zero_accumulators()
        a.accumulate(X, y)
        b.zero_accumulators()
        b.accumulate_raw(raw, y, lens, c, cmvn=table)
        for l in range(a.L):
            same("training hidden %d" % l, b.debug_fetch(_lib.DBG_HIDDEN, l, T), a.debug_fetch(_lib.DBG_HIDDEN, l, T))
        same("dLogits", b.debug_fetch(_lib.DBG_LOGITS, 0, T), a.debug_fetch(_lib.DBG_LOGITS, 0, T))
        assert a.scalar(_lib.BATCH_LOSS) == b.scalar(_lib.BATCH_LOSS) and b.scalar(_lib.NUM_FRAMES) == T
        ga, gb = engine_grads(a), engine_grads(b)
        for k in ga:
            same("gradient %s" % k, gb[k], ga[k])
        a.zero_accumulators()
        a.accumulate_stacked(X, y, seg_rows)
        b.zero_accumulators()
        b.accumulate_stacked_raw(raw, y, lens, c, seg_utts, cmvn=table)
        assert a.scalar(_lib.BATCH_LOSS) == b.scalar(_lib.BATCH_LOSS) and b.scalar(_lib.NUM_FRAMES) == T
        ga, gb = engine_grads(a), engine_grads(b)
        for k in ga:
            same("stacked gradient %s" % k, gb[k], ga[k])
        for e in (a, b):
            e.zero_accumulators()
        assert not differ, (with_cmvn, differ)
        checked.append("cmvn %d: loss stacked / segments %.1e, / float64 %.1e" % (with_cmvn, _rel(loss_stacked, loss_segments),
                                                                                 _rel(loss_stacked, loss64)))
    print("decode-edges B splice D %2d context %d F %3d %-9s U %3d T %3d | hidden 0, logits, posteriors, ldraw = D + 3, CUDA slice, "
          "validation loss, training pass (plain, stacked): bit-identical | %s" % (D, c, F, which, U, T, " | ".join(checked)))


# ================= C. evaluation-mode hidden layers =================

NET_C = dict(input_dim=20, num_layers=2, output_dim=13, init_learning_rate=1e-3, num_steps=10, max_frames=257)
CHAINS_C = [("relu", True), ("sigmoid", True), ("tanh", True), ("linear", True), ("tanh", False)]
ROWS_C = [1, 63, 64, 65, 129, 257]
EVAL_CASES = [(d, n, bn, H) for d in ("float32", "float32_mfma", "bfloat16") for n, bn in CHAINS_C for H in (130, 33)]
BIG_VAR_COL = 3


def _zero_var_cols(H):
    return [1, H - 1]  # (H - 1: the two-column tail of H = 130, the one-column tail of H = 33)


def _edge_net(kw, dtype, rng):
    """an oracle whose layer 0 has |mean| = 30 on every other column (offset_layer) with moving means to match, a moving variance
    of exactly 0 on two columns whose weights are four times as large (rstd = 31.6 turns a spread of 4 into 126: saturation, and
    expf(-u) = Inf) and of 1e8 on another; layer 1 has a zero-variance column as well"""
    oracle = _oracle(kw, dtype, rng)
    F, H = kw["input_dim"], kw["num_units"]
    W, b = offset_layer(rng, F, H, 1.5)
    W[:, _zero_var_cols(H)] *= 4.0
    oracle.W[0], oracle.b[0] = W.astype(np.float64), b.astype(np.float64)
    if oracle.bn:
        f = lambda v: v.astype(np.float32).astype(np.float64)
        oracle.mov_mean[0] = f(b + rng.standard_normal(H) * 0.1)
        oracle.mov_var[0] = f(1.0 + 0.2 * rng.random(H))
        oracle.mov_var[0][_zero_var_cols(H)] = 0.0
        oracle.mov_var[0][BIG_VAR_COL] = 1e8
        oracle.mov_var[1][1] = 0.0
    return oracle


def _eval_chain64(oracle, l, z):
    """(u, layer output before L2Norm) of hidden layer l in evaluation mode, float64 on the fp32 pre-activation z, with the fp32
    values the device holds: moving statistics, beta, eps = float32(1e-3)"""
    u = z.astype(np.float64)
    if oracle.bn:
        rstd = 1.0 / np.sqrt(oracle.mov_var[l] + BN_EPS)
        u = (u - oracle.mov_mean[l]) * rstd + oracle.beta[l]
    return u, _nonlin(u, oracle.nonlin)


@pytest.mark.parametrize("dtype,nonlin,bn,H", EVAL_CASES, ids=["%s-%s-bn%d-H%d" % c for c in EVAL_CASES])
def test_eval_layers_fused_and_unfused(nets, dtype, nonlin, bn, H):
    from tfkaldi_amd import _lib
    kw = dict(NET_C, num_units=H, nonlin=nonlin, batch_norm=bn)
    unfused, fused = nets(dtype, fuse="0", **kw), nets(dtype, fuse="1", **kw)
    rng = np.random.default_rng(7000 + H + len(nonlin))
    oracle = _edge_net(kw, dtype, rng)
    for e in (unfused, fused):
        copy_oracle_to_engine(oracle, e)
    L = kw["num_layers"]
    Xall = batch(rng, max(ROWS_C), kw["input_dim"], kw["output_dim"])[0]
    worst = dict(hidden=0.0, rstd=0.0, ulp=0, saturated=0, zeros=0)
    for T in ROWS_C:
        X = Xall[:T]
        post0 = unfused.posteriors(X).copy()
        post1 = fused.posteriors(X).copy()
        assert np.isfinite(post0).all() and np.isfinite(post1).all()
        for l in range(L):
            z = unfused.debug_fetch(_lib.DBG_PREACT, l, T)
            h0, h1 = unfused.debug_fetch(_lib.DBG_HIDDEN, l, T), fused.debug_fetch(_lib.DBG_HIDDEN, l, T)
            assert np.isfinite(z).all() and np.isfinite(h0).all() and np.isfinite(h1).all(), (T, l)
            if bn:
                mean_d = unfused.debug_fetch(_lib.DBG_BN_MEAN, l, T)[0]
                rstd_d = unfused.debug_fetch(_lib.DBG_BN_RSTD, l, T)[0]
                assert (mean_d == oracle.mov_mean[l].astype(np.float32)).all(), (T, l)
                want_rstd = 1.0 / np.sqrt(oracle.mov_var[l] + BN_EPS)
                ulps = np.abs(rstd_d - want_rstd) / np.spacing(want_rstd.astype(np.float32))
                worst["rstd"] = max(worst["rstd"], float(ulps.max()))
                assert ulps.max() <= 2, (T, l, ulps.max())
            u, want = _eval_chain64(oracle, l, z)
            worst["hidden"] = max(worst["hidden"], float(np.abs(h0 - want).max()))
            assert_close("hidden%d at T = %d" % (l, T), h0, want, 1e-4, 2e-5)
            np.testing.assert_array_max_ulp(h1, h0, maxulp=2)
            worst["ulp"] = max(worst["ulp"], int(np.abs(h1.view(np.int32).astype(np.int64) - h0.view(np.int32)).max()))
            if nonlin in ("sigmoid", "tanh"):
                hi, lo = u > 20, u < (-104 if nonlin == "sigmoid" else -20)
                if bn and l == 0 and T >= 63:  # the zero-variance columns saturate both ways (and expf(-u) overflows)
                    assert hi.any() and lo.any(), (T, float(u.min()), float(u.max()))
                floor = 0.0 if nonlin == "sigmoid" else -1.0
                for h in (h0, h1):
                    assert (h[hi] == 1.0).all() and (h[lo] == floor).all(), (T, l)
                    assert nonlin == "tanh" or not np.signbit(h[lo]).any(), (T, l)
                worst["saturated"] += int(hi.sum() + lo.sum())
                if nonlin == "sigmoid":
                    worst["zeros"] += int(lo.sum())
            if l + 1 < L:
                # the next layer's pre-activation from THIS output (padding columns of the output enter the contraction's
                # operand twins): finite, and the affine map of the layer output at the contraction's accuracy
                nxt = unfused.debug_fetch(_lib.DBG_PREACT, l + 1, T)
                ref = oracle._mm(h0.astype(np.float64), oracle.W[l + 1]) + oracle.b[l + 1]
                scale = np.abs(h0.astype(np.float64)).dot(np.abs(oracle.W[l + 1])) + np.abs(oracle.b[l + 1])
                assert (np.abs(nxt - ref) <= (2.0 ** -7 if dtype == "bfloat16" else 1e-5) * scale + 1e-30).all(), (T, l)
        np.testing.assert_array_max_ulp(post1, post0, maxulp=4) if dtype != "bfloat16" else \
            np.testing.assert_allclose(post1, post0, rtol=1e-5, atol=1e-8)
    print("decode-edges C eval %-12s %-7s bn %d H %3d T %s | unfused: hidden %.1e rstd %.2f ulp | fused - unfused %d ulp | "
          "saturated elements %d (sigmoid +0: %d)" % (dtype, nonlin, bn, H, ROWS_C, worst["hidden"], worst["rstd"], worst["ulp"],
                                                     worst["saturated"], worst["zeros"]))


L2_CASES = [(d, n, T) for d in ("float32", "float32_mfma", "bfloat16") for n in ("tanh", "relu") for T in (1, 65, 257)]


@pytest.mark.parametrize("dtype,nonlin,T", L2_CASES, ids=["%s-%s-%d" % c for c in L2_CASES])
def test_eval_l2_norm_chain(nets, dtype, nonlin, T):
    """tanh: every v^2 < 1, so the mean square s stays below the kink and L2Norm is the identity; relu: rows scaled by 0.3 .. 3 so
    that s straddles 1.  Rows whose float64 s lies within 1e-5 of 1 are excluded (at most 1 in 100)."""
    from tfkaldi_amd import _lib
    kw = dict(NET_C, num_units=130, nonlin=nonlin, batch_norm=True, l2_norm=True)
    eng = nets(dtype, **kw)
    rng = np.random.default_rng(8000 + T + len(nonlin))
    oracle = _oracle(kw, dtype, rng)
    copy_oracle_to_engine(oracle, eng)
    X = batch(rng, T, kw["input_dim"], kw["output_dim"])[0]
    X *= np.exp(rng.uniform(np.log(0.3), np.log(3.0), size=(T, 1))).astype(np.float32) if T > 1 else np.float32(2.0)
    post = eng.posteriors(X)
    assert np.isfinite(post).all()
    figures = []
    for l in range(kw["num_layers"]):
        z, hid = eng.debug_fetch(_lib.DBG_PREACT, l, T), eng.debug_fetch(_lib.DBG_HIDDEN, l, T)
        _, v = _eval_chain64(oracle, l, z)
        s = (v ** 2).mean(axis=1, keepdims=True)
        want = np.where(s > 1, v / s, v)
        near = np.abs(s[:, 0] - 1) < 1e-5
        assert near.sum() <= T / 100.0, int(near.sum())
        above = int((s > 1).sum())
        if l == 0:
            assert above == 0 if nonlin == "tanh" else (above > 0 and (above < T or T == 1)), (above, T)
        figures.append("layer %d: rows above the kink %d, excluded %d, hidden %.1e" % (l, above, int(near.sum()),
                                                                                      float(np.abs(hid - want)[~near].max())))
        assert_close("hidden%d" % l, hid[~near], want[~near], 1e-4, 2e-5)
    print("decode-edges C l2 %-12s %-4s T %3d | %s" % (dtype, nonlin, T, " | ".join(figures)))


# ================= D. validation loss over several micro-batches =================

NET_D = dict(input_dim=20, num_layers=2, num_units=32, output_dim=1025, nonlin="relu", batch_norm=True, init_learning_rate=1e-3,
             num_steps=10, max_frames=1025)
ROWS_D = [1, 255, 256, 257, 1025]


def _labels(rng, T, O):
    return _forced_labels(rng, max(T, 8), O)[:T]


def _loss64(z, y):
    return float((lse64(z)[:, 0] - z[np.arange(len(y)), y].astype(np.float64)).sum())


@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
def test_validation_loss_over_micro_batches(gpu, dtype):
    from tfkaldi_amd import _lib
    from tfkaldi_amd.engine import Engine
    kw, O = NET_D, NET_D["output_dim"]
    eng = Engine(_lib.make_config(max_frames=kw["max_frames"], seed=1234, compute_dtype=dtype,
                                  **{k: v for k, v in kw.items() if k != "max_frames"}), torch_state=True)
    rng = np.random.default_rng(9000)
    oracle = _oracle(kw, dtype, rng)
    copy_oracle_to_engine(oracle, eng)
    at = eng.buckets()[eng.L + 2][0]  # the bucket of the step's scalars: (loss sum, frames, micro-batches) lead it

    def sums():
        eng.synchronize()
        return eng.reduce_view()[at:at + 3].cpu().numpy().astype(np.float64)

    worst = 0.0
    for group in [[T] for T in ROWS_D] + [[255, 257, 1025]]:
        loss64, frames = 0.0, 0
        for i, T in enumerate(group):
            X, y = batch(rng, T, kw["input_dim"], O)[0], _labels(rng, T, O)
            eng.eval_accumulate(X, y)
            loss64 += _loss64(eng.debug_fetch(_lib.DBG_LOGITS, 0, T), y)
            frames += T
            got = sums()
            assert got[1] == frames == eng.scalar(_lib.NUM_FRAMES) and got[2] == i + 1, (group, got)
            assert_close("loss sum after pass %d of %s" % (i, group), got[0], loss64, 2e-5, 0)
        got = eng.eval_finish()
        worst = max(worst, _rel(got, loss64 / frames))
        assert_close("validation loss of %s" % group, got, loss64 / frames, 2e-5, 0)
        assert eng.scalar(_lib.NUM_FRAMES) == 0
    print("decode-edges D loss %-12s T %s and [255, 257, 1025] in a row | device / float64 on the device's logits %.1e, frame and "
          "micro-batch counts exact" % (dtype, ROWS_D, worst))
    eng.close()


def test_evaluation_drops_nothing(nets):
    """keep_prob = 0.7: dropout is the identity in evaluation mode -- the loss of the same parameters with keep_prob = 1, bit for bit"""
    kw, O = dict(NET_D, keep_prob=0.7), NET_D["output_dim"]
    drop, keep = nets("float32", **kw), nets("float32", **NET_D)
    rng = np.random.default_rng(9100)
    oracle = _oracle(NET_D, "float32", rng)
    for e in (drop, keep):
        copy_oracle_to_engine(oracle, e)
        e.zero_accumulators()
    losses = []
    for group in ([257], [255, 257, 1025]):
        data = [(batch(rng, T, kw["input_dim"], O)[0], _labels(rng, T, O)) for T in group]
        got = []
        for e in (drop, keep):
            for X, y in data:
                e.eval_accumulate(X, y)
            got.append(e.eval_finish())
        assert got[0] == got[1] and np.isfinite(got[0]), got
        losses.append(got[0])
    print("decode-edges D keep_prob 0.7 | validation loss %s: bit-identical to keep_prob 1" % losses)


# ================= E. the forward-only pass leaves the training state alone =================

@pytest.mark.parametrize("dtype", ["float32", "float32_mfma", "bfloat16"])
def test_forward_only_pass_inside_a_training_step(nets, dtype):
    from tfkaldi_amd import _lib
    D, c, O = 3, 1, 13
    kw = dict(input_dim=D * (2 * c + 1), num_layers=2, num_units=32, output_dim=O, nonlin="relu", batch_norm=True,
              init_learning_rate=1e-2, num_steps=10, max_frames=128)
    busy, plain = nets(dtype, **kw), nets(dtype, tag=1, **kw)  # busy evaluates in the middle of the step, plain never does
    rng = np.random.default_rng(9500)
    oracle = _oracle(kw, dtype, rng)
    lens = [7, 0, 30, 12]
    raw = rng.standard_normal((sum(lens), D)).astype(np.float32)
    Xv = np.concatenate([host_splice(raw[s:s + n], c) for s, n in zip(np.cumsum([0] + lens[:-1]), lens)])
    yv = rng.integers(0, O, size=len(Xv)).astype(np.int32)
    mbs = [batch(rng, T, kw["input_dim"], O) for T in (40, 33, 40, 33)]
    for e in (busy, plain):
        copy_oracle_to_engine(oracle, e)
        e.set_scalar(_lib.GLOBAL_STEP, 0)
        e.zero_accumulators()
        e.set_prior(np.full(O, 1.0 / O, dtype=np.float32))
        e.accumulate(*mbs[0])  # a first step, so that the Adam moments are not zero
        e.accumulate(*mbs[1])
        e.apply()
        e.accumulate(*mbs[2])

    def state(e):
        s = dict(engine_params(e))
        s.update(("grad " + k, v) for k, v in engine_grads(e).items())
        for l in range(e.L + 1):
            for kind, name in ((_lib.WEIGHTS, "W"), (_lib.BIASES, "b")):
                s["m %s%d" % (name, l)] = e.get(kind, l, _lib.SLOT_ADAM_M)
                s["v %s%d" % (name, l)] = e.get(kind, l, _lib.SLOT_ADAM_V)
        for l in range(e.L):
            s["mov_mean%d" % l], s["mov_var%d" % l] = e.get(_lib.BN_MOVING_MEAN, l), e.get(_lib.BN_MOVING_VAR, l)
            s["m beta%d" % l], s["v beta%d" % l] = e.get(_lib.BN_BETA, l, _lib.SLOT_ADAM_M), e.get(_lib.BN_BETA, l, _lib.SLOT_ADAM_V)
        s["loss sum"], s["frames"] = np.float64(e.scalar(_lib.BATCH_LOSS)), np.float64(e.scalar(_lib.NUM_FRAMES))
        return s

    before = state(busy)
    assert before["frames"] == 40 and any(v.any() for k, v in before.items() if k.startswith("m "))
    post = busy.posteriors(Xv).copy()
    busy.posteriors(Xv, log_div_prior=True)
    assert (busy.posteriors_raw(raw, lens, c) == post).all()
    busy.eval_accumulate(Xv[:20], yv[:20])
    z = [busy.debug_fetch(_lib.DBG_LOGITS, 0, 20)]
    busy.eval_accumulate(Xv[20:], yv[20:])
    z.append(busy.debug_fetch(_lib.DBG_LOGITS, 0, len(Xv) - 20))
    assert busy.scalar(_lib.NUM_FRAMES) == len(Xv)  # the evaluation's own count while it runs
    valid = busy.eval_finish()
    assert_close("validation loss inside the step", valid, _loss64(np.concatenate(z), yv) / len(Xv), 2e-5, 0)
    after = state(busy)
    for k in before:
        assert (before[k] == after[k]).all(), k
    for e in (busy, plain):
        e.accumulate(*mbs[3])
    loss_busy, loss_plain = busy.apply(), plain.apply()
    assert loss_busy == loss_plain and np.isfinite(loss_busy)
    end_busy, end_plain = state(busy), state(plain)
    for k in end_plain:
        assert (end_busy[k] == end_plain[k]).all(), k
    print("decode-edges E state %-12s | posteriors, log(post / prior), posteriors_raw, 2 x eval_accumulate + eval_finish (loss %.6f) "
          "inside a step: %d tensors and the step's sums bit-identical, step loss %.6f = the undisturbed engine's" % (
              dtype, valid, len(before) - 2, loss_busy))
